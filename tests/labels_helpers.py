"""Partially labelled rows (svihmm_set_labels, ``set_labels`` of the batch classes): the clamp in NumPy and a label
generator whose labels are never infeasible."""
import numpy as np


def clamp(ll, labels_rows):
    """``ll`` [..., K] with one label per row (``labels_rows`` of ``ll.shape[:-1]``): a copy whose labelled rows hold
    ``-inf`` everywhere but at the label, whose entry keeps its bits."""
    ll = np.asarray(ll, dtype=np.float64)
    lab = np.asarray(labels_rows).reshape(ll.shape[:-1])
    out = ll.copy()
    k = np.arange(ll.shape[-1])
    out[(lab[..., None] >= 0) & (k != lab[..., None])] = -np.inf
    return out


def window_labels(labels, starts, Lm):
    """The labels of the rows of the windows ``[s, s + Lm)``: int [B, Lm]."""
    return np.stack([np.asarray(labels)[int(s):int(s) + Lm] for s in np.asarray(starts).ravel()])


def make_labels(ll, K, rng, frac=0.3, windows=None, full_window=None, masked_row=None, sts=None):
    """int32 [T] labels for the rows whose unlabelled lliks are ``ll`` [T, K]: about ``frac`` of the rows, always the
    first and last row of every window of ``windows`` (pairs (start, Lm)), every row of the window ``full_window``,
    the row ``masked_row`` and one row labelled ``K - 1``.  A label is the row's generating state ``sts[t]`` when
    ``sts`` is given, else the argmax of its llik row -- so no label is infeasible; the row labelled ``K - 1`` is the
    one whose llik of that state is largest relative to its best state."""
    ll = np.asarray(ll)
    T = ll.shape[0]
    best = (np.asarray(sts) % K).astype(np.int64) if sts is not None else np.argmax(ll, axis=1)
    pick = rng.random(T) < frac
    for s, Lm in (windows or ()):
        pick[int(s)] = pick[int(s) + Lm - 1] = True
    if full_window is not None:
        pick[int(full_window[0]):int(full_window[0]) + full_window[1]] = True
    if masked_row is not None:
        pick[int(masked_row)] = True
    lab = np.where(pick, best, -1).astype(np.int32)
    if not np.any(lab == K - 1):
        t = int(np.argmax(ll[:, K - 1] - ll.max(axis=1)))
        lab[t] = K - 1
    return lab
