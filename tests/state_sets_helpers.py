"""Allowed-state sets per row (svihmm_set_state_sets, ``set_state_sets`` of the batch classes): the clamp in NumPy, a
generator of sets none of which is infeasible, and the check that the generator yields the cases the tests rely on."""
import numpy as np


def clamp_sets(ll, allowed_rows):
    """``ll`` [..., K] with one bool row per llik row (``allowed_rows`` of ``ll.shape``): a copy that holds ``-inf``
    wherever the state is not allowed; the kept entries keep their bits."""
    ll = np.asarray(ll, dtype=np.float64)
    out = ll.copy()
    out[~np.asarray(allowed_rows, dtype=bool).reshape(ll.shape)] = -np.inf
    return out


def window_sets(allowed, starts, Lm):
    """The sets of the rows of the windows ``[s, s + Lm)``: bool [B, Lm, K]."""
    return np.stack([np.asarray(allowed)[int(s):int(s) + Lm] for s in np.asarray(starts).ravel()])


def singleton_labels(allowed):
    """int32 [T]: the state of a row whose set holds exactly one state, -1 elsewhere."""
    allowed = np.asarray(allowed, dtype=bool)
    return np.where(allowed.sum(axis=1) == 1, np.argmax(allowed, axis=1), -1).astype(np.int32)


def make_sets(ll, K, rng, frac=0.3, windows=None, full_window=None, masked_row=None, sts=None, inside=None):
    """bool [T, K] sets for the rows whose unclamped lliks are ``ll`` [T, K] (K >= 3).  About ``frac`` of the rows are
    constrained, always the first and last row of every window of ``windows`` (pairs (start, Lm)), every row of the
    window ``full_window`` and the row ``masked_row``.  A constrained row's set holds its generating state ``sts[t]``
    when ``sts`` is given, else the argmax of its llik row, plus 0 to 3 random others (never all K states) -- so no set
    is infeasible.  Four more rows, chosen among the rows ``inside`` (bool [T]; default: all) and distinct from the
    forced ones above: one whose set is that one state alone, one that allows all but its least likely state, one
    that allows state ``K - 1`` beside its best state, and for K > 64 one whose only allowed state lies in the last
    64-bit word (the row whose llik there is largest relative to its best state)."""
    ll = np.asarray(ll)
    T = ll.shape[0]
    best = (np.asarray(sts) % K).astype(np.int64) if sts is not None else np.argmax(ll, axis=1)
    pick = rng.random(T) < frac
    forced = np.zeros(T, bool)
    for s, Lm in (windows or ()):
        forced[int(s)] = forced[int(s) + Lm - 1] = True
    if full_window is not None:
        forced[int(full_window[0]):int(full_window[0]) + full_window[1]] = True
    if masked_row is not None:
        forced[int(masked_row)] = True
    pick |= forced
    allowed = np.ones((T, K), bool)
    nmax = min(3, K - 2)
    for t in np.flatnonzero(pick):
        row = np.zeros(K, bool)
        row[best[t]] = True
        others = np.delete(np.arange(K), best[t])
        row[rng.choice(others, size=int(rng.integers(0, nmax + 1)), replace=False)] = True
        allowed[t] = row
    free = (np.ones(T, bool) if inside is None else np.asarray(inside, bool).copy()) & ~forced
    rel = ll - ll.max(axis=1, keepdims=True)
    rel = np.where(np.isfinite(rel), rel, 0.0)               # (a masked row's lliks are all equal)

    def take(score):
        t = int(np.flatnonzero(free)[np.argmax(score[free])])
        free[t] = False
        return t
    t = take(np.zeros(T))                                     # a singleton
    allowed[t] = False
    allowed[t, best[t]] = True
    t = take(np.zeros(T))                                     # all but one state
    allowed[t] = True
    allowed[t, int(np.argmin(np.where(np.arange(K) == best[t], np.inf, ll[t])))] = False
    t = take(rel[:, K - 1])                                   # state K - 1 beside the best state
    allowed[t] = False
    allowed[t, [best[t], K - 1]] = True
    if K > 64:
        w0 = 64 * ((K - 1) // 64)
        t = take(rel[:, w0:].max(axis=1))                     # the last word only
        allowed[t] = False
        allowed[t, w0 + int(np.argmax(ll[t, w0:]))] = True
    return allowed


def check_cases(allowed, K, windows=None, full_window=None, masked_row=None, inside=None):
    """The cases ``make_sets`` promises, read from its result alone."""
    allowed = np.asarray(allowed)
    T = allowed.shape[0]
    assert allowed.shape == (T, K) and allowed.dtype == np.bool_
    n = allowed.sum(axis=1)
    assert n.min() >= 1
    con = n < K
    assert 0.2 < con.mean() < 0.7
    for s, Lm in (windows or ()):
        assert con[int(s)] and con[int(s) + Lm - 1]
    if full_window is not None:
        assert con[int(full_window[0]):int(full_window[0]) + full_window[1]].all()
    if masked_row is not None:
        assert con[int(masked_row)]
    ins = np.ones(T, bool) if inside is None else np.asarray(inside, bool)
    assert np.any(ins & (n == 1))
    assert np.any(ins & (n == K - 1))
    assert np.any(ins & con & allowed[:, K - 1])
    if K > 64:
        w0 = 64 * ((K - 1) // 64)
        assert np.any(ins & ~allowed[:, :w0].any(axis=1))
