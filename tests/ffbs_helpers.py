"""NumPy statements of the draw rule of svihmm_ffbs_windows (include/svihmm.h) for its tests; host-side only.

``draw`` is the rule for one step; ``backward_sample`` walks a window with it; ``check_paths`` recomputes
every step of device paths from the device's own lalpha rows, the path's own z[t+1] and the uniform, so one
discrepancy cannot cascade.  A step whose device state differs from NumPy's is *excused* only if the
threshold u * tot lies within EXCUSE * tot of the running sum c_j at every state j from the lower of the two
up to (not including) the higher one: the two sides then differ only in how exp and the sums rounded at
those boundaries (states of probability zero in between share one boundary).  Every other mismatch is an
error."""
import numpy as np

EXCUSE = 1e-11


def draw(la_row, logA_col, u):
    """Smallest k with u * tot <= c_k (K - 1 if none); ``logA_col`` is None at the window's last row.
    Returns (k, c, tot)."""
    lp = np.asarray(la_row, dtype=np.float64) if logA_col is None else la_row + logA_col
    p = np.exp(lp - lp.max())
    c = np.cumsum(p)                      # running sum in ascending state order
    tot = c[-1]
    hit = np.nonzero(u * tot <= c)[0]
    return (int(hit[0]) if hit.size else len(c) - 1), c, tot


def backward_sample(la, logA, u):
    """One path of a window: la [Lm, K], logA [K, K] used as logA[k, z_next], u [Lm]."""
    Lm = la.shape[0]
    z = np.empty(Lm, dtype=np.int32)
    z[Lm - 1] = draw(la[Lm - 1], None, u[Lm - 1])[0]
    for t in range(Lm - 2, -1, -1):
        z[t] = draw(la[t], logA[:, z[t + 1]], u[t])[0]
    return z


def _steps(z, la, logA, u):
    """Vectorised per-step recomputation: z, u [..., Lm], la broadcastable to [..., Lm, K].
    Returns (NumPy's state, c [..., Lm, K], thr, tot)."""
    z = np.asarray(z)
    K = la.shape[-1]
    lp = np.broadcast_to(la, z.shape + (K,)).astype(np.float64, copy=True)
    if z.shape[-1] > 1:
        lp[..., :-1, :] += logA.T[z[..., 1:]]          # logA[k, z[t+1]]
    p = np.exp(lp - lp.max(axis=-1, keepdims=True))
    c = np.cumsum(p, axis=-1)
    tot = c[..., -1]
    thr = u * tot
    hit = thr[..., None] <= c
    k = np.where(hit.any(axis=-1), hit.argmax(axis=-1), K - 1)
    return k, c, thr, tot


def check_paths(z, la, logA, u):
    """Device paths z [S, B, Lm] (or [B, Lm], [Lm]) against lalpha la [B, Lm, K] (or [Lm, K]) and the
    uniforms u (shape of z).  Returns the number of excused steps; raises AssertionError on any mismatch
    that is not excused, or a state outside [0, K)."""
    z = np.asarray(z)
    u = np.asarray(u, dtype=np.float64)
    assert z.shape == u.shape, (z.shape, u.shape)
    K = la.shape[-1]
    assert z.min() >= 0 and z.max() < K, "state outside [0, K)"
    k, c, thr, tot = _steps(z, la, logA, u)
    bad = np.argwhere(k != z)
    excused = 0
    for idx in map(tuple, bad):
        lo, hi = sorted((int(z[idx]), int(k[idx])))
        near = np.abs(thr[idx] - c[idx][lo:hi]) <= EXCUSE * tot[idx]      # every boundary between the two states
        assert near.all(), ("step %s: device state %d, NumPy %d, u*tot = %r, c = %r"
                           % (idx, z[idx], k[idx], thr[idx], c[idx]))
        excused += 1
    return excused


def near_boundary_steps(z, la, logA, u):
    """Steps at which u * tot is within EXCUSE * tot of some running sum (where an excuse could arise),
    and the smallest such distance relative to tot."""
    k, c, thr, tot = _steps(z, la, logA, np.asarray(u, dtype=np.float64))
    d = np.min(np.abs(c - thr[..., None]), axis=-1) / tot
    return int((d <= EXCUSE).sum()), float(d.min())
