"""NumPy statements of the window / buffer growth rule (include/svihmm.h, svihmm_grow_windows) and the
inputs the growth tests share.

``grow_direct`` is the rule as the reference runs it (hmmsgd_metaobs.py:521-661): one log-domain
forward / backward pass over the whole candidate window per candidate.  ``grow_products`` is the matrix
formulation the product kernel uses (nested candidates share F, Mid, R), rescaled by one exact power of two
per matrix and step."""
import numpy as np

from oracle import ref_numpy
from tests.helpers import make_problem

DBL_MAX = np.finfo(np.float64).max

# (K, D, T, seed, sep, stick, n, half0, m, inc, cutoff, eps, rule); F has explicit centres
CASES = {
    "A": (4, 2, 600, 11, .5, 20, 6, 5, 5, 1, 1000, 1e-5, 0),
    "B": (20, 3, 900, 12, .4, 40, 5, 2, 0, 3, 1000, 1e-5, 0),
    "C": (64, 4, 1500, 13, .4, 100, 4, 8, 8, 1, 1000, 1e-5, 0),
    "D": (64, 4, 1500, 13, .4, 100, 4, 1, 0, 1, 1000, 1e-5, 1),
    "E": (16, 3, 400, 14, .3, 60, 4, 3, 3, 2, 12, 1e-9, 0),
    "F": (16, 3, 400, 14, .3, 60, None, 2, 0, 1, 1000, 1e-9, 0),
    "G": (64, 32, 3000, 21, .15, 200, 3, 128, 128, 1, 1000, 1e-5, 0),
}
F_CENTERS = [4, 9, 392, 396]
# half-widths of the cases on the CPU (smallest, largest), as recorded with the rule's NumPy statement
EXPECTED_HALF = {"A": (13, 19), "B": (26, 41), "C": (27, 44), "D": (16, 28), "E": (13, 13), "G": (133, 140)}


def grow_problem(K, D, T, seed, sep, stick, miss=0):
    """A weak, sticky model (with make_problem's own transition counts growth stops after two or three
    steps).  The returned ``rng`` continues the stream the centres are drawn from."""
    p = make_problem(K, D, T, seed=seed, sep=sep, miss=miss)
    rng = np.random.default_rng(seed + 1)
    var_tran = 1 + stick * np.eye(K) + rng.random((K, K))
    p["var_tran"] = var_tran
    p["mod_init"], p["ltran"] = ref_numpy.psi_expectations(p["var_init"], var_tran)
    p["rng"] = rng
    return p


def grow_case(name, miss=0):
    """(problem, centers int64[n], dict of the rule's arguments) of case ``name``."""
    K, D, T, seed, sep, stick, n, half0, m, inc, cutoff, eps, rule = CASES[name]
    p = grow_problem(K, D, T, seed, sep, stick, miss=miss)
    if n is None:
        centers = np.array(F_CENTERS, dtype=np.int64)
    else:
        centers = (p["rng"].integers(0, T - 2 * half0 - 1, size=n) + half0).astype(np.int64)
    return p, centers, dict(half0=half0, m=m, inc=inc, cutoff=cutoff, eps=eps, rule=rule)


def niw_lliks(p, mask_as_nan=False):
    ll = ref_numpy.lliks_niw(p["obs"], p["mu"], p["sigma"], p["kappa"], p["nu"])
    if mask_as_nan:
        ll[p["mask"]] = 0.0
    return ll


def _rule(probes, T, c, half0, inc, cutoff, eps, rule, compared):
    """The growth rule around ``probes(b) -> (q_left, q_right)``."""
    b = half0
    ql, qr = probes(b)
    dl = dr = DBL_MAX
    count = 0
    run = np.zeros(2)
    old = np.zeros(2)
    trace = []
    while True:
        if c - b < 1 + inc or c + b + inc + 1 > T or b > cutoff:
            break
        if rule == 0:
            if compared is not None and trace:
                compared.extend([dl, dr])
            if dl < eps and dr < eps:
                break
        else:
            count += 1
            if count > 1:
                v = (run - old) / (count - 1)
                if compared is not None:
                    compared.extend(v.tolist())
                if v[0] < eps and v[1] < eps:
                    break
        b += inc
        nl, nr = probes(b)
        dl, dr = float(np.sum(np.abs(nl - ql))), float(np.sum(np.abs(nr - qr)))
        old = run.copy()
        run = run + (dl, dr)
        ql, qr = nl, nr
        trace.append((dl, dr))
    return b, np.array(trace, dtype=np.float64).reshape(-1, 2)


def grow_direct(ll, mod_init, ltran, T, c, half0, m, inc, cutoff, eps, rule, compared=None, row0=0):
    """``(half, trace[steps, 2])`` of centre ``c``: per candidate the posterior of the whole window
    [c - b, c + b] (oracle.ref_numpy forward_msgs / backward_msgs / posterior), probes at rows c - m, c + m.
    ``ll[t - row0]`` are the lliks of row t (all T rows with row0 = 0, or any range that covers the centre's
    reach).  ``compared`` (a list) collects every value the rule compares with ``eps``."""
    c = int(c)

    def probes(b):
        w = ll[c - b - row0:c + b + 1 - row0]
        q = ref_numpy.posterior(ref_numpy.forward_msgs(w, mod_init, ltran), ref_numpy.backward_msgs(w, ltran))
        return q[b - m].copy(), q[b + m].copy()
    return _rule(probes, T, c, half0, inc, cutoff, eps, rule, compared)


def _pow2_rescale(M):
    mx = M.max()
    return np.ldexp(M, -int(np.frexp(mx)[1])) if mx > 0 else M


def grow_products(ll, mod_init, ltran, T, c, half0, m, inc, cutoff, eps, rule, compared=None, row0=0):
    """The same rule on the shared matrices: G_t = A diag(e_t), F grows on the left, R on the right,
    Mid = G_{c-m+1} .. G_{c+m} once; q_left ~ (v' F) * (Mid R 1), q_right ~ (v' F Mid) * (R 1)."""
    c = int(c)
    K = ll.shape[1]
    A = np.exp(ltran)

    def G(t):
        r = ll[t - row0]
        return A * np.exp(r - r.max())[None, :]
    Mid = np.eye(K)
    for t in range(c - m + 1, c + m + 1):
        Mid = _pow2_rescale(Mid.dot(G(t)))
    state = {"b": m, "F": np.eye(K), "R": np.eye(K)}

    def probes(b):
        while state["b"] < b:
            bb = state["b"]
            state["F"] = _pow2_rescale(G(c - bb).dot(state["F"]))
            state["R"] = _pow2_rescale(state["R"].dot(G(c + bb + 1)))
            state["b"] = bb + 1
        x = mod_init + ll[c - b - row0]
        alpha = np.exp(x - x.max()).dot(state["F"])
        beta = state["R"].sum(1)
        ql = alpha * Mid.dot(beta)
        qr = alpha.dot(Mid) * beta
        return ql / ql.sum(), qr / qr.sum()
    return _rule(probes, T, c, half0, inc, cutoff, eps, rule, compared)


def grow_batch(fn, lls, row0s, mod_init, ltran, T, centers, trace_cap=0, **rule):
    """``fn`` (grow_direct / grow_products) over the centres -> ``(half int32[n], steps int32[n],
    trace [n, trace_cap, 2])``, the trace NaN-padded and truncated like the C ABI's.  ``lls[i]`` are lliks rows
    starting at absolute row ``row0s[i]`` that cover centre i's reach."""
    n = len(centers)
    half = np.empty(n, dtype=np.int32)
    steps = np.empty(n, dtype=np.int32)
    trace = np.full((n, trace_cap, 2), np.nan)
    for i, c in enumerate(centers):
        h, tr = fn(lls[i], mod_init, ltran, T, int(c), row0=int(row0s[i]), **rule)
        half[i], steps[i] = h, len(tr)
        k = min(len(tr), trace_cap)
        trace[i, :k] = tr[:k]
    return half, steps, trace


def reach_windows(centers, T, half0, inc, cutoff):
    """The product route's emission pass (include/svihmm.h): ``(starts int64[n], W)`` of the n windows of one
    common length that cover every row a centre can reach."""
    centers = np.asarray(centers, dtype=np.int64)
    lim = np.minimum(np.minimum(centers - 1 - inc, T - centers - inc - 1), cutoff)
    smax = np.where(lim >= half0, (lim - half0) // inc + 1, 0)
    R = int(max(half0, np.max(half0 + smax * inc)))
    W = min(2 * R + 1, T)
    return np.clip(centers - R, 0, T - W), W
