"""NumPy statements of the Viterbi recursion for the tests of svihmm_viterbi (host-side only).

``viterbi_numpy`` follows the operation order the C ABI fixes (include/svihmm.h): one add per
(i, j), a max over i in which the lowest index wins ties (np.argmax), one add of ll.  With identical
inputs the device result has to equal it bit for bit."""
import itertools

import numpy as np


def viterbi_numpy(ll, mod_init, ltran):
    """(z int32[T], score) of one window ``ll[T, K]``."""
    ll = np.asarray(ll, dtype=np.float64)
    ltran = np.asarray(ltran, dtype=np.float64)
    T, K = ll.shape
    delta = np.asarray(mod_init, dtype=np.float64) + ll[0]
    psi = np.zeros((T, K), dtype=np.int32)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            m = delta[:, None] + ltran              # m[i, j]: one add
            psi[t] = np.argmax(m, axis=0)           # first maximum
            delta = m[psi[t], np.arange(K)] + ll[t]  # the maximum itself, then one add
    z = np.empty(T, dtype=np.int32)
    z[T - 1] = np.argmax(delta)
    for t in range(T - 1, 0, -1):
        z[t - 1] = psi[t, z[t]]
    return z, float(delta[z[T - 1]])


def viterbi_batch(ll, mod_init, ltran):
    """``ll[B, Lm, K]`` -> (z int32[B, Lm], score float64[B])."""
    out = [viterbi_numpy(w, mod_init, ltran) for w in ll]
    return np.stack([o[0] for o in out]), np.array([o[1] for o in out])


def path_score(z, ll, mod_init, ltran):
    """log-score of the path ``z`` under (ll, mod_init, ltran), summed in path order."""
    z = np.asarray(z)
    s = mod_init[z[0]] + ll[0, z[0]]
    for t in range(1, len(z)):
        s = (s + ltran[z[t - 1], z[t]]) + ll[t, z[t]]
    return float(s)


def brute_force(ll, mod_init, ltran):
    """Best score over all K^T paths and every path that attains it (in lexicographic order)."""
    T, K = ll.shape
    best, arg = -np.inf, []
    for z in itertools.product(range(K), repeat=T):
        s = path_score(z, ll, mod_init, ltran)
        if s > best:
            best, arg = s, [z]
        elif s == best:
            arg.append(z)
    return best, arg
