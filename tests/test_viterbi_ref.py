"""The NumPy Viterbi the GPU tests compare against (tests/viterbi_helpers.py), itself checked against
brute-force enumeration of all K^T paths; runs without a GPU."""
import numpy as np
import pytest

from tests.viterbi_helpers import brute_force, path_score, viterbi_batch, viterbi_numpy

K, T = 3, 6


def _random(seed):
    rng = np.random.default_rng(seed)
    ll = rng.normal(size=(T, K)) * 2
    mod_init = np.log(rng.dirichlet(np.ones(K)))
    ltran = np.log(rng.dirichlet(np.ones(K), size=K))
    return ll, mod_init, ltran


@pytest.mark.parametrize("seed", range(6))
def test_optimal_against_enumeration(seed):
    ll, mod_init, ltran = _random(seed)
    z, score = viterbi_numpy(ll, mod_init, ltran)
    best, arg = brute_force(ll, mod_init, ltran)
    assert len(arg) == 1 and tuple(z) == arg[0]
    assert score == best == path_score(z, ll, mod_init, ltran)      # same adds in the same order


def test_forbidden_transitions():
    ll, mod_init, ltran = _random(11)
    ltran[0, 1] = ltran[1, 2] = ltran[2, 0] = -np.inf
    mod_init[2] = -np.inf
    z, score = viterbi_numpy(ll, mod_init, ltran)
    best, arg = brute_force(ll, mod_init, ltran)
    assert np.isfinite(score) and score == best and tuple(z) in arg
    assert all(np.isfinite(ltran[a, b]) for a, b in zip(z[:-1], z[1:]))


def test_exact_ties_lowest_index_wins():
    """Integer-valued inputs: sums are exact, many paths tie.  The rule of the contract (first argmax at
    the end, first maximising predecessor at every step) singles out one of the optimal paths."""
    rng = np.random.default_rng(3)
    ll = rng.integers(-1, 2, size=(T, K)).astype(float)
    mod_init = np.zeros(K)
    ltran = rng.integers(-1, 1, size=(K, K)).astype(float)
    z, score = viterbi_numpy(ll, mod_init, ltran)
    best, arg = brute_force(ll, mod_init, ltran)
    assert len(arg) > 1                                    # the input really ties
    assert score == best and tuple(z) in arg
    # the rule, restated path by path: among the optimal paths take the lowest last state, then
    # going backwards the lowest predecessor that still continues an optimal prefix
    delta = np.empty((T, K))
    delta[0] = mod_init + ll[0]
    for t in range(1, T):
        delta[t] = (delta[t - 1][:, None] + ltran).max(0) + ll[t]
    want = [int(np.flatnonzero(delta[-1] == delta[-1].max())[0])]
    for t in range(T - 1, 0, -1):
        cand = delta[t - 1] + ltran[:, want[0]]
        want.insert(0, int(np.flatnonzero(cand == cand.max())[0]))
    assert list(z) == want
    # all-zero lliks under uniform transitions: everything ties, the path is all zeros
    z0, s0 = viterbi_numpy(np.zeros((T, K)), np.zeros(K), np.zeros((K, K)))
    assert not z0.any() and s0 == 0.0


def test_edges_and_batch():
    ll, mod_init, ltran = _random(5)
    z, s = viterbi_numpy(ll[:1], mod_init, ltran)
    assert z.tolist() == [int(np.argmax(mod_init + ll[0]))] and s == (mod_init + ll[0]).max()
    # an all -inf column decodes to predecessor 0 and a -inf score, without an error
    lt = np.full((K, K), -np.inf)
    z, s = viterbi_numpy(ll, mod_init, lt)
    assert s == -np.inf and z[:-1].tolist() == [0] * (T - 1) and z.dtype == np.int32
    zb, sb = viterbi_batch(np.stack([ll, ll[::-1]]), mod_init, ltran)
    assert zb.shape == (2, T) and sb.shape == (2,)
    assert tuple(zb[1]) == brute_force(ll[::-1], mod_init, ltran)[1][0]
