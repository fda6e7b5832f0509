"""Poisson count emissions, host side: the ``ProductPoisson`` plugin against numerical integrals of its Gamma
factors, the conjugate update, the helpers' statement of the contract loop, the batch class on the oracle engine
(host-lliks route), the packed view, the C-ABI prototype and the CPU-side preconditions of the GPU tests.  No GPU."""
import itertools

import numpy as np
import pytest
from scipy import integrate, stats

from pysvihmm_amd import _lib, hmmbatchcd
from pysvihmm_amd.distributions import ProductPoisson
from pysvihmm_amd.engine import PackedPoissonStats, rewrap_packed
from oracle.engine import OracleEngine

from tests import poisson_helpers as H
from tests.decode_sequences_helpers import near_boundary_sequences
from tests.grow_helpers import grow_direct


def test_signature_and_limits():
    assert "svihmm_set_emission_poisson" in _lib.SIGNATURES
    assert _lib.POISSON_MAX_D == 128 and _lib.POISSON_MAX_COUNT == (1 << 20) - 1


def _factor(rng, D, max_count=4095):
    return ProductPoisson(rng.random(D) * 3 + 0.5, rng.random(D) * 2 + 0.5, alpha_mf=rng.random(D) * 30 + 1.0,
                          beta_mf=rng.random(D) * 5 + 0.5, max_count=max_count)


def test_expected_log_likelihood_of_single_entries_against_quadrature():
    rng = np.random.default_rng(0)
    D = 3
    p = _factor(rng, D)
    for d in range(D):
        a, b = p.alpha_mf[d], p.beta_mf[d]
        for c in (0, 1, 7, 40):
            x = np.full((1, D), np.nan)
            x[0, d] = c
            want = integrate.quad(lambda lam: stats.gamma.pdf(lam, a, scale=1 / b) * stats.poisson.logpmf(c, lam),
                                  0, np.inf, epsabs=0, epsrel=1e-12, limit=400)[0]
            got = p.expected_log_likelihood(x)[0]
            assert abs(got - want) <= 1e-9 * abs(want), (d, c, got, want)


def test_get_vlb_against_quadrature():
    rng = np.random.default_rng(1)
    D = 3
    p = _factor(rng, D)
    want = 0.0
    for d in range(D):
        q = stats.gamma(p.alpha_mf[d], scale=1 / p.beta_mf[d])
        pr = stats.gamma(p.alpha_0[d], scale=1 / p.beta_0[d])
        lo, hi = q.ppf(1e-300), q.isf(1e-300)
        want -= integrate.quad(lambda lam: q.pdf(lam) * (q.logpdf(lam) - pr.logpdf(lam)), lo, hi, epsabs=0,
                               epsrel=1e-12, limit=400, points=[q.mean()])[0]
    assert abs(p.get_vlb() - want) <= 1e-8 * abs(want)
    assert p.num_parameters() == D


def test_meanfieldupdate_is_the_conjugate_update_and_skips_absent_entries():
    rng = np.random.default_rng(2)
    D, n = 4, 50
    p = _factor(rng, D, max_count=30)
    x = rng.poisson(6.0, size=(n, D)).astype(float)
    x[rng.random((n, D)) < 0.2] = np.nan
    x[3] = np.nan
    x[4, 0], x[5, 1], x[6, 2], x[7, 3], x[8, 0], x[9, 1] = 31.0, -1.0, np.inf, -0.5, 3.7, 30.0
    sx, cnt = np.zeros(D), np.zeros(D)
    for t in range(n):
        for d in range(D):
            v = x[t, d]
            if v == v and 0.0 <= v < 31.0:
                sx[d] += int(v)
                cnt[d] += 1
    p.meanfieldupdate(x, np.ones(n))
    np.testing.assert_allclose(p.alpha_mf, p.alpha_0 + sx, rtol=1e-14)
    np.testing.assert_allclose(p.beta_mf, p.beta_0 + cnt, rtol=1e-14)
    np.testing.assert_allclose(p.rates, p.alpha_mf / p.beta_mf, rtol=1e-14)
    w = rng.random(n)
    got = p._get_weighted_statistics(x, w)
    np.testing.assert_allclose(np.concatenate(got), H.poisson_stats(x, None, 30, w[:, None])[0], rtol=1e-13)
    assert p.rvs(5).shape == (5, D)


def test_helper_loop_equals_the_class_bit_for_bit():
    rng = np.random.default_rng(3)
    x, _ = H.make_data(300, 5, 4095, rng, lam=np.exp(rng.uniform(-2, 5, size=(4, 5))))
    p = _factor(rng, 5)
    elog, erate = p.expected_tables()
    want = H.poisson_lliks(x, None, elog[None], erate[None], H.logfact_table(4095))[:, 0]
    got = p.expected_log_likelihood(x)
    _, ok = H.present(x, 4095)
    dead = ~ok.any(1)
    assert dead.sum() >= 2 and np.all(np.isnan(got[dead])) and np.all(want[dead] == 0.0)
    np.testing.assert_array_equal(got[~dead], want[~dead])
    # 3.7 counts as 3; +inf, -0.5, -1 and C + 1 are absent
    c, ok = H.present(np.array([[3.7, np.inf, -0.5, -1.0, 4096.0, 4095.0, np.nan, -0.0]]), 4095)
    assert ok.tolist() == [[True, False, False, False, False, True, False, True]]
    assert c[0, 0] == 3 and c[0, 5] == 4095 and c[0, 7] == 0


def test_batchcd_on_the_oracle_engine_recovers_planted_rates():
    """The engine without the family keeps the host-lliks route: the literal loop through the plugin."""
    K, D, T = 3, 4, 600
    rng = np.random.default_rng(7)
    lam = np.array([[1.0, 20.0, 5.0, 60.0], [12.0, 2.0, 40.0, 5.0], [40.0, 60.0, 0.5, 20.0]])
    sts = np.repeat(rng.integers(0, K, size=T // 20 + 1), 20)[:T]
    obs = rng.poisson(lam[sts]).astype(float)
    obs[rng.random((T, D)) < 0.03] = np.nan
    np.random.seed(3)
    # the start knows nothing of the planted rates: K complete data rows, the first drawn at random, each next one the
    # farthest (in square-root counts) from those taken; weak priors
    full = obs[~np.isnan(obs).any(1)]
    r = np.sqrt(full)
    pick = [int(rng.integers(len(full)))]
    while len(pick) < K:
        pick.append(int(np.argmax(np.min([((r - r[i]) ** 2).sum(1) for i in pick], axis=0))))
    emit = np.array([ProductPoisson(np.ones(D), np.full(D, 0.1), alpha_mf=full[i] + 0.5, beta_mf=np.ones(D))
                     for i in pick])
    m = hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), emit, mask=np.zeros(T, bool), maxit=3, engine=OracleEngine())
    assert not m._poisson_fastpath() and not m._device_family()
    m.infer(fused=False)
    got = np.stack([e.rates for e in m.var_emit])
    # (the states come back in the order of the picked rows: match them to the planted ones)
    err = min(np.abs(got[list(p)] / lam - 1.0).max() for p in itertools.permutations(range(K)))
    assert err <= 0.2, err


def test_packed_poisson_stats_slicing():
    K, D = 3, 4
    assert PackedPoissonStats.size(K, D) == K * K + 2 * K * D + 1
    buf = np.arange(PackedPoissonStats.size(K, D), dtype=float)
    st = PackedPoissonStats(buf, K, D)
    assert not hasattr(st, "counts") and not hasattr(st, "col_counts")
    assert st.A_raw.shape == (K, K) and st.flat.shape == (K, 2 * D) and st.sx.shape == st.n.shape == (K, D)
    assert st.sx[1, 2] == K * K + 2 * D + 2 and st.n[1, 2] == K * K + 2 * D + D + 2 and st.lb[0] == buf[-1]
    st.n[2, 3] = -7.0                        # views, not copies
    assert buf[K * K + 2 * 2 * D + D + 3] == -7.0
    st2 = rewrap_packed(st, buf * 2)
    assert type(st2) is PackedPoissonStats and st2.D == D and st2.sx[1, 2] == 2 * st.sx[1, 2]


@pytest.mark.parametrize("i", range(5), ids=H.IDS[:5])
def test_ffbs_seed_of_the_gpu_test_has_no_step_near_a_boundary(i):
    la, u, z, off = H.ffbs_reference(i)
    assert near_boundary_sequences(z, la, H.problem(i)["ltran"], u, off) == 0


def test_grow_case_of_the_gpu_test_keeps_its_margin():
    p, Tg = H.grow_case()
    ll = H.lliks_of(p, mask=None)
    compared, halves = [], []
    for c in H.GROW_CENTERS:
        halves.append(grow_direct(ll, p["mod_init"], p["ltran"], Tg, int(c), compared=compared, **H.GROW_RULE)[0])
    compared = np.array(compared)
    eps = H.GROW_RULE["eps"]
    assert len(compared) and np.all((compared < eps / 3) | (compared > eps * 3))
    assert len(set(halves)) > 1
