"""Gaussian tracks with missing entries, host side: the ``ProductGaussian`` plugin against ``DiagonalGaussian`` (complete
data, and column by column with missing entries), the origin of the statistics, the helpers' statement of the contract
loop, the batch class on the oracle engine (host-lliks route), the packed view, the C-ABI prototype and the CPU-side
preconditions of the GPU tests.  No GPU."""
import numpy as np

from pysvihmm_amd import _lib, hmmbatchcd
from pysvihmm_amd.distributions import DiagonalGaussian, ProductGaussian
from pysvihmm_amd.engine import PackedGaussTrackStats, PackedPoissonStats, rewrap_packed
from pysvihmm_amd.hmmbase import is_diag_gaussian
from oracle.engine import OracleEngine

from tests import pgauss_helpers as H

PIN = 1e-10         # the project's pin level for two host statements of one formula (cf. the SciPy pin)


def test_signature_and_limits():
    assert "svihmm_set_emission_pgauss" in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["svihmm_set_emission_pgauss"][1]) == 7
    assert _lib.PGAUSS_MAX_D == 128 and _lib.PGAUSS_ABSENT == 1e150


def _pair(rng, D, loc=0.0):
    """A DiagonalGaussian and a ProductGaussian with one prior and one mean-field factor."""
    np.random.seed(int(rng.integers(1 << 30)))
    kw = dict(mu_0=loc + rng.normal(size=D), nus_0=rng.uniform(0.05, 2.0, size=D), alphas_0=rng.uniform(1.0, 4.0, size=D),
              betas_0=rng.uniform(0.5, 4.0, size=D))
    a, b = DiagonalGaussian(**kw), ProductGaussian(**kw)
    mf = (loc + rng.normal(size=D), rng.uniform(1.0, 30.0, size=D), rng.uniform(2.0, 20.0, size=D),
          rng.uniform(1.0, 40.0, size=D))
    a._set_mf(*[m.copy() for m in mf])
    b._set_mf(*[m.copy() for m in mf])
    return a, b


def _mf(g):
    return g.mf_mu, g.mf_nus, g.mf_alphas, g.mf_betas


def test_complete_data_equals_diagonal_gaussian():
    rng = np.random.default_rng(0)
    D, n = 6, 200
    a, b = _pair(rng, D)
    assert not is_diag_gaussian(b) and is_diag_gaussian(a)       # the device's diagonal family is not taken for it
    x = rng.normal(size=(n, D)) * 2.0 + 1.0
    np.testing.assert_allclose(b.expected_log_likelihood(x), a.expected_log_likelihood(x), rtol=PIN)
    np.testing.assert_allclose(b.get_vlb(), a.get_vlb(), rtol=PIN)
    w = rng.random(n)
    a.meanfieldupdate(x, w)
    b.meanfieldupdate(x, w)
    for got, want in zip(_mf(b), _mf(a)):
        np.testing.assert_allclose(got, want, rtol=PIN)
    np.testing.assert_allclose(b.sigmas, a.sigmas, rtol=PIN)
    np.testing.assert_allclose(b.get_vlb(), a.get_vlb(), rtol=PIN)
    np.testing.assert_allclose(b.expected_log_likelihood(x), a.expected_log_likelihood(x), rtol=PIN)
    eta = b.to_natural(*_mf(b))
    for got, want in zip(b.from_natural(eta), _mf(b)):
        np.testing.assert_allclose(got, want, rtol=1e-12)


def test_update_of_a_column_is_the_diagonal_update_on_its_present_rows():
    rng = np.random.default_rng(1)
    D, n = 5, 300
    a, b = _pair(rng, D)
    x = rng.normal(size=(n, D)) * 3.0 - 2.0
    x[rng.random((n, D)) < 0.15] = np.nan
    x[7, 1], x[8, 2], x[9, 3], x[10, 4], x[11, 0] = np.inf, -np.inf, 1e308, -1e200, 1e150
    x[12] = np.nan
    x[:, 3] = np.where(rng.random(n) < 0.5, np.nan, x[:, 3])
    w = rng.random(n)
    ok = H.present(x)
    assert not ok[11, 0] and not ok[12].any() and np.array_equal(ok, b._present(x)[1])
    b.meanfieldupdate(x, w)
    for d in range(D):
        c = DiagonalGaussian(mu_0=a.mu_0[d:d + 1], nus_0=a.nus_0[d:d + 1], alphas_0=a.alphas_0[d:d + 1],
                             betas_0=a.betas_0[d:d + 1])
        c.meanfieldupdate(x[ok[:, d], d][:, None], w[ok[:, d]])
        for got, want in zip(_mf(b), _mf(c)):
            np.testing.assert_allclose(got[d], want[0], rtol=PIN)
    # the statistics are the helpers'
    n_, sx, sxx, o = b._get_weighted_statistics(x, w)
    np.testing.assert_allclose(np.concatenate([sxx, sx, n_]), H.pgauss_stats(x, None, o, w[:, None])[0], rtol=1e-13)
    np.testing.assert_array_equal(o, H.data_origin(x))
    assert b.rvs(5).shape == (5, D) and np.isnan(b.rvs(400, missing=0.5)).mean() > 0.3


def test_two_origins_give_one_posterior_for_data_far_from_zero():
    """Data at mean 1e6, spread 1: sxx about the column means is O(n), about zero it is O(n 1e12) and sxx - sx^2 / n
    loses six digits there -- the stable form still agrees to 1e-9 from a nearby origin, which is why the origin exists."""
    rng = np.random.default_rng(2)
    D, n = 4, 500
    _, b = _pair(rng, D, loc=1e6)
    x = 1e6 + rng.normal(size=(n, D))
    x[rng.random((n, D)) < 0.1] = np.nan
    w = rng.random(n)
    o1 = b.data_origin(x)
    o2 = o1 + rng.normal(size=D) * 3.0
    h1 = b._posterior_hypparams(*b._get_weighted_statistics(x, w, origin=o1))
    h2 = b._posterior_hypparams(*b._get_weighted_statistics(x, w, origin=o2))
    for got, want in zip(h2, h1):
        np.testing.assert_allclose(got, want, rtol=1e-9)
    # the same statistics about zero: betas_n is off by far more than that
    h0 = b._posterior_hypparams(*b._get_weighted_statistics(x, w, origin=np.zeros(D)))
    assert np.max(np.abs(h0[3] / h1[3] - 1.0)) > 1e-7
    # and the centred betas_n is what two-pass arithmetic gives
    ok = H.present(x)
    for d in range(D):
        xd, wd = x[ok[:, d], d], w[ok[:, d]]
        m = np.sum(wd * xd) / wd.sum()
        ss = np.sum(wd * (xd - m) ** 2)
        want = b.betas_0[d] + 0.5 * (ss + b.nus_0[d] * wd.sum() / (b.nus_0[d] + wd.sum()) * (m - b.mu_0[d]) ** 2)
        np.testing.assert_allclose(h1[3][d], want, rtol=1e-9)


def test_all_absent_column_returns_the_prior():
    rng = np.random.default_rng(3)
    D, n = 3, 40
    _, b = _pair(rng, D)
    x = rng.normal(size=(n, D))
    x[:, 1] = [(np.nan, np.inf, -1e200)[t % 3] for t in range(n)]
    b.meanfieldupdate(x, rng.random(n))
    prior = (b.mu_0, b.nus_0, b.alphas_0, b.betas_0)
    for got, want in zip(_mf(b), prior):
        assert got[1] == want[1] and got[0] != want[0]
    assert np.all(np.isfinite(np.concatenate(_mf(b))))


def test_helper_loop_equals_the_class_bit_for_bit():
    rng = np.random.default_rng(4)
    p = H.make_model(4, 5, rng)
    x, _ = H.make_data(300, 5, rng, p["means"], p["sig"])
    _, b = _pair(rng, 5, loc=1e3)
    mu, hprec, cst = b.expected_tables()
    np.testing.assert_array_equal(np.stack([mu, hprec, cst]), np.stack(H.tables(*_mf(b))))
    want = H.pgauss_lliks(x, None, mu[None], hprec[None], cst[None])[:, 0]
    got = b.expected_log_likelihood(x)
    dead = ~H.present(x).any(1)
    assert dead.sum() >= 2 and np.all(np.isnan(got[dead])) and np.all(want[dead] == 0.0)
    assert not np.any(np.signbit(want[dead]))
    np.testing.assert_array_equal(got[~dead], want[~dead])
    ok = H.present(np.array([[np.nan, np.inf, -np.inf, 1e150, -1e150, np.nextafter(1e150, 0), -0.0, 1e308, -1e200]]))
    assert ok.tolist() == [[False, False, False, False, False, True, True, False, False]]


def test_batchcd_on_the_oracle_engine_elbo_does_not_decrease():
    """The engine without the family keeps the host-lliks route: the literal loop through the plugin is coordinate
    ascent, so the ELBO does not decrease (to 1e-8 relative) over 5 iterations."""
    K, D, T = 3, 4, 400
    rng = np.random.default_rng(7)
    means = 1e3 + rng.normal(size=(K, D)) * 4.0
    sts = np.repeat(rng.integers(0, K, size=T // 20 + 1), 20)[:T]
    obs = means[sts] + rng.normal(size=(T, D))
    obs[rng.random((T, D)) < 0.15] = np.nan
    obs[5] = np.nan
    np.random.seed(3)
    emit = np.array([ProductGaussian(mu=obs[np.where(~np.isnan(obs).any(1))[0][7 * k]].copy(), sigmas=np.full(D, 4.0),
                                     mu_0=np.full(D, 1e3), nus_0=0.01, alphas_0=2.0, betas_0=2.0) for k in range(K)])
    m = hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), emit, mask=np.zeros(T, bool), maxit=5, engine=OracleEngine())
    assert not m._pgauss_fastpath() and not m._device_family()
    m.infer(fused=False)
    e = m.elbo_vec
    assert len(e) == 5 and np.all(np.isfinite(e))
    assert np.all(np.diff(e) >= -1e-8 * np.abs(e[:-1])), e
    got = np.stack([g.mf_mu for g in m.var_emit])
    assert np.all(np.isfinite(got))


def test_packed_gauss_track_stats_slicing():
    K, D = 3, 4
    assert PackedGaussTrackStats.size(K, D) == K * K + 3 * K * D + 1
    buf = np.arange(PackedGaussTrackStats.size(K, D), dtype=float)
    o = np.arange(D) + 0.5
    st = PackedGaussTrackStats(buf, K, D, o)
    assert not hasattr(st, "counts") and not hasattr(st, "col_counts") and not hasattr(st, "xsq")
    assert st.A_raw.shape == (K, K) and st.flat.shape == (K, 3 * D) and st.sxx.shape == st.sx.shape == st.n.shape == (K, D)
    assert st.sxx[1, 2] == K * K + 3 * D + 2 and st.sx[1, 2] == K * K + 3 * D + D + 2
    assert st.n[1, 2] == K * K + 3 * D + 2 * D + 2 and st.lb[0] == buf[-1]
    st.n[2, 3] = -7.0                        # views, not copies
    assert buf[K * K + 2 * 3 * D + 2 * D + 3] == -7.0
    st2 = rewrap_packed(st, buf * 2)
    assert type(st2) is PackedGaussTrackStats and st2.D == D and st2.sx[1, 2] == 2 * st.sx[1, 2] and st2.origin is o
    assert type(rewrap_packed(PackedPoissonStats(np.zeros(PackedPoissonStats.size(K, D)), K, D),
                              np.zeros(PackedPoissonStats.size(K, D)))) is PackedPoissonStats


def test_problems_hold_every_kind_of_entry():
    for i, (K, D) in enumerate(H.SHAPES):
        p = H.problem(i)
        x, mask = p["x"], p["mask"]
        ok = H.present(x)
        assert 0.05 < np.isnan(x).mean() and np.isposinf(x).any() and np.isneginf(x).any()
        assert (x == 1e308).any() and (x == -1e200).any() and mask.any() and 0.03 < mask.mean() < 0.2
        assert (~ok.any(1) & ~mask).sum() >= 2
        if D > 1:
            assert not ok[:, D // 2].any() and p["origin"][D // 2] == 0.0
        assert np.all(p["hprec"] < 0) and np.all(np.abs(p["mu"]) < 2e3)
        ll = H.lliks_of(p)
        assert np.all(np.isfinite(ll)) and not np.any(np.signbit(ll[~ok.any(1)]))


def test_grow_case_of_the_gpu_test_keeps_its_margin():
    from tests.grow_helpers import grow_direct
    p, Tg = H.grow_case()
    compared, ll = H.grow_compared(p, Tg)
    eps = H.GROW_RULE["eps"]
    assert len(compared) and np.all((compared < eps / 3) | (compared > eps * 3))
    halves = [grow_direct(ll, p["mod_init"], p["ltran"], Tg, int(c), **H.GROW_RULE)[0] for c in H.GROW_CENTERS]
    assert len(set(halves)) > 1
