"""Multi-column Categorical emissions, host side: the ``ProductCategorical`` plugin against ``Categorical``
(D = 1) and against brute-force sums (D = 3), the batch class on the oracle engine, the packed view and the
C-ABI prototype.  No GPU."""
import numpy as np
from scipy.special import digamma

from pysvihmm_amd import _lib, hmmbatchcd
from pysvihmm_amd.distributions import Categorical, ProductCategorical
from pysvihmm_amd.engine import PackedMCatStats
from oracle.engine import OracleEngine

from tests.mcat_helpers import mcat_counts, mcat_lliks, offsets_of


def test_signature_and_limits():
    assert "svihmm_set_emission_mcat" in _lib.SIGNATURES
    assert _lib.MCAT_MAX_D == 128 and _lib.MCAT_MAX_F == 1024


def test_product_categorical_d1_equals_categorical():
    rng = np.random.default_rng(0)
    V = 6
    a0, am = rng.random(V) + 0.5, rng.random(V) * 3 + 0.2
    c = Categorical(alphav_0=a0, alpha_mf=am, weights=am / am.sum())
    p = ProductCategorical(alphav_0=[a0], alpha_mf=[am], weights=[am / am.sum()])
    x = rng.integers(0, V, size=(40, 1)).astype(float)
    x[[3, 17]] = np.nan
    assert np.array_equal(c.expected_log_likelihood(x), p.expected_log_likelihood(x), equal_nan=True)
    assert c.get_vlb() == p.get_vlb()
    assert c.num_parameters() == p.num_parameters()
    w = rng.random(40)
    ok = ~np.isnan(x[:, 0])
    c.meanfieldupdate(x[ok], w[ok])
    p.meanfieldupdate(x[ok], w[ok])
    assert np.array_equal(c.alpha_mf, p.alpha_mf[0])
    assert np.array_equal(c.weights, p.weights[0])
    assert c.get_vlb() == p.get_vlb()
    assert np.array_equal(c.expected_log_likelihood(x), p.expected_log_likelihood(x), equal_nan=True)


def test_product_categorical_d3_against_brute_force():
    rng = np.random.default_rng(1)
    V = (2, 5, 1)
    a0 = [rng.random(v) + 0.5 for v in V]
    am = [rng.random(v) * 3 + 0.2 for v in V]
    p = ProductCategorical(alphav_0=a0, alpha_mf=am)
    n = 60
    x = np.stack([rng.integers(0, v, size=n) for v in V], axis=1).astype(float)
    x[rng.random((n, 3)) < 0.2] = np.nan
    x[5] = np.nan                      # no column present
    x[6] = [2.0, -1.0, 1.0]            # every column out of range
    x[7, 1] = 5.0                      # one past the last symbol: skipped, the others count
    ell = p.expected_log_likelihood(x)
    w = rng.random(n)
    counts = [np.zeros(v) for v in V]
    for t in range(n):
        s, any_present = 0.0, False
        for d in range(3):
            v = x[t, d]
            if v != v or not 0 <= int(v) < V[d]:
                continue
            any_present = True
            s += digamma(am[d][int(v)]) - digamma(am[d].sum())
            counts[d][int(v)] += w[t]
        if any_present:
            assert abs(ell[t] - s) <= 1e-14 * max(1.0, abs(s))
        else:
            assert np.isnan(ell[t])
    assert np.isnan(ell[5]) and np.isnan(ell[6]) and np.isfinite(ell[7])
    # the helpers state the same loop
    logp = np.concatenate([digamma(a) - digamma(a.sum()) for a in am])[None, :]
    np.testing.assert_array_equal(np.nan_to_num(ell), mcat_lliks(x, None, V, logp)[:, 0])
    np.testing.assert_allclose(mcat_counts(x, None, V, w[:, None])[0], np.concatenate(counts), rtol=1e-13)
    vlb = sum(Categorical(alphav_0=a0[d], alpha_mf=am[d], weights=am[d] / am[d].sum()).get_vlb() for d in range(3))
    assert abs(p.get_vlb() - vlb) <= 1e-13 * abs(vlb)
    p.meanfieldupdate(x, w)
    for d in range(3):
        np.testing.assert_allclose(p.alpha_mf[d], a0[d] + counts[d], rtol=1e-13)
        np.testing.assert_allclose(p.weights[d].sum(), 1.0, rtol=1e-14)
    assert p.rvs(4).shape == (4, 3) and p.num_parameters() == 8


def _cat_problem(K, V, T, seed, miss=0.1):
    rng = np.random.default_rng(seed)
    theta = rng.dirichlet(np.ones(V) * 0.3, size=K)
    sts = np.repeat(rng.integers(0, K, size=T // 10 + 1), 10)[:T]
    obs = np.array([rng.choice(V, p=theta[s]) for s in sts], dtype=float)
    return obs, rng.random(T) < miss


def test_batchcd_product_categorical_d1_equals_categorical_on_the_oracle_engine():
    """The engine without the family keeps the host-lliks route: the literal loop through the plugin."""
    K, V, T = 3, 6, 400
    obs, mask = _cat_problem(K, V, T, 5)

    def run(make):
        np.random.seed(3)
        emit = np.array([make() for _ in range(K)])
        m = hmmbatchcd.VBHMM(obs.copy()[:, None], np.ones(K), np.ones((K, K)), emit, mask=mask, maxit=4,
                             engine=OracleEngine())
        m.infer(fused=False)
        return m
    a = run(lambda: Categorical(alphav_0=np.ones(V) * 0.5))
    b = run(lambda: ProductCategorical(alphav_0=[np.ones(V) * 0.5]))
    assert not b._mcat_fastpath() and not b._cat_fastpath() and a._cat_fastpath()
    np.testing.assert_allclose(b.var_tran, a.var_tran, rtol=1e-10)
    for k in range(K):
        np.testing.assert_allclose(b.var_emit[k].alpha_mf[0], a.var_emit[k].alpha_mf, rtol=1e-10)
    np.testing.assert_allclose(b.elbo_vec, a.elbo_vec, rtol=1e-10)


def test_packed_mcat_stats_slicing():
    K, V = 3, (2, 5, 1)
    F = sum(V)
    assert PackedMCatStats.size(K, V) == K * K + K * F + 1
    buf = np.arange(PackedMCatStats.size(K, V), dtype=float)
    st = PackedMCatStats(buf, K, V)
    assert not hasattr(st, "counts")         # (the batch classes tell the one-column family by that name)
    assert st.A_raw.shape == (K, K) and st.flat.shape == (K, F) and st.lb.shape == (1,)
    assert st.A_raw[0, 0] == 0 and st.flat[0, 0] == K * K and st.lb[0] == buf[-1]
    off = offsets_of(V)
    assert [c.shape for c in st.col_counts] == [(K, v) for v in V]
    for d in range(3):
        np.testing.assert_array_equal(st.col_counts[d], st.flat[:, off[d]:off[d + 1]])
    st.col_counts[1][2, 3] = -7.0            # views, not copies
    assert buf[K * K + 2 * F + off[1] + 3] == -7.0
