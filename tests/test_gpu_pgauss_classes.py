"""The batch classes on ``ProductGaussian`` emitters (Gaussian tracks with missing entries on the device): hmmbatchcd
and hmmbatchsgd on the HipEngine against the same classes on host lliks through the plugin, a list of sequences,
sequence minibatches on the host route of the step, and the entry-wise held-out score after ``speckle_holdout``."""
import numpy as np
import pytest

from pysvihmm_amd import hmmbatchcd, hmmbatchsgd, util
from pysvihmm_amd.distributions import ProductGaussian
from pysvihmm_amd.engine import PackedGaussTrackStats
from tests import pgauss_helpers as H

pytestmark = pytest.mark.gpu

K, D, T = 4, 3, 300
LENGTHS = (40, 1, 65, 30, 64, 57, 43)
MEANS = 1e3 + np.array([[0.0, 5.0, -3.0], [4.0, -2.0, 6.0], [-5.0, 1.0, 2.0], [8.0, 9.0, -8.0]])


def data(T_, seed):
    rng = np.random.default_rng(seed)
    sts = np.repeat(rng.integers(0, K, size=T_ // 12 + 1), 12)[:T_]
    x = MEANS[sts] + rng.normal(size=(T_, D)) * np.array([1.0, 2.0, 0.5])
    x[rng.random(x.shape) < 0.15] = np.nan            # single missing entries
    x[rng.permutation(T_)[:3]] = np.nan               # whole missing rows
    x[5, 1], x[6, 2] = np.inf, -1e200                 # sentinels: skipped
    mask = rng.random(T_) < 0.1
    return x, mask


def emitters():
    rng = np.random.default_rng(9)
    np.random.seed(11)
    return np.array([ProductGaussian(mu=MEANS[k] + rng.normal(size=D), sigmas=np.full(D, 4.0), mu_0=np.full(D, 1e3),
                                     nus_0=0.05, alphas_0=2.0, betas_0=2.0) for k in range(K)])


def factors(m):
    return [np.stack([getattr(e, n) for e in m.var_emit]) for n in ("mf_mu", "mf_nus", "mf_alphas", "mf_betas")]


def close(a, b, rtol):
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=rtol, atol=1e-9)
    for fa, fb in zip(factors(a), factors(b)):
        np.testing.assert_allclose(fa, fb, rtol=rtol)


def split(x, mask):
    off = np.concatenate(([0], np.cumsum(LENGTHS)))
    return [x[a:b].copy() for a, b in zip(off[:-1], off[1:])], [mask[a:b].copy() for a, b in zip(off[:-1], off[1:])], off


@pytest.mark.parametrize("cls", [hmmbatchcd, hmmbatchsgd], ids=["batchcd", "batchsgd"])
def test_fused_equals_the_same_class_on_host_lliks(cls):
    x, mask = data(T, 1)

    def make():
        np.random.seed(3)
        return cls.VBHMM(x.copy(), np.ones(K), np.ones((K, K)), emitters(), mask=mask, maxit=3)
    a = make()
    assert a.engine.name == "hip" and a._pgauss_fastpath() and a._device_family() and not a._diag_fastpath()
    a.infer(fused=True)
    b = make()
    b._engine = a.engine                               # the same GPU engine
    b._pgauss_fastpath = lambda: False                 # ... through the plugin: host lliks, literal global_update
    assert not b._device_family()
    b.infer(fused=False)
    assert len(a.elbo_vec) == 3 and np.all(np.isfinite(a.elbo_vec))
    close(a, b, 1e-6)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=1e-8)
    c = make()                                         # fused=False with the family
    c._engine = a.engine
    c.infer(fused=False)
    close(a, c, 1e-6)
    st = a._batch_estep_stats()
    assert type(st) is PackedGaussTrackStats
    np.testing.assert_array_equal(st.origin, H.data_origin(a.obs))


def test_list_obs_is_accepted_and_minibatches_step_on_the_host_route():
    x, mask = data(sum(LENGTHS), 2)
    xs, ms, off = split(x, mask)
    np.random.seed(4)
    m = hmmbatchcd.VBHMM(xs, np.ones(K), np.ones((K, K)), emitters(), mask=ms, maxit=2)
    assert m._pgauss_fastpath()
    m.infer()
    assert len(m.elbo_vec) == 2 and np.all(np.isfinite(m.elbo_vec)) and m.var_x.shape == (sum(LENGTHS), K)
    assert all(np.all(np.isfinite(f)) for f in factors(m))
    zs, score = m.viterbi()
    assert len(zs) == len(LENGTHS) and all(len(z) == n for z, n in zip(zs, LENGTHS))
    np.random.seed(6)
    s = hmmbatchsgd.VBHMM(xs, np.ones(K), np.ones((K, K)), emitters(), mask=ms, maxit=3, seq_minibatch=3)
    with pytest.raises(RuntimeError, match="device_loop=True.*ProductGaussian"):
        s.infer(device_loop=True)
    s.infer()
    assert len(s.elbo_vec) == 3 and np.all(np.isfinite(s.elbo_vec)) and s.batchfactor == len(LENGTHS) / 3.0
    assert all(np.all(np.isfinite(f)) for f in factors(s)) and np.all(factors(s)[3] > 0)


def test_heldout_entries_logprob_after_speckle_holdout():
    x, _ = data(T, 5)
    xb, r, c, v = util.speckle_holdout(x, 0.1, seed=4)
    np.random.seed(4)
    m = hmmbatchcd.VBHMM(xb, np.ones(K), np.ones((K, K)), emitters(), maxit=3)
    m.infer()
    m.local_update()                                   # the class's own var_x under the factors infer() left
    q = np.array(m.var_x)
    before = [f.copy() for f in factors(m)]
    tabs = [e.expected_tables() for e in m.var_emit]
    p = dict(K=K, D=D, mu=np.stack([t[0] for t in tabs]), hprec=np.stack([t[1] for t in tabs]),
             cst=np.stack([t[2] for t in tabs]))
    want, _ = H.heldout_entries_numpy(p, q, r, c, v)
    val, lp = m.heldout_entries_logprob(r, c, v, per_entry=True)
    present = H.present(v)
    assert len(lp) == len(r) > 50 and np.array_equal(np.isnan(lp), ~present) and present.mean() > 0.9
    np.testing.assert_allclose(lp[present], want[present], rtol=1e-9)
    np.testing.assert_allclose(val, np.mean(want[present]), rtol=1e-9)
    assert m.heldout_entries_logprob(r, c, v) == val
    assert all(np.array_equal(a, b) for a, b in zip(before, factors(m))) and np.array_equal(q, m.var_x)
    with pytest.raises(ValueError, match="not blanked"):
        m.heldout_entries_logprob([0], [int(np.flatnonzero(~np.isnan(m.obs[0]))[0])], [1.0])
