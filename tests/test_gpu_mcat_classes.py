"""The batch classes on ``ProductCategorical`` emitters (multi-column Categorical family on the device):
hmmbatchcd fused against the literal host path through the plugin, a list of sequences (infer / viterbi /
ffbs_windows), and hmmbatchsgd minibatches of whole sequences."""
import numpy as np
import pytest

from oracle import ref_c
from oracle import ref_numpy as R
from pysvihmm_amd import hmmbatchcd, hmmbatchsgd
from pysvihmm_amd.distributions import ProductCategorical
from pysvihmm_amd.hmmsgd_metaobs import MetaObs
from tests.mcat_helpers import mcat_counts, mcat_lliks

pytestmark = pytest.mark.gpu

K, V = 4, (2, 3, 4)
LENGTHS = (40, 1, 65, 30, 64, 57, 43)


def data(T, seed):
    rng = np.random.default_rng(seed)
    theta = [rng.dirichlet(np.ones(v) * 0.4, size=K) for v in V]
    sts = np.repeat(rng.integers(0, K, size=T // 12 + 1), 12)[:T]
    x = np.stack([[rng.choice(v, p=th[s]) for s in sts] for v, th in zip(V, theta)], axis=1).astype(float)
    x[rng.random(x.shape) < 0.05] = np.nan            # single missing entries
    x[rng.permutation(T)[:3]] = np.nan                # whole missing rows
    mask = rng.random(T) < 0.1
    return x, mask


def emitters():
    return np.array([ProductCategorical(alphav_0=[np.ones(v) * 0.5 for v in V]) for _ in range(K)])


def close(a, b, rtol):
    """tests/test_categorical.py _close_cat, per column."""
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=max(rtol, 1e-8))
    for k in range(K):
        for d in range(len(V)):
            np.testing.assert_allclose(a.var_emit[k].alpha_mf[d], b.var_emit[k].alpha_mf[d], rtol=rtol, atol=1e-9)
            np.testing.assert_allclose(a.var_emit[k].weights[d], b.var_emit[k].weights[d], rtol=rtol, atol=1e-10)
    np.testing.assert_allclose(a.var_x, b.var_x, rtol=rtol * 10, atol=1e-11)


def test_batchcd_fused_equals_the_literal_host_path():
    x, mask = data(300, 1)

    def make():
        np.random.seed(3)
        return hmmbatchcd.VBHMM(x.copy(), np.ones(K), np.ones((K, K)), emitters(), mask=mask, maxit=5)
    a = make()
    assert a.engine.name == "hip" and a._mcat_fastpath()
    a.infer(fused=True)
    b = make()
    b._engine = a.engine                               # the same GPU engine
    b._mcat_fastpath = lambda: False                   # ... through the plugin: host lliks, literal global_update
    b.infer(fused=False)
    assert len(a.elbo_vec) == 5
    close(a, b, 1e-6)
    c = make()                                         # fused=False with the family: device statistics of var_x
    c._engine = a.engine
    c.infer(fused=False)
    close(a, c, 1e-6)


def split(x, mask):
    off = np.concatenate(([0], np.cumsum(LENGTHS)))
    return [x[a:b].copy() for a, b in zip(off[:-1], off[1:])], [mask[a:b].copy() for a, b in zip(off[:-1], off[1:])], off


def test_batchcd_on_a_list_of_sequences():
    x, mask = data(sum(LENGTHS), 2)
    xs, ms, off = split(x, mask)
    np.random.seed(4)
    m = hmmbatchcd.VBHMM(xs, np.ones(K), np.ones((K, K)), emitters(), mask=ms, maxit=3)
    assert m._mcat_fastpath()
    m.infer()
    assert len(m.elbo_vec) == 3 and np.all(np.isfinite(m.elbo_vec)) and m.var_x.shape == (sum(LENGTHS), K)
    zs, score = m.viterbi()
    assert len(zs) == len(LENGTHS)
    for s in range(len(LENGTHS)):
        z1, s1 = m.viterbi(metaobs=MetaObs(int(off[s]), int(off[s + 1]) - 1))
        np.testing.assert_array_equal(zs[s], z1)
        assert score[s] == s1
    paths = m.ffbs_windows(n_draws=2, seed=11)
    assert [p.shape for p in paths] == [(2, n) for n in LENGTHS]
    assert all(p.min() >= 0 and p.max() < K for p in paths)


def test_batchsgd_sequence_minibatch_statistics():
    x, mask = data(sum(LENGTHS), 5)
    xs, ms, off = split(x, mask)
    np.random.seed(6)
    m = hmmbatchsgd.VBHMM(xs, np.ones(K), np.ones((K, K)), emitters(), mask=ms, maxit=3, seq_minibatch=3)
    seen = []
    inner = m._sequence_subset_estep

    def spy(idx):
        tabs = [e.expected_log_tables() for e in m.var_emit]
        out = inner(idx)
        seen.append((np.array(idx), tabs, m.mod_init.copy(), m.mod_tran.copy(), m.obs.copy()))
        return out
    m._sequence_subset_estep = spy
    stats = []
    scaled = m._seq_minibatch_stats
    m._seq_minibatch_stats = lambda: stats.append(scaled()) or stats[-1]
    m.infer()
    assert len(m.elbo_vec) == 3 and len(seen) == 3 and np.all(np.isfinite(m.elbo_vec))
    idx, tabs, mod_init, mod_tran, obs = seen[0]
    bf = len(LENGTHS) / 3.0
    assert m.batchfactor == bf and len(idx) == 3
    logp = np.stack([np.concatenate(t) for t in tabs])
    A, C, lb, rows = 0.0, 0.0, 0.0, 0
    for s in idx:
        a, b = int(off[s]), int(off[s + 1])
        ll = mcat_lliks(obs[a:b], None, V, logp, 0)
        la, lbeta = ref_c.forward(ll, mod_init, mod_tran), ref_c.backward(ll, mod_tran)
        q = R.posterior(la, lbeta)
        A = A + (q[:-1].T.dot(q[1:]) if b - a > 1 else 0.0)
        C = C + mcat_counts(obs[a:b], mask[a:b], V, q)
        lb += R.local_lower_bound(la)
        rows += b - a
    st = stats[0]
    np.testing.assert_allclose(st.A_raw, bf * A, rtol=1e-6, atol=1e-9 * rows * bf)
    np.testing.assert_allclose(st.flat, bf * C, rtol=1e-6, atol=1e-9 * rows * bf)
    np.testing.assert_allclose(st.lb[0], bf * lb, rtol=1e-10)
    assert min(a.min() for e in m.var_emit for a in e.alpha_mf) > 0
