"""The batch classes on ``ProductPoisson`` emitters (Poisson count family on the device): hmmbatchcd fused against
the literal host path through the plugin, a list of sequences, and hmmbatchsgd minibatches of whole sequences."""
import numpy as np
import pytest

from oracle import ref_c
from oracle import ref_numpy as R
from pysvihmm_amd import hmmbatchcd, hmmbatchsgd
from pysvihmm_amd.distributions import ProductPoisson
from tests.poisson_helpers import logfact_table, poisson_lliks, poisson_stats

pytestmark = pytest.mark.gpu

K, D, CMAX = 4, 3, 255
LENGTHS = (40, 1, 65, 30, 64, 57, 43)
LAM = np.array([[1.0, 9.0, 30.0], [6.0, 1.5, 12.0], [15.0, 20.0, 2.0], [3.0, 40.0, 60.0]])


def data(T, seed):
    rng = np.random.default_rng(seed)
    sts = np.repeat(rng.integers(0, K, size=T // 12 + 1), 12)[:T]
    x = rng.poisson(LAM[sts]).astype(float)
    x[rng.random(x.shape) < 0.05] = np.nan            # single missing entries
    x[rng.permutation(T)[:3]] = np.nan                # whole missing rows
    x[5, 1] = CMAX + 1.0                              # out of the table's range: skipped
    mask = rng.random(T) < 0.1
    return x, mask


def emitters():
    rng = np.random.default_rng(9)
    return np.array([ProductPoisson(np.ones(D), np.full(D, 0.2), alpha_mf=rng.uniform(1.0, 40.0, size=D) * 2.0,
                                    beta_mf=np.full(D, 2.0), max_count=CMAX) for _ in range(K)])


def close(a, b, rtol):
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=rtol, atol=1e-9)
    for k in range(K):
        np.testing.assert_allclose(a.var_emit[k].alpha_mf, b.var_emit[k].alpha_mf, rtol=rtol, atol=1e-9)
        np.testing.assert_allclose(a.var_emit[k].beta_mf, b.var_emit[k].beta_mf, rtol=rtol, atol=1e-9)


def split(x, mask):
    off = np.concatenate(([0], np.cumsum(LENGTHS)))
    return [x[a:b].copy() for a, b in zip(off[:-1], off[1:])], [mask[a:b].copy() for a, b in zip(off[:-1], off[1:])], off


def test_batchcd_fused_equals_the_literal_host_path():
    x, mask = data(300, 1)

    def make():
        np.random.seed(3)
        return hmmbatchcd.VBHMM(x.copy(), np.ones(K), np.ones((K, K)), emitters(), mask=mask, maxit=2)
    a = make()
    assert a.engine.name == "hip" and a._poisson_fastpath() and a._device_family()
    a.infer(fused=True)
    b = make()
    b._engine = a.engine                               # the same GPU engine
    b._poisson_fastpath = lambda: False                # ... through the plugin: host lliks, literal global_update
    b.infer(fused=False)
    assert len(a.elbo_vec) == 2
    close(a, b, 1e-6)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=1e-8)
    c = make()                                         # fused=False with the family: device statistics of var_x
    c._engine = a.engine
    c.infer(fused=False)
    close(a, c, 1e-6)


def test_batchcd_on_a_list_of_sequences():
    x, mask = data(sum(LENGTHS), 2)
    xs, ms, off = split(x, mask)

    def make(obs, msk):
        np.random.seed(4)
        return hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), emitters(), mask=msk, maxit=2)
    m = make(xs, ms)
    assert m._poisson_fastpath()
    m.infer()
    assert len(m.elbo_vec) == 2 and np.all(np.isfinite(m.elbo_vec)) and m.var_x.shape == (sum(LENGTHS), K)
    # the literal host path: per sequence the plugin's lliks and the referee's recursions, the plugin's update
    emit = emitters()
    np.random.seed(4)
    ref = hmmbatchcd.VBHMM(xs, np.ones(K), np.ones((K, K)), emit, mask=ms, maxit=2)
    for _ in range(2):
        ref._psi_expectations()
        mod_init, mod_tran = ref.mod_init, ref.mod_tran
        ll = np.nan_to_num(np.stack([e.expected_log_likelihood(x) for e in emit], axis=1))
        q = np.zeros((len(x), K))
        A, q0 = np.zeros((K, K)), np.zeros(K)
        for a, b in zip(off[:-1], off[1:]):
            la, lbeta = ref_c.forward(ll[a:b], mod_init, mod_tran), ref_c.backward(ll[a:b], mod_tran)
            q[a:b] = R.posterior(la, lbeta)
            if b - a > 1:
                A += q[a:b - 1].T.dot(q[a + 1:b])
            q0 += q[a]
        ref.var_tran = ref.prior_tran + A
        ref.var_init = ref.prior_init + q0
        for k in range(K):
            emit[k].meanfieldupdate(x[~mask], q[~mask, k])
    np.testing.assert_allclose(m.var_tran, ref.var_tran, rtol=1e-6, atol=1e-9)
    for k in range(K):
        np.testing.assert_allclose(m.var_emit[k].alpha_mf, emit[k].alpha_mf, rtol=1e-6, atol=1e-9)
        np.testing.assert_allclose(m.var_emit[k].beta_mf, emit[k].beta_mf, rtol=1e-6, atol=1e-9)
    zs, score = m.viterbi()
    assert len(zs) == len(LENGTHS) and all(len(z) == n for z, n in zip(zs, LENGTHS))


def test_batchsgd_sequence_minibatch_statistics():
    x, mask = data(sum(LENGTHS), 5)
    xs, ms, off = split(x, mask)
    np.random.seed(6)
    m = hmmbatchsgd.VBHMM(xs, np.ones(K), np.ones((K, K)), emitters(), mask=ms, maxit=3, seq_minibatch=3)
    seen = []
    inner = m._sequence_subset_estep

    def spy(idx):
        tabs = [e.expected_tables() for e in m.var_emit]
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
    elog, erate = np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs])
    A, S, lb, rows = 0.0, 0.0, 0.0, 0
    for s in idx:
        a, b = int(off[s]), int(off[s + 1])
        ll = poisson_lliks(obs[a:b], None, elog, erate, logfact_table(CMAX), 0)
        la, lbeta = ref_c.forward(ll, mod_init, mod_tran), ref_c.backward(ll, mod_tran)
        q = R.posterior(la, lbeta)
        A = A + (q[:-1].T.dot(q[1:]) if b - a > 1 else 0.0)
        S = S + poisson_stats(obs[a:b], mask[a:b], CMAX, q)
        lb += R.local_lower_bound(la)
        rows += b - a
    st = stats[0]
    np.testing.assert_allclose(st.A_raw, bf * A, rtol=1e-6, atol=1e-9 * rows * bf)
    np.testing.assert_allclose(st.n, bf * S[:, D:], rtol=1e-6, atol=1e-9 * rows * bf)
    np.testing.assert_allclose(st.sx, bf * S[:, :D], rtol=1e-6, atol=1e-9 * rows * bf * np.nanmax(obs[obs <= CMAX]))
    np.testing.assert_allclose(st.lb[0], bf * lb, rtol=1e-10)
    assert min(e.alpha_mf.min() for e in m.var_emit) > 0 and min(e.beta_mf.min() for e in m.var_emit) > 0
