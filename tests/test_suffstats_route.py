"""Route selection of the host loops' statistics (no GPU): an engine with ``suffstats`` built from
oracle/ref_numpy stands in for the device.  The metaobs host loop calls it once per minibatch when
only the message methods are overridden, and never when ``intermediate_pars`` is replaced, a
communicator is set, the engine lacks the method or the emission family has no device statistics;
the batch classes call it once per iteration when ``local_update`` is overridden.  Results equal
the host path."""
import glob
import os

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle.engine import OracleEngine, TRANS_WRAP
from pysvihmm_amd import hmmbatchcd, hmmbatchsgd, hmmsgd_metaobs
from pysvihmm_amd.distributions import Categorical, DiagonalGaussian, Gaussian
from pysvihmm_amd.engine import PackedCatStats, PackedDiagStats, PackedStats

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
META = sorted(glob.glob(os.path.join(GOLDEN, "metaobs_K4_D2_L10_mask.npz")))


class StatsEngine(OracleEngine):
    """OracleEngine + ``suffstats`` in the HIP engine's calling convention, counted."""

    def __init__(self):
        super(StatsEngine, self).__init__()
        self.suffstats_calls = []

    def suffstats(self, starts, Lm, var_x, flags=TRANS_WRAP, read=True):
        self._pre_mutate()
        st = np.asarray(starts, dtype=np.int64).ravel()
        q = np.asarray(var_x, dtype=np.float64)
        if q.shape != (len(st), Lm, self.K):
            raise ValueError("suffstats: var_x shape")
        self.suffstats_calls.append((len(st), Lm, flags))
        K, D = self.K, self.D
        mask = np.zeros(self.T, bool) if self.mask is None else self.mask
        A = np.zeros((K, K))
        for b in range(len(st)):
            A += R.transition_stat_wrap(q[b]) if flags & TRANS_WRAP else R.transition_stat_batch(q[b])
        rows = st[:, None] + np.arange(Lm)
        keep = ~mask[rows]
        X, W = self.obs[rows][keep], q[keep]
        if getattr(self, "V", 0):
            V = self.V
            P = PackedCatStats(np.zeros(PackedCatStats.size(K, V)), K, V)
            ok = ~np.isnan(X[:, 0])
            for v in range(V):
                P.counts[:, v] = W[ok][X[ok, 0].astype(int) == v].sum(0)
        elif getattr(self, "diag", False):
            P = PackedDiagStats(np.zeros(PackedDiagStats.size(K, D)), K, D)
            for k in range(K):
                P.xbar[k], P.neff[k], P.xsq[k] = R.diag_suffstats(X, W[:, k])
        else:
            P = PackedStats(np.zeros(PackedStats.size(K, D)), K, D)
            for k in range(K):
                P.xbar[k], P.neff[k], P.S[k] = R.niw_suffstats(X, W[:, k])
        P.A_raw[:] = A
        return P


def _emit_from_fixture(g, K):
    out = []
    for k in range(K):
        e = Gaussian(mu=g["init_mu"][k], sigma=np.eye(len(g["init_mu"][k])),
                     mu_0=g["prior_mu0"][k], sigma_0=g["prior_sigma0"][k],
                     kappa_0=float(g["prior_kappa0"][k]), nu_0=float(g["prior_nu0"][k]))
        e.mu_mf = g["init_mu"][k].copy(); e.sigma_mf = g["init_sigma"][k].copy()
        e.kappa_mf = float(g["init_kappa"][k]); e.nu_mf = float(g["init_nu"][k])
        out.append(e)
    return np.array(out)


class MsgOverride(hmmsgd_metaobs.VBHMM):
    def backward_msgs(self, metaobs=None):
        super(MsgOverride, self).backward_msgs(metaobs)


class InterOverride(MsgOverride):
    def intermediate_pars(self, metaobs=None):
        return super(InterOverride, self).intermediate_pars(metaobs)


def _meta(cls, family, engine, grow=False, maxit=3):
    if family == "niw":
        g = np.load(META[0])
        K = int(g["K"])
        return cls(g["obs"].copy(), np.ones(K), g["prior_tran"], _emit_from_fixture(g, K), tau=1.0, kappa=0.7,
                   metaobs_half=int(g["L"]), mb_sz=int(g["S"]), mask=g["mask"], init_tran=g["init_tran"],
                   maxit=maxit, seed=5, growBuffer=grow, engine=engine)
    rng = np.random.default_rng(11)
    K, T = 3, 400
    sts = np.repeat(rng.integers(0, K, size=T // 20), 20)
    mask = rng.random(T) < 0.1
    np.random.seed(2)
    if family == "diag":
        D = 2
        means = rng.normal(0, 4, size=(K, D))
        obs = means[sts] + rng.normal(size=(T, D))
        emit = np.array([DiagonalGaussian(mu=means[k] + rng.normal(size=D), mu_0=obs.mean(0), nus_0=0.01,
                                          alphas_0=2.0, betas_0=obs.var(0)) for k in range(K)])
    else:
        V = 5
        theta = rng.dirichlet(np.ones(V) * 0.3, size=K)
        obs = np.array([rng.choice(V, p=theta[s]) for s in sts], dtype=float)
        emit = np.array([Categorical(alphav_0=np.ones(V) * 0.5) for _ in range(K)])
    return cls(obs, np.ones(K), np.ones((K, K)), emit, tau=1.0, kappa=0.7, metaobs_half=4, mb_sz=4,
               mask=mask, maxit=maxit, seed=4, growBuffer=grow, engine=engine)


def _factors(m):
    out = []
    for G in m.var_emit:
        if isinstance(G, Categorical):
            out.append(np.asarray(G.alpha_mf))
        elif isinstance(G, DiagonalGaussian):
            out += [np.asarray(G.mf_mu), np.asarray(G.mf_nus), np.asarray(G.mf_alphas), np.asarray(G.mf_betas)]
        else:
            out += [np.asarray(G.mu_mf), np.asarray(G.sigma_mf), np.asarray([G.kappa_mf, G.nu_mf])]
    return out


def _agree(a, b, rtol):
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=rtol)
    # (the ELBO is a sum of gammaln terms that cancel to a few parts in 1e3: the statistics' last
    #  bits, summed in another order, show there ~100x magnified)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=max(rtol, 1e-10))
    for x, y in zip(_factors(a), _factors(b)):
        np.testing.assert_allclose(x, y, rtol=rtol, atol=1e-13)


@pytest.mark.parametrize("family,grow", [("niw", False), ("diag", False), ("cat", False), ("niw", True)])
def test_metaobs_message_override_takes_the_route(monkeypatch, family, grow):
    host = _meta(MsgOverride, family, OracleEngine(), grow)
    host.infer()
    eng = StatsEngine()
    m = _meta(MsgOverride, family, eng, grow)
    assert m._suffstats_route()

    def boom(*a, **k):
        raise AssertionError("host statistics ran")
    monkeypatch.setattr(hmmsgd_metaobs.VBHMM, "_intermediate", boom)
    m.infer()
    assert len(eng.suffstats_calls) == m.maxit                  # one call per minibatch
    assert all(f == TRANS_WRAP for _, _, f in eng.suffstats_calls)
    if grow:
        assert all(Lm == 2 * m.metaobs_half + 1 for _, Lm, _ in eng.suffstats_calls)
    _agree(m, host, 1e-12)


def test_metaobs_no_route_when_intermediate_pars_is_replaced():
    eng = StatsEngine()
    m = _meta(InterOverride, "niw", eng)
    assert not m._suffstats_route()
    m.infer()
    assert eng.suffstats_calls == []
    eng2 = StatsEngine()
    m2 = _meta(MsgOverride, "niw", eng2)
    m2.intermediate_pars = lambda metaobs=None: hmmsgd_metaobs.VBHMM.intermediate_pars(m2, metaobs)
    assert not m2._suffstats_route()
    m2.infer()
    assert eng2.suffstats_calls == []
    host = _meta(MsgOverride, "niw", OracleEngine())
    host.infer()
    _agree(m, host, 1e-12)
    _agree(m2, host, 1e-12)


def test_metaobs_no_route_without_method_comm_or_fast_path():
    m = _meta(MsgOverride, "niw", OracleEngine())
    assert not m._suffstats_route()                               # engine lacks suffstats
    m = _meta(MsgOverride, "niw", StatsEngine())
    m.comm = object()
    assert not m._suffstats_route()                               # a communicator shards the minibatch
    m = _meta(MsgOverride, "niw", StatsEngine())
    m.obs = np.zeros((m.T, 97))                                   # wider than the NIW kernels: no fast path
    assert not m._suffstats_route()


class _Local(object):
    def local_update(self, obs=None, mask=None):
        super(_Local, self).local_update(obs, mask)


@pytest.mark.parametrize("name,mod", [("batchcd_K4_D2_T300", hmmbatchcd), ("batchsgd_K4_D3_T250", hmmbatchsgd)])
def test_batch_local_update_override_takes_the_route(monkeypatch, name, mod):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K = int(g["K"])
    Sub = type("Sub", (_Local, mod.VBHMM), {})

    def make(engine):
        kw = dict(mask=g["mask"], init_tran=g["init_tran"], maxit=int(g["maxit"]), engine=engine)
        if mod is hmmbatchsgd:
            kw.update(tau=1.0, kappa=0.7)
        return Sub(g["obs"].copy(), g["prior_init"], g["prior_tran"], _emit_from_fixture(g, K), **kw)

    host = make(OracleEngine())
    host.infer()
    eng = StatsEngine()
    m = make(eng)

    def boom(*a, **k):
        raise AssertionError("literal global_update ran")
    monkeypatch.setattr(mod.VBHMM, "global_update", boom)
    m.infer()
    n_it = len(eng.suffstats_calls)
    assert n_it >= len(m.elbo_vec) and all(c == (1, m.T, 0) for c in eng.suffstats_calls)
    _agree(m, host, 1e-9)
    np.testing.assert_allclose(m.var_init, host.var_init, rtol=1e-12)


def test_batch_global_update_override_keeps_the_host_path():
    g = np.load(os.path.join(GOLDEN, "batchcd_K4_D2_T300.npz"))
    K = int(g["K"])

    class Sub(hmmbatchcd.VBHMM):
        def global_update(self):
            super(Sub, self).global_update()

    eng = StatsEngine()
    m = Sub(g["obs"].copy(), g["prior_init"], g["prior_tran"], _emit_from_fixture(g, K), mask=g["mask"],
            init_tran=g["init_tran"], maxit=3, engine=eng)
    m.infer()
    assert eng.suffstats_calls == []
