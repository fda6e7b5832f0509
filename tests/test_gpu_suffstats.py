"""svihmm_suffstats / Engine.suffstats on the MI355X: expected sufficient statistics of posteriors
the caller supplies, against NumPy (oracle/ref_numpy), against the E-step on the same windows, its
error cases, and the class routes that use it (a message or local-update override keeps the
device statistics)."""
import os
import re

import numpy as np
import pytest
from scipy.special import digamma

from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from pysvihmm_amd import hmmbatchcd, hmmbatchsgd, hmmsgd_metaobs
from pysvihmm_amd.distributions import Categorical, DiagonalGaussian, Gaussian

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EPS = 1e-9


def _engine():
    from pysvihmm_amd.engine import HipEngine
    return HipEngine(0)


def _globals(eng, K, rng):
    vt = 1.0 + rng.random((K, K)) * 10
    vi = rng.random(K) + 0.1
    eng.set_globals(digamma(vi + EPS) - digamma(vi.sum() + EPS),
                    digamma(vt + EPS) - digamma(vt.sum(1)[:, None] + EPS))


def _posteriors(rng, B, Lm, K):
    """Non-negative, some rows normalised, some not, some all zero."""
    q = rng.random((B, Lm, K)) ** 3
    norm = rng.random((B, Lm)) < 0.5
    q[norm] /= q[norm].sum(-1, keepdims=True)
    q[rng.random((B, Lm)) < 0.1] = 0.0
    return q


def _windows(rng, T, B, Lm):
    return rng.integers(0, T - Lm + 1, size=B).astype(np.int64)


def _ref(obs, mask, starts, q, wrap, family, V=0):
    """(values, sums of |terms|) per packed block, window by window with oracle/ref_numpy."""
    B, Lm, K = q.shape
    D = obs.shape[1]
    A = np.zeros((K, K))
    out = {}
    for b in range(B):
        A += R.transition_stat_wrap(q[b]) if wrap else R.transition_stat_batch(q[b])
    out["A_raw"] = (A, A)                       # (q >= 0: the terms are their own magnitudes)
    s = starts[:, None] + np.arange(Lm)
    keep = ~mask[s]
    X = obs[s][keep]                            # [n, D] unmasked rows
    W = q[keep]                                 # [n, K]
    if family == "cat":
        ok = ~np.isnan(X[:, 0])
        sym = X[ok, 0].astype(int)
        counts = np.zeros((K, V))
        for v in range(V):
            counts[:, v] = W[ok][sym == v].sum(0)
        out["counts"] = (counts, counts)
        return out
    xbar, neff = np.zeros((K, D)), np.zeros(K)
    sec, axbar, asec = (np.zeros((K, D)) if family == "diag" else np.zeros((K, D, D)),
                        np.zeros((K, D)),
                        np.zeros((K, D)) if family == "diag" else np.zeros((K, D, D)))
    for k in range(K):
        if family == "diag":
            xbar[k], neff[k], sec[k] = R.diag_suffstats(X, W[:, k])
            axbar[k], _, asec[k] = R.diag_suffstats(np.abs(X), W[:, k])
        else:
            xbar[k], neff[k], sec[k] = R.niw_suffstats(X, W[:, k])
            axbar[k], _, asec[k] = R.niw_suffstats(np.abs(X), W[:, k])
    out["xbar"] = (xbar, axbar)
    out["neff"] = (neff, neff)
    out["xsq" if family == "diag" else "S"] = (sec, asec)
    return out


def _check(st, ref, tol=1e-12):
    for name, (val, mag) in ref.items():
        got = getattr(st, name)
        err = np.abs(got - val)
        bound = tol * mag + 1e-300
        assert np.all(err <= bound), "%s: worst excess %g (max err %g)" % (name, (err / (mag + 1e-300)).max(), err.max())
    assert st.lb[0] == 0.0


def _cases():
    # (B, Lm): below one 32-row stage, a row that is its own wrap predecessor, a minibatch
    return [(1, 1), (3, 1), (1, 2), (3, 2), (3, 31), (64, 31), (1, 257), (3, 257), (64, 257)]


def _run_family(eng, obs, mask, family, K, rng, V=0, shift=False):
    T = obs.shape[0]
    for i, (B, Lm) in enumerate(_cases()):
        if shift and i == len(_cases()) // 2:
            eng.shift_obs(np.full(obs.shape[1], 2.75))
        starts = _windows(rng, T, B, Lm)
        q = _posteriors(rng, B, Lm, K)
        for wrap in (True, False):
            st = eng.suffstats(starts, Lm, q, flags=L.TRANS_WRAP if wrap else 0)
            _check(st, _ref(obs, mask, starts, q, wrap, family, V))


@pytest.mark.parametrize("K", [3, 16, 64, 100, 256])
@pytest.mark.parametrize("D", [1, 2, 32])
@pytest.mark.parametrize("masked", [False, True])
def test_niw_against_numpy(K, D, masked):
    rng = np.random.default_rng(K * 100 + D + masked)
    T = 3000
    obs = rng.normal(size=(T, D)) * 2 + 40.0            # away from the origin: the centring matters
    mask = rng.random(T) < (0.15 if masked else 0.0)
    eng = _engine()
    try:
        eng.set_obs(obs, mask if masked else None)
        _globals(eng, K, rng)
        A = rng.normal(size=(K, D, D))
        eng.set_emission_niw(rng.normal(size=(K, D)) + 40.0, np.einsum('kij,klj->kil', A, A) + D * np.eye(D),
                             0.5 + rng.random(K), D + 2 + rng.random(K))
        _run_family(eng, obs, mask, "niw", K, rng, shift=masked)
    finally:
        eng.close()


@pytest.mark.parametrize("K", [5, 64, 100])
@pytest.mark.parametrize("D", [1, 8, 64])
def test_diag_against_numpy(K, D):
    rng = np.random.default_rng(7 * K + D)
    T = 2000
    obs = rng.normal(size=(T, D)) - 12.0
    mask = rng.random(T) < 0.1
    eng = _engine()
    try:
        eng.set_obs(obs, mask)
        _globals(eng, K, rng)
        eng.set_emission_diag(rng.normal(size=(K, D)) - 12.0, 1.0 + rng.random((K, D)),
                              2.0 + rng.random((K, D)), 1.0 + rng.random((K, D)))
        _run_family(eng, obs, mask, "diag", K, rng, shift=True)
    finally:
        eng.close()


@pytest.mark.parametrize("V", [2, 7, 32])
@pytest.mark.parametrize("K", [3, 64, 100])
def test_categorical_against_numpy(V, K):
    rng = np.random.default_rng(V * 1000 + K)
    T = 2000
    obs = rng.integers(0, V, size=(T, 1)).astype(float)
    mask = rng.random(T) < 0.1
    eng = _engine()
    try:
        eng.set_obs(obs, mask)
        _globals(eng, K, rng)
        eng.set_emission_cat(np.log(rng.dirichlet(np.ones(V), size=K)))
        _run_family(eng, obs, mask, "cat", K, rng, V=V)
    finally:
        eng.close()


@pytest.mark.parametrize("B,Lm,prec", [(8, 33, "f64"), (256, 65, "f64"), (256, 65, "f32")])
def test_matches_estep_and_leaves_it_alone(B, Lm, prec):
    from tests.helpers import make_problem
    p = make_problem(64, 8, 20000, seed=B + Lm, miss=0.1)
    rng = np.random.default_rng(3)
    eng = _engine()
    try:
        eng.set_obs(p["obs"], p["mask"])
        eng.set_globals(p["mod_init"], p["ltran"])
        eng.set_emission_niw(p["mu"], p["sigma"], p["kappa"], p["nu"])
        starts = _windows(rng, p["T"], B, Lm)
        # posteriors of these windows as the recursions give them
        q = eng.forward_backward(starts, Lm, want=("var_x",))["var_x"]
        est = eng.estep(starts, Lm, flags=L.TRANS_WRAP)
        q_e = eng.read_intermediate("var_x", B, Lm)
        np.testing.assert_allclose(q_e, q, rtol=1e-9, atol=1e-13)
        eng.set_precision(prec)
        st = eng.suffstats(starts, Lm, q_e)
        for name in ("A_raw", "xbar", "neff", "S"):
            a, b = getattr(st, name), getattr(est, name)
            assert np.abs(a - b).max() <= 1e-12 * np.abs(b).max(), name
        # the last E-step (in the precision mode under test) is undisturbed by a suffstats call
        eng.estep(starts, Lm, flags=L.TRANS_WRAP)
        z0, _ = eng.state_argmax()
        mode0 = eng.precision()
        qr = _posteriors(rng, 5, 17, 64)
        sr = _windows(rng, p["T"], 5, 17)
        st2 = eng.suffstats(sr, 17, qr)
        _check(st2, _ref(p["obs"], p["mask"], sr, qr, True, "niw"))
        assert eng.precision() == mode0
        q0 = eng.read_intermediate("var_x", B, Lm)
        ll0 = eng.read_rows("lliks", 0, Lm)
        z1, _ = eng.state_argmax()
        np.testing.assert_array_equal(z1, z0)
        eng.suffstats(sr, 17, qr)
        np.testing.assert_array_equal(eng.read_intermediate("var_x", B, Lm), q0)
        np.testing.assert_array_equal(eng.read_rows("lliks", 0, Lm), ll0)
        np.testing.assert_array_equal(eng.state_argmax()[0], z0)
        # the result stays in HBM for read_packed
        np.testing.assert_array_equal(eng.read_packed().buf, st2.buf)
        assert eng.suffstats(starts, Lm, q_e, read=False) is None
        np.testing.assert_array_equal(eng.read_packed().buf, st.buf)
    finally:
        eng.close()


def test_errors():
    rng = np.random.default_rng(0)
    T, K, D = 500, 4, 3
    obs = rng.normal(size=(T, D))
    eng = _engine()
    try:
        def bad(msg, fn, *a, **k):                 # the whole message, as the C ABI words it
            with pytest.raises(RuntimeError, match="^" + re.escape("svihmm_suffstats failed: svihmm_suffstats: " + msg) + "$"):
                fn(*a, **k)
        def cabi(st_, B_, Lm_, q_):
            return lambda: L.check(eng._lib.svihmm_suffstats(eng._h, st_, B_, Lm_, 0, q_, None), "svihmm_suffstats")
        st1, q1 = L.i64ptr(np.zeros(1, np.int64)), L.dptr(np.zeros(2 * K))
        # (straight to the C ABI: K is unknown yet)
        bad("no observations: call svihmm_set_obs first", cabi(st1, 1, 2, q1))
        eng.set_obs(obs)
        _globals(eng, K, rng)
        q = _posteriors(rng, 2, 10, K)
        bad("no emission family: call svihmm_set_emission_niw / _diag / _cat first", eng.suffstats, [0, 5], 10, q)
        diag = (rng.normal(size=(K, D)), np.ones((K, D)), 2 * np.ones((K, D)), np.ones((K, D)))
        eng.set_emission_diag(*diag)
        eng.suffstats([0, 5], 10, q)
        with pytest.raises(ValueError):            # K mismatch (posteriors)
            eng.suffstats([0, 5], 10, _posteriors(rng, 2, 10, K + 1))
        with pytest.raises(ValueError):            # wrongly shaped var_x
            eng.suffstats([0, 5], 10, q[:, :9])
        with pytest.raises(ValueError):            # B = 0
            eng.suffstats([], 10, np.zeros((0, 10, K)))
        bad("window 1 reaches outside [0, T)", eng.suffstats, [0, T - 9], 10, q)      # a window outside the sequence
        bad("window 0 reaches outside [0, T)", eng.suffstats, [-1, 5], 10, q)
        # (what the Python layer refuses itself, at the C ABI)
        bad("B and Lm must be positive", cabi(st1, 0, 2, q1))
        bad("B and Lm must be positive", cabi(st1, 1, 0, q1))
        bad("starts / var_x is NULL", cabi(None, 1, 2, q1))
        bad("starts / var_x is NULL", cabi(st1, 1, 2, None))
        eng.set_obs(rng.normal(size=(T, D + 1)))
        bad("emission D does not match obs D", eng.suffstats, [0, 5], 10, q)
        eng.set_obs(obs)
        eng.set_emission_diag(*diag)
        eng.suffstats([0, 5], 10, q)
        _globals(eng, K + 1, rng)                  # K of the globals != the family's K
        bad("K of the globals (%d) differs from the emission family's K (%d)" % (K + 1, K),
            eng.suffstats, [0, 5], 10, _posteriors(rng, 2, 10, K + 1))
    finally:
        eng.close()


# ---- class routes -------------------------------------------------------------------------------
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


class _MsgMeta(hmmsgd_metaobs.VBHMM):
    def forward_msgs(self, metaobs=None):
        super(_MsgMeta, self).forward_msgs(metaobs)


def _meta_model(family, engine, grow=False):
    if family == "niw":
        g = np.load(os.path.join(GOLDEN, "metaobs_K4_D2_L10_mask.npz"))
        K = int(g["K"])
        return _MsgMeta(g["obs"].copy(), np.ones(K), g["prior_tran"], _emit_from_fixture(g, K), tau=1.0,
                        kappa=0.7, metaobs_half=int(g["L"]), mb_sz=int(g["S"]), mask=g["mask"],
                        init_tran=g["init_tran"], maxit=3, seed=5, growBuffer=grow, engine=engine)
    rng = np.random.default_rng(11)
    K, T = 4, 800
    sts = np.repeat(rng.integers(0, K, size=T // 20), 20)
    mask = rng.random(T) < 0.1
    np.random.seed(2)
    if family == "diag":
        D = 3
        means = rng.normal(0, 4, size=(K, D))
        obs = means[sts] + rng.normal(size=(T, D))
        emit = np.array([DiagonalGaussian(mu=means[k] + rng.normal(size=D), mu_0=obs.mean(0), nus_0=0.01,
                                          alphas_0=2.0, betas_0=obs.var(0)) for k in range(K)])
    else:
        V = 6
        theta = rng.dirichlet(np.ones(V) * 0.3, size=K)
        obs = np.array([rng.choice(V, p=theta[s]) for s in sts], dtype=float)
        emit = np.array([Categorical(alphav_0=np.ones(V) * 0.5) for _ in range(K)])
    return _MsgMeta(obs, np.ones(K), np.ones((K, K)), emit, tau=1.0, kappa=0.7, metaobs_half=6, mb_sz=5,
                    mask=mask, maxit=3, seed=4, growBuffer=grow, engine=engine)


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


def _agree(a, b):
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=1e-9)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=1e-9)
    for x, y in zip(_factors(a), _factors(b)):
        np.testing.assert_allclose(x, y, rtol=1e-9, atol=1e-12)


def _forbid(monkeypatch, cls, name):
    def boom(*a, **k):
        raise AssertionError("the host statistics ran: %s.%s" % (cls.__name__, name))
    monkeypatch.setattr(cls, name, boom)


@pytest.mark.parametrize("family,grow", [("niw", False), ("diag", False), ("cat", False), ("niw", True)])
def test_metaobs_message_override_keeps_device_statistics(monkeypatch, family, grow):
    host = _meta_model(family, OracleEngine(), grow)
    host.infer()
    dev = _meta_model(family, None, grow)
    assert dev._suffstats_route()
    _forbid(monkeypatch, hmmsgd_metaobs.VBHMM, "_intermediate")
    dev.engine.profile(True)
    dev.infer()
    assert dev.engine.profile_read().get("stats", (0, 0))[1] >= dev.maxit
    _agree(dev, host)


@pytest.mark.parametrize("name,mod", [("batchcd_K4_D2_T300", hmmbatchcd), ("batchsgd_K4_D3_T250", hmmbatchsgd)])
def test_batch_local_update_override_keeps_device_statistics(monkeypatch, name, mod):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K = int(g["K"])

    class Sub(mod.VBHMM):
        def local_update(self, obs=None, mask=None):
            super(Sub, self).local_update(obs, mask)

    def make(engine):
        kw = dict(mask=g["mask"], init_tran=g["init_tran"], maxit=int(g["maxit"]), engine=engine)
        if mod is hmmbatchsgd:
            kw.update(tau=1.0, kappa=0.7)
        return Sub(g["obs"].copy(), g["prior_init"], g["prior_tran"], _emit_from_fixture(g, K), **kw)

    host = make(OracleEngine())
    host.infer()
    dev = make(None)
    _forbid(monkeypatch, mod.VBHMM, "global_update")
    dev.infer()
    _agree(dev, host)
    np.testing.assert_allclose(dev.var_init, host.var_init, rtol=1e-9)
