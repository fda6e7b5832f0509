"""svihmm_ffbs_windows / Engine.ffbs_windows / VBHMM.ffbs_windows on the MI355X.

Paths are checked step by step against the NumPy draw rule (tests/ffbs_helpers.py) on the device's own
lalpha: every step is recomputed from the path's own z[t+1], and a step may differ only where u * tot is
within 1e-11 tot of the boundary between the two states -- at most ONE such step per test (none is expected:
tests/test_ffbs_windows_ref.py counts them for these sizes).  Windows below 2048 rows take the
lane-per-(window, draw) kernel (K <= 64 in registers, wider models in three passes), longer ones the blocked
composition of svihmm_ffbs once per (window, draw)."""
import re

import numpy as np
import pytest
from scipy.special import digamma

from oracle import ref_numpy as R
from pysvihmm_amd import _lib as L
from tests.ffbs_helpers import check_paths
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu

_PROBLEMS = {}


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _fresh():
    from pysvihmm_amd.engine import HipEngine
    return HipEngine(0)


def _problem(K, T=700, D=3, miss=0.0):
    key = (K, T, D, miss)
    if key not in _PROBLEMS:
        _PROBLEMS[key] = make_problem(K, D, T, seed=K + T, miss=miss)
    return _PROBLEMS[key]


def _push(e, p):
    e.set_obs(p["obs"], p["mask"])
    e.set_globals(p["mod_init"], p["ltran"])
    e.set_emission_niw(p["mu"], p["sigma"], p["kappa"], p["nu"])


def _logA(K, seed):
    """The sampler's transition: not the filter's ltran, un-normalised like ffbs_fast's log(var_tran + eps)."""
    rng = np.random.default_rng(seed)
    return np.log(3.0 * (0.6 * np.eye(K) + 0.4 * rng.dirichlet(np.ones(K), size=K)))


def _philox_uniforms(seed, S, B, Lm):
    w = R.philox4x32_10(seed, np.arange(S * B * Lm, dtype=np.uint64), 0)
    return R._u53(w[0], w[1]).reshape(S, B, Lm)


def _starts(T, B, Lm, seed):
    return np.random.default_rng(seed).integers(0, T - Lm + 1, size=B)


def _checked(e, starts, Lm, logA, S, seed, flags=0, what=""):
    B = len(starts) if starts is not None else None
    nb = B if B is not None else e._host_ll_windows
    u = np.random.default_rng(seed).random((S, nb, Lm))
    z, la = e.ffbs_windows(starts, Lm, logA, n_draws=S, uniforms=u, flags=flags, want_lalpha=True)
    assert z.dtype == np.int32 and z.shape == (S, nb, Lm) and la.shape == (nb, Lm, e.K)
    assert np.all(np.isfinite(la))
    excused = check_paths(z, la, logA, u)
    print("%s K=%d B=%d Lm=%d S=%d: %d steps, %d excused" % (what, e.K, nb, Lm, S, z.size, excused))
    assert excused <= 1
    return z, la, u


# ---- forward filter ---------------------------------------------------------------------------------
@pytest.mark.parametrize("K,B,Lm", [(3, 1, 1), (16, 5, 33), (64, 5, 257), (100, 3, 40)])
def test_filter_is_forward_backwards(eng, K, B, Lm):
    p = _problem(K)
    _push(eng, p)
    starts = _starts(p["T"], B, Lm, K)
    want = eng.forward_backward(starts, Lm, want=("lalpha",))["lalpha"]
    z, la = eng.ffbs_windows(starts, Lm, _logA(K, 1), n_draws=2, seed=3, want_lalpha=True)
    np.testing.assert_array_equal(la, want)
    z2, none = eng.ffbs_windows(starts, Lm, _logA(K, 1), n_draws=2, seed=3)
    assert none is None
    np.testing.assert_array_equal(z2, z)
    # afterwards lalpha of these windows is the readable intermediate
    np.testing.assert_array_equal(eng.read_intermediate("lalpha", B, Lm), want)


# ---- window kernel ----------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [3, 16, 17, 64])
@pytest.mark.parametrize("B,Lm,S", [(1, 1, 1), (1, 2, 3), (5, 257, 1), (5, 33, 130), (70, 9, 3)])
def test_shape_grid(eng, K, B, Lm, S):
    p = _problem(K)
    _push(eng, p)
    _checked(eng, _starts(p["T"], B, Lm, 7 * K + B), Lm, _logA(K, K), S, seed=1000 * K + 10 * Lm + S, what="grid")


@pytest.mark.parametrize("K", [65, 200])
def test_wide(eng, K):
    p = _problem(K)
    _push(eng, p)
    _checked(eng, _starts(p["T"], 3, 40, K), 40, _logA(K, K), 5, seed=K, what="wide")


def test_placement_independence(eng):
    K, B, Lm, S = 16, 5, 33, 130
    p = _problem(K)
    _push(eng, p)
    starts = _starts(p["T"], B, Lm, 11)
    logA = _logA(K, 2)
    z, la, u = _checked(eng, starts, Lm, logA, S, seed=5, what="placement")
    for s in (0, 1, 63, 64, 129):                          # a draw alone: other lanes, other waves
        z1, _ = eng.ffbs_windows(starts, Lm, logA, n_draws=1, uniforms=u[s:s + 1])
        np.testing.assert_array_equal(z1[0], z[s])
    for b in range(B):                                     # a window alone
        zb, _ = eng.ffbs_windows(starts[b:b + 1], Lm, logA, n_draws=S, uniforms=np.ascontiguousarray(u[:, b:b + 1]))
        np.testing.assert_array_equal(zb[:, 0], z[:, b])


# ---- Philox mode ------------------------------------------------------------------------------------
def test_philox_mode_window_kernel(eng):
    K, B, Lm, S, seed = 16, 3, 20, 70, 0x1234567890ABCDEF
    p = _problem(K)
    _push(eng, p)
    starts = _starts(p["T"], B, Lm, 3)
    logA = _logA(K, 4)
    zp, _ = eng.ffbs_windows(starts, Lm, logA, n_draws=S, seed=seed)
    zu, _ = eng.ffbs_windows(starts, Lm, logA, n_draws=S, uniforms=_philox_uniforms(seed, S, B, Lm))
    np.testing.assert_array_equal(zp, zu)
    z2, _ = eng.ffbs_windows(starts, Lm, logA, n_draws=S, seed=seed + 1)
    assert not np.array_equal(z2, zp)


# ---- long route -------------------------------------------------------------------------------------
def test_long_route_whole_chain(eng):
    K, T = 5, 4100
    p = _problem(K, T=T)
    _push(eng, p)
    logA = _logA(K, 6)
    u = np.random.default_rng(8).random(T)
    zf, laf = eng.ffbs(logA, u)
    z, la = eng.ffbs_windows([0], T, logA, n_draws=1, uniforms=u[None, None, :], want_lalpha=True)
    np.testing.assert_array_equal(la[0], laf)
    np.testing.assert_array_equal(z[0, 0], zf)             # the same kernels on the same lalpha
    assert check_paths(z, la, logA, u[None, None, :]) <= 1
    _checked(eng, [0], T, logA, 3, seed=9, what="chain")
    # Philox mode on the long route: the uniform row is generated on the device
    seed = 77
    zp, _ = eng.ffbs_windows([0], T, logA, n_draws=2, seed=seed)
    zu, _ = eng.ffbs_windows([0], T, logA, n_draws=2, uniforms=_philox_uniforms(seed, 2, 1, T))
    np.testing.assert_array_equal(zp, zu)


def test_long_route_two_windows(eng):
    p = _problem(5, T=4100)
    _push(eng, p)
    _checked(eng, [0, 1600], 2500, _logA(5, 6), 2, seed=10, what="long windows")


def test_long_route_wide(eng):
    p = _problem(100, T=2300)
    _push(eng, p)
    _checked(eng, [0], 2300, _logA(100, 6), 2, seed=12, what="long wide")


# ---- logA with -inf ---------------------------------------------------------------------------------
def test_forbidden_transitions(eng):
    K, B, Lm, S = 16, 4, 50, 20
    p = _problem(K)
    _push(eng, p)
    band = np.abs(np.arange(K)[:, None] - np.arange(K)[None, :]) <= 1
    logA = np.where(band, _logA(K, 3), -np.inf)
    z, la, u = _checked(eng, _starts(p["T"], B, Lm, 5), Lm, logA, S, seed=13, what="banded")
    assert np.all(logA[z[..., :-1], z[..., 1:]] > -np.inf)
    assert len(np.unique(z)) > 3
    dead = logA.copy()
    dead[:, 5] = -np.inf
    with pytest.raises(RuntimeError, match="no finite entry"):
        eng.ffbs_windows([0], Lm, dead, n_draws=1)
    for v in (np.inf, np.nan):
        bad = _logA(K, 3)
        bad[2, 7] = v
        with pytest.raises(RuntimeError, match="NaN or \\+inf"):
            eng.ffbs_windows([0], Lm, bad, n_draws=1)
    _checked(eng, [0], Lm, logA, 1, seed=14, what="after the failures")


# ---- families and flags -----------------------------------------------------------------------------
@pytest.mark.parametrize("family", ["diag", "cat", "mask_as_nan", "host_lliks"])
def test_families_and_flags(eng, family):
    K, B, Lm, S, T, D = 4, 3, 12, 4, 200, 3
    rng = np.random.default_rng(31)
    sts = np.repeat(rng.integers(0, K, size=T // 20), 20)
    var_tran = 1.0 + 20 * np.eye(K) + rng.random((K, K))
    vi = rng.random(K) + 0.1
    eps = 1e-9
    mod_init = digamma(vi + eps) - digamma(vi.sum() + eps)
    ltran = digamma(var_tran + eps) - digamma(var_tran.sum(1)[:, None] + eps)
    means = rng.normal(0, 3, size=(K, D))
    obs = means[sts] + rng.normal(size=(T, D))
    starts, flags = np.array([0, 37, T - Lm]), 0
    if family == "diag":
        eng.set_obs(obs)
        eng.set_globals(mod_init, ltran)
        eng.set_emission_diag(means + 0.3 * rng.normal(size=(K, D)), 1.0 + rng.random((K, D)),
                              2.0 + rng.random((K, D)), 1.0 + rng.random((K, D)))
    elif family == "cat":
        V = 6
        theta = rng.dirichlet(np.ones(V) * 0.4, size=K)
        sym = np.array([rng.choice(V, p=theta[s]) for s in sts], dtype=float)[:, None]
        a = 0.5 + 40 * theta
        eng.set_obs(sym)
        eng.set_globals(mod_init, ltran)
        eng.set_emission_cat(digamma(a) - digamma(a.sum(1))[:, None])
    elif family == "mask_as_nan":
        mask = np.zeros(T, dtype=bool)
        mask[40:46] = True                                  # a masked stretch inside the second window
        A = rng.normal(size=(K, D, D))
        eng.set_obs(obs, mask)
        eng.set_globals(mod_init, ltran)
        eng.set_emission_niw(means, np.einsum('kij,klj->kil', A, A) + (D + 2.0) * np.eye(D), np.ones(K),
                             D + 2.0 + np.zeros(K))
        flags = L.MASK_AS_NAN
        ll = eng.loglik(starts, Lm, flags=flags)
        assert np.all(ll[1, 3:9] == 0.0) and np.all(ll[1, :3] != 0.0)
    else:
        eng.set_globals(mod_init, ltran)
        eng.set_lliks(rng.normal(size=(B, Lm, K)) * 2.0)
        starts, flags = None, L.USE_HOST_LLIKS
    z, la, u = _checked(eng, starts, Lm, _logA(K, 9), S, seed=15, flags=flags, what=family)
    if family == "mask_as_nan":                             # the flag reached the filter
        np.testing.assert_array_equal(la, eng.forward_backward(starts, Lm, flags=flags, want=("lalpha",))["lalpha"])
        assert not np.array_equal(la, eng.forward_backward(starts, Lm, flags=0, want=("lalpha",))["lalpha"])


# ---- distribution -----------------------------------------------------------------------------------
DIST_SEED = 20261018   # chosen by running the NumPy sampler (ffbs_helpers.backward_sample) alone on the CPU,
                       # on the CPU oracle's lliks of this model with these Philox uniforms: it passes the bounds below


def _dist_model():
    p = make_problem(3, 2, 60, seed=5, sep=0.5)
    return p, np.array([3, 30]), 5, 20000


def _fb_numpy(ll, mod_init, ltran):
    Lm, K = ll.shape
    la, lb = np.empty((Lm, K)), np.zeros((Lm, K))
    la[0] = mod_init + ll[0]
    for t in range(1, Lm):
        la[t] = np.logaddexp.reduce(la[t - 1][:, None] + ltran, axis=0) + ll[t]
    for t in range(Lm - 2, -1, -1):
        lb[t] = np.logaddexp.reduce(ltran + (lb[t + 1] + ll[t + 1])[None, :], axis=1)
    return la, lb


def _posteriors_numpy(ll, mod_init, ltran):
    """(var_x [Lm, K], pairwise posterior of (z_t, z_{t+1}) [Lm - 1, K, K]) of one window."""
    la, lb = _fb_numpy(ll, mod_init, ltran)
    lz = np.logaddexp.reduce(la[-1])
    q = np.exp(la + lb - lz)
    xi = np.exp(la[:-1, :, None] + ltran[None] + (ll[1:] + lb[1:])[:, None, :] - lz)
    return q, xi


def _check_frequencies(z, var_x, xi):
    """z [S, Lm] of one window against its smoothing marginals and pair posteriors."""
    S, Lm = z.shape
    K = var_x.shape[1]
    freq = np.stack([(z == k).mean(axis=0) for k in range(K)], axis=1)
    bound = 5.0 * np.sqrt(var_x * (1.0 - var_x) / S) + 1e-3
    worst = float(np.max(np.abs(freq - var_x) - bound))
    assert np.all(np.abs(freq - var_x) <= bound), worst
    pair = np.zeros((Lm - 1, K, K))
    for t in range(Lm - 1):
        np.add.at(pair[t], (z[:, t], z[:, t + 1]), 1.0 / S)
    pb = 5.0 * np.sqrt(xi * (1.0 - xi) / S) + 1e-3
    assert np.all(np.abs(pair - xi) <= pb), float(np.max(np.abs(pair - xi) - pb))
    return worst


def test_distribution(eng):
    p, starts, Lm, S = _dist_model()
    _push(eng, p)
    z, _ = eng.ffbs_windows(starts, Lm, p["ltran"], n_draws=S, seed=DIST_SEED)    # logA = ltran: the smoothing posterior
    r = eng.forward_backward(starts, Lm, want=("var_x",))
    ll = eng.loglik(starts, Lm)
    for b in range(len(starts)):
        q, xi = _posteriors_numpy(ll[b], p["mod_init"], p["ltran"])
        np.testing.assert_allclose(q, r["var_x"][b], rtol=1e-9, atol=1e-12)
        assert np.sum((q > 0.05) & (q < 0.95)) >= 2 * Lm and len(np.unique(z[:, b])) == 3     # no degenerate posterior
        print("window %d: worst |freq - var_x| - bound = %.3g" % (b, _check_frequencies(z[:, b], r["var_x"][b], xi)))


# ---- bookkeeping ------------------------------------------------------------------------------------
def test_packed_statistics_and_precision_survive():
    p = make_problem(16, 4, 6000, seed=2, miss=0.1)
    B, Lm = 256, 65
    starts = np.random.default_rng(1).integers(0, p["T"] - Lm + 1, size=B)
    e = _fresh()
    try:
        _push(e, p)
        e.set_precision("f32")
        e.estep(starts, Lm, flags=L.TRANS_WRAP, read=False)
        want = e.read_packed().buf.copy()
        e.estep(starts, Lm, flags=L.TRANS_WRAP, read=False)
        mode = e.precision()
        assert mode[0] == "f32"
        logA = _logA(16, 1)
        _checked(e, starts[:7], Lm, logA, 3, seed=16, what="f32 mode")
        _checked(e, [100], 2100, logA, 1, seed=17, flags=L.MASK_AS_NAN, what="f32 mode, chain")
        assert e.precision() == mode
        np.testing.assert_array_equal(e.read_packed().buf, want)
    finally:
        e.close()


# ---- errors -----------------------------------------------------------------------------------------
def test_errors_leave_the_engine_usable():
    rng = np.random.default_rng(0)
    T, K, D = 300, 4, 3
    obs = rng.normal(size=(T, D))
    logA = _logA(K, 1)
    e = _fresh()
    try:
        def bad_call(msg, fn):                            # the whole message, as the C ABI words it
            e.profile_reset()
            with pytest.raises(RuntimeError,
                               match="^" + re.escape("svihmm_ffbs_windows failed: svihmm_ffbs_windows: " + msg) + "$"):
                fn()
            assert not e.profile_read()                   # nothing was launched or copied
        def bad(msg, *a, **k):
            bad_call(msg, lambda: e.ffbs_windows(*a, **k))
        def cabi(st_, la_, out_):
            return lambda: L.check(e._lib.svihmm_ffbs_windows(e._h, st_, 1, 5, 0, la_, 1, None, 0, out_, None),
                                   "svihmm_ffbs_windows")
        host = "SVIHMM_USE_HOST_LLIKS without uploaded lliks of shape [B, Lm, K] (svihmm_set_lliks)"
        outside = "window %d reaches outside [0, T)"
        e.profile(True)
        st0, out0 = np.zeros(1, np.int64), np.empty(5, dtype=np.int32)
        bad_call("no globals: call svihmm_set_globals first",       # (C ABI: the engine has no K yet)
                 cabi(L.i64ptr(st0), L.dptr(logA), out0.ctypes.data))
        mi = np.log(rng.dirichlet(np.ones(K)))
        lt = np.log(rng.dirichlet(np.ones(K), size=K))
        e.set_globals(mi, lt)
        bad("no observations: call svihmm_set_obs first", [0], 5, logA)
        bad(host, [0], 5, logA, flags=L.USE_HOST_LLIKS)   # no host lliks either
        e.set_obs(obs)
        bad("no emission family: call svihmm_set_emission_niw / _diag / _cat first", [0], 5, logA)
        A = rng.normal(size=(K, D, D))
        niw = (rng.normal(size=(K, D)), np.einsum('kij,klj->kil', A, A) + D * np.eye(D), np.ones(K), D + 2.0 + np.zeros(K))
        e.set_emission_niw(*niw)
        u = rng.random((2, 2, 5))
        z, _ = e.ffbs_windows([0, 7], 5, logA, n_draws=2, uniforms=u)
        bad("S, B and Lm must be positive", [], 5, logA)
        bad("S, B and Lm must be positive", [0], 0, logA)
        bad("S, B and Lm must be positive", [0], 5, logA, n_draws=0)
        bad(outside % 0, [T - 4], 5, logA)                # window past the end
        bad(outside % 1, [0, -1], 5, logA)                # ... and before the start
        st = np.zeros(1, np.int64)
        out = np.empty(5, dtype=np.int32)
        bad_call("starts is NULL", cabi(None, L.dptr(logA), out.ctypes.data))      # (C ABI)
        e.set_obs(rng.normal(size=(T, D + 1)))
        bad("emission D does not match obs D", [0], 5, logA)
        e.set_obs(obs)
        e.set_emission_niw(*niw)
        e.set_lliks(rng.normal(size=(2, 6, K)))
        bad(host, [0, 0], 5, logA, flags=L.USE_HOST_LLIKS)      # host lliks of another shape
        bad(host, [0], 6, logA, flags=L.USE_HOST_LLIKS)
        for la_, out_ in ((None, out.ctypes.data), (L.dptr(logA), None)):      # NULL logA / out_z (C ABI)
            bad_call("logA and out_z must be given", cabi(L.i64ptr(st), la_, out_))
        e.set_globals(np.log(rng.dirichlet(np.ones(K + 1))), np.log(rng.dirichlet(np.ones(K + 1), size=K + 1)))
        bad("K of the globals (%d) differs from the emission family's K (%d)" % (K + 1, K), [0], 5, _logA(K + 1, 1))
        Kw = 257
        e.set_globals(np.zeros(Kw), np.zeros((Kw, Kw)))
        e.set_lliks(np.zeros((1, 3, Kw)))
        bad("K = 257 > 256 not supported", [0], 3, np.zeros((Kw, Kw)), flags=L.USE_HOST_LLIKS)
        # still usable
        e.profile(False)
        e.set_globals(mi, lt)
        z2, _ = e.ffbs_windows([0, 7], 5, logA, n_draws=2, uniforms=u)
        np.testing.assert_array_equal(z2, z)
    finally:
        e.close()


# ---- class surface ----------------------------------------------------------------------------------
def test_class_ffbs_windows_on_the_two_blob_demo():
    from pysvihmm_amd import hmmsgd_metaobs
    from pysvihmm_amd.distributions import Gaussian
    from pysvihmm_amd.hmmsgd_metaobs import MetaObs
    rng = np.random.RandomState(5)
    np.random.seed(5)
    N, K, D = 600, 2, 2
    sts = (np.arange(N) >= N // 2).astype(int)
    obs = rng.randn(N, D) + 5.0 * sts[:, None]
    prior_emit = np.array([Gaussian(mu_0=np.zeros(D), sigma_0=0.75 * np.cov(obs.T), kappa_0=0.01, nu_0=4)
                           for _ in range(K)])
    svi = hmmsgd_metaobs.VBHMM(obs, np.ones(K), np.ones((K, K)), prior_emit, metaobs_half=10, mb_sz=8,
                               maxit=60, seed=3)
    svi.infer()
    before = (svi.var_tran.copy(), svi.var_init.copy(), [e.mu.copy() for e in svi.var_emit])
    u = rng.random_sample(N)
    z = svi.ffbs_windows(None, n_draws=1, var_init=svi.var_init, uniforms=u[None, None, :])
    zf, la = svi.ffbs_fast(svi.var_init, uniforms=u)
    assert z.shape == (1, 1, N) and z.dtype == np.int32
    # T < 1024: ffbs_fast draws with the sequential single-wave sampler (p / tot, u <= cumsum): the same
    # path up to the excuse rule
    logA = np.log(svi.var_tran + np.finfo(np.float64).eps)
    n1 = check_paths(z[0, 0], la, logA, u)
    n2 = check_paths(zf.astype(np.int32), la, logA, u)
    assert n1 + n2 <= 1
    if n1 + n2 == 0:
        np.testing.assert_array_equal(z[0, 0], zf)
    assert np.mean(z[0, 0] == zf) > 0.99
    # a list of meta-observations, draws reproducible through np.random.seed
    mos = [MetaObs(10, 30), MetaObs(290, 310), MetaObs(579, 599)]
    np.random.seed(11)
    za = svi.ffbs_windows(mos, n_draws=4)
    np.random.seed(11)
    zb = svi.ffbs_windows(mos, n_draws=4)
    assert za.shape == (4, 3, 21)
    np.testing.assert_array_equal(za, zb)
    zc = svi.ffbs_windows(MetaObs(290, 310), n_draws=2, seed=5)
    assert zc.shape == (2, 1, 21)
    with pytest.raises(RuntimeError, match="equal lengths"):
        svi.ffbs_windows([MetaObs(10, 30), MetaObs(40, 61)])
    assert np.array_equal(svi.var_tran, before[0]) and np.array_equal(svi.var_init, before[1])
    assert all(np.array_equal(e.mu, m) for e, m in zip(svi.var_emit, before[2]))
