"""svihmm_viterbi / Engine.viterbi / VBHMM.viterbi on the MI355X.

Given identical lliks the device path and score have to EQUAL the NumPy recursion of
tests/viterbi_helpers.py (the operation order is part of the C ABI's contract), so most cases here
demand exact equality.  Lengths: the kernels keep psi in LDS up to 1008 rows (K <= 64) / 240 rows
(K > 64) and backtrack longer windows in chunks of that many rows (kernels_viterbi.h), hence the
cases either side of 1008 / 240, at exact multiples, and with a ragged last chunk."""
import os
import re

import numpy as np
import pytest
from scipy.special import digamma

from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from tests.viterbi_helpers import path_score, viterbi_batch, viterbi_numpy

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
EPS = 1e-9


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _fresh():
    from pysvihmm_amd.engine import HipEngine
    return HipEngine(0)


def _tran(rng, K, kind):
    if kind == "sticky":          # paths coalesce within a few rows
        A = 0.98 * np.eye(K) + 0.02 * rng.dirichlet(np.ones(K), size=K)
    elif kind == "flat":          # near-uniform: with weak emissions the back-pointers differ from row to row
        A = rng.dirichlet(np.ones(K) * 200.0, size=K)
    elif kind == "cycle":         # state i -> i + 1: the back-pointer maps are bijections, paths never coalesce
        A = 0.9 * np.roll(np.eye(K), 1, axis=1) + 0.1 * rng.dirichlet(np.ones(K), size=K)
    else:
        A = rng.dirichlet(np.ones(K), size=K)
    return np.log(A / A.sum(1)[:, None])


def _chunk_map(ll, mod_init, ltran, lo, hi):
    """Entry state at row ``hi`` -> state at row ``lo`` along the back-pointers (NumPy)."""
    delta = mod_init + ll[0]
    psi = np.zeros(ll.shape, dtype=np.int64)
    for t in range(1, hi + 1):
        m = delta[:, None] + ltran
        psi[t] = np.argmax(m, axis=0)
        delta = m.max(0) + ll[t]
    cur = np.arange(ll.shape[1])
    for t in range(hi, lo, -1):
        cur = psi[t][cur]
    return cur


def _host_case(eng, K, B, Lm, seed, kind="random", ll_scale=2.0, distinct=None):
    rng = np.random.default_rng(seed)
    ll = rng.normal(size=(B, Lm, K)) * ll_scale
    mod_init = np.log(rng.dirichlet(np.ones(K)))
    ltran = _tran(rng, K, kind)
    if distinct is not None:      # the map of one whole chunk is not constant: composing the maps matters
        assert len(np.unique(_chunk_map(ll[0], mod_init, ltran, *distinct))) > 1
    return _host_exact(eng, ll, mod_init, ltran)


def _host_exact(eng, ll, mod_init, ltran):
    B, Lm, K = ll.shape
    eng.set_globals(mod_init, ltran)
    eng.set_lliks(ll)
    z, score = eng.viterbi(np.zeros(B, np.int64), Lm, flags=L.USE_HOST_LLIKS)
    zr, sr = viterbi_batch(ll, mod_init, ltran)
    assert z.dtype == np.int32 and z.shape == (B, Lm) and score.shape == (B,)
    np.testing.assert_array_equal(z, zr)
    np.testing.assert_array_equal(score, sr)              # bit-equal
    return z, score


# ---- exact, host-lliks route ---------------------------------------------------------------------
@pytest.mark.parametrize("K", [2, 5, 16, 17, 64])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("Lm", [1, 2, 7, 33])
def test_wave_kernel_lds_backtrack(eng, K, B, Lm):
    _host_case(eng, K, B, Lm, seed=1000 * K + 10 * Lm + B)


@pytest.mark.parametrize("K", [65, 200, 256])
def test_wide_kernel(eng, K):
    _host_case(eng, K, 2, 9, seed=K)


def test_score_only_and_path_only(eng):
    rng = np.random.default_rng(8)
    ll = rng.normal(size=(3, 40, 7))
    mi, lt = np.log(rng.dirichlet(np.ones(7))), _tran(rng, 7, "random")
    z, s = _host_exact(eng, ll, mi, lt)
    z0, s0 = eng.viterbi(np.zeros(3, np.int64), 40, flags=L.USE_HOST_LLIKS, want_z=False)
    assert z0 is None
    np.testing.assert_array_equal(s0, s)
    out = np.empty((3, 40), dtype=np.int32)               # out_score = NULL at the C ABI
    st = np.zeros(3, np.int64)
    L.check(eng._lib.svihmm_viterbi(eng._h, L.i64ptr(st), 3, 40, L.USE_HOST_LLIKS, out.ctypes.data, None),
            "svihmm_viterbi")
    np.testing.assert_array_equal(out, z)


# K <= 64: psi in LDS up to 1008 rows, chunks of 1008 rows beyond
@pytest.mark.parametrize("kind", ["sticky", "flat", "cycle"])
@pytest.mark.parametrize("K", [5, 17, 64])
@pytest.mark.parametrize("B,Lm", [(1, 1008), (1, 1009), (1, 2016), (1, 2017), (1, 2047), (1, 2048), (1, 5000), (3, 3000)])
def test_long_windows(eng, K, kind, B, Lm):
    """sticky: the paths coalesce within a few rows; flat: near-uniform transitions, weak emissions;
    cycle: back-pointer maps that stay bijections over a whole chunk (checked in NumPy for the windows
    of three chunks and more), so a wrong composition of the chunk maps cannot go unnoticed."""
    scale = {"sticky": 2.0, "flat": 0.05, "cycle": 0.01}[kind]
    distinct = (1008, 2016) if kind == "cycle" and Lm > 2016 else None
    _host_case(eng, K, B, Lm, seed=K + Lm + B, kind=kind, ll_scale=scale, distinct=distinct)


@pytest.mark.parametrize("B,Lm", [(2, 240), (2, 241), (1, 5000)])
def test_wide_long_windows(eng, B, Lm):
    _host_case(eng, 130, B, Lm, seed=Lm)


# ---- ties ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Lm", [(5, 50), (64, 1500), (100, 300)])
def test_all_ties_give_the_zero_path(eng, K, Lm):
    z, score = _host_exact(eng, np.zeros((2, Lm, K)), np.zeros(K), np.zeros((K, K)))
    assert not z.any() and not score.any()


@pytest.mark.parametrize("K,Lm", [(4, 60), (64, 70), (7, 1300), (90, 300)])
def test_integer_inputs_with_many_ties(eng, K, Lm):
    rng = np.random.default_rng(K * Lm)
    ll = rng.integers(-1, 2, size=(2, Lm, K)).astype(float)
    _host_exact(eng, ll, np.zeros(K), rng.integers(-1, 1, size=(K, K)).astype(float))


# ---- range --------------------------------------------------------------------------------------
@pytest.mark.parametrize("K,Lm", [(6, 40), (64, 1100), (80, 30)])
def test_transition_range(eng, K, Lm):
    """ltran at -1000 (psi of a 1e-3 pseudo-count) and -inf, one finite entry kept per column: no slow
    route, no error, exact."""
    rng = np.random.default_rng(K)
    ltran = _tran(rng, K, "random")
    ltran[rng.random((K, K)) < 0.3] = -1000.0
    ltran[rng.random((K, K)) < 0.3] = -np.inf
    keep = rng.integers(0, K, size=K)
    ltran[keep, np.arange(K)] = np.log(0.5)
    assert np.isneginf(ltran).any() and (ltran == -1000.0).any()
    ll = rng.normal(size=(2, Lm, K))
    mod_init = np.log(rng.dirichlet(np.ones(K)))
    mod_init[0] = -np.inf
    z, score = _host_exact(eng, ll, mod_init, ltran)
    assert np.all(np.isfinite(score))


# ---- device emission ----------------------------------------------------------------------------
def _psi(var_init, var_tran):
    return (digamma(var_init + EPS) - digamma(var_init.sum() + EPS),
            digamma(var_tran + EPS) - digamma(var_tran.sum(1)[:, None] + EPS))


def _fixture_model(name):
    g = np.load(os.path.join(GOLDEN, name + ".npz"))
    K = int(g["K"])
    mod_init, ltran = _psi(np.ones(K), np.asarray(g["init_tran"], dtype=np.float64))
    em = ("niw", (g["init_mu"], g["init_sigma"], g["init_kappa"], g["init_nu"]))
    return g["obs"], g["mask"], mod_init, ltran, em, 2 * int(g["L"]) + 1


def _synthetic_model(family):
    rng = np.random.default_rng(21)
    K, T = 6, 700
    sts = np.repeat(rng.integers(0, K, size=T // 25), 25)
    mask = rng.random(T) < 0.1
    mod_init, ltran = _psi(rng.random(K) + 0.1, 1.0 + 30 * np.eye(K) + rng.random((K, K)))
    if family == "diag":
        D = 3
        means = rng.normal(0, 3, size=(K, D))
        obs = means[sts] + rng.normal(size=(T, D))
        em = ("diag", (means + 0.3 * rng.normal(size=(K, D)), 1.0 + rng.random((K, D)), 2.0 + rng.random((K, D)),
                       1.0 + rng.random((K, D))))
    else:
        V = 7
        theta = rng.dirichlet(np.ones(V) * 0.4, size=K)
        obs = np.array([rng.choice(V, p=theta[s]) for s in sts], dtype=float)[:, None]
        a = 0.5 + 40 * theta
        em = ("cat", (digamma(a) - digamma(a.sum(1))[:, None],))
    return obs, mask, mod_init, ltran, em, 21


def _push(e, obs, mask, mod_init, ltran, em):
    e.set_obs(obs, mask)
    e.set_globals(mod_init, ltran)
    getattr(e, "set_emission_" + em[0])(*em[1])


@pytest.mark.parametrize("model,flags", [
    ("metaobs_K4_D2_L10_mask", 0), ("metaobs_K4_D2_L10_mask", L.MASK_AS_NAN), ("metaobs_K16_D8_L16", L.MASK_AS_NAN),
    ("diag", L.MASK_AS_NAN), ("cat", L.MASK_AS_NAN)])
def test_device_emission(eng, model, flags):
    obs, mask, mod_init, ltran, em, Lw = _fixture_model(model) if model.startswith("metaobs") else _synthetic_model(model)
    T = obs.shape[0]
    _push(eng, obs, mask, mod_init, ltran, em)
    ora = OracleEngine()
    _push(ora, obs, mask, mod_init, ltran, em)
    rng = np.random.default_rng(4)
    for starts, Lm in ((rng.integers(0, T - Lw + 1, size=3), Lw), ([0], T)):
        z, score = eng.viterbi(starts, Lm, flags=flags)
        # exact against NumPy on the engine's own lliks
        ll = eng.loglik(starts, Lm, flags=flags)
        zr, sr = viterbi_batch(ll, mod_init, ltran)
        np.testing.assert_array_equal(z, zr)
        np.testing.assert_array_equal(score, sr)
        # after the call the lliks of these windows are the readable intermediate
        z2, _ = eng.viterbi(starts, Lm, flags=flags)
        np.testing.assert_array_equal(eng.read_intermediate("lliks", len(starts), Lm), ll)
        np.testing.assert_array_equal(z2, z)
        # optimality under the CPU oracle's lliks: the device path, re-scored there, reaches the oracle's
        # optimum to the project's fp64 contract (1e-6 relative to |score|), every row included
        llo = ora.loglik(starts, Lm, flags=flags)
        for b in range(len(starts)):
            _, opt = viterbi_numpy(llo[b], mod_init, ltran)
            got = path_score(z[b], llo[b], mod_init, ltran)
            print("%s flags=%d Lm=%d window %d: oracle optimum %.12g, device path re-scored %.12g"
                  % (model, flags, Lm, b, opt, got))
            assert got <= opt + 1e-9 * abs(opt)
            assert opt - got <= 1e-6 * abs(opt)


# ---- independence -------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Lm", [(8, 33), (256, 65)])
def test_packed_statistics_survive_a_viterbi_call(B, Lm):
    from tests.helpers import make_problem
    p = make_problem(16, 4, 6000, seed=B, miss=0.1)
    starts = np.random.default_rng(1).integers(0, p["T"] - Lm + 1, size=B)
    e = _fresh()
    try:
        e.set_obs(p["obs"], p["mask"])
        e.set_globals(p["mod_init"], p["ltran"])
        e.set_emission_niw(p["mu"], p["sigma"], p["kappa"], p["nu"])
        e.estep(starts, Lm, flags=L.TRANS_WRAP, read=False)
        want = e.read_packed().buf.copy()
        e.estep(starts, Lm, flags=L.TRANS_WRAP, read=False)
        mode = e.precision()
        z, score = e.viterbi(np.minimum(starts[:5], p["T"] - 1500), 1500)            # (long windows: the HBM psi / path buffers too)
        zs, _ = e.viterbi(starts, Lm, flags=L.MASK_AS_NAN)
        assert e.precision() == mode
        np.testing.assert_array_equal(e.read_packed().buf, want)
        assert z.shape == (5, 1500) and zs.shape == (B, Lm) and np.all(np.isfinite(score))
    finally:
        e.close()


# ---- class surface ------------------------------------------------------------------------------
def test_class_viterbi_on_the_two_blob_demo():
    from pysvihmm_amd import hmmbatchcd, hmmsgd_metaobs, util
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
    before = (svi.var_tran.copy(), svi.var_init.copy())
    z, score = svi.viterbi()
    assert z.shape == (N,) and z.dtype == np.int32 and np.isfinite(score)
    assert np.array_equal(svi.var_tran, before[0]) and np.array_equal(svi.var_init, before[1])
    ham = lambda path: float(np.mean(util.munkres_match(sts, path, K)[path] != sts))
    marg = np.argmax(svi.full_local_update(), axis=1)
    print("Hamming distance: MAP path %.4f, marginal decode %.4f" % (ham(z), ham(marg)))
    assert ham(z) <= ham(marg) + 0.01
    # one meta-observation: the MAP path of that window on its own
    zw, sw = svi.viterbi(MetaObs(290, 310))
    ll = svi.engine.loglik([290], 21, flags=L.MASK_AS_NAN)[0]
    mi, lt = svi.engine.read_globals()
    zr, sr = viterbi_numpy(ll, mi, lt)
    np.testing.assert_array_equal(zw, zr)
    assert sw == sr
    # inherited by the batch classes; an emission plugin without a device family goes through set_lliks
    class Plug(object):
        def __init__(self, g):
            self.g = g
        def expected_log_likelihood(self, x):
            return self.g.expected_log_likelihood(x)
        def get_vlb(self):
            return 0.0
    cd = hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), prior_emit, maxit=15)
    cd.infer()
    zc, sc = cd.viterbi()
    plug = hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), np.array([Plug(e) for e in cd.var_emit]), maxit=1)
    plug.var_tran, plug.var_init = cd.var_tran.copy(), cd.var_init.copy()
    zp, sp = plug.viterbi()
    np.testing.assert_array_equal(zp, zc)
    assert abs(sp - sc) <= 1e-9 * abs(sc)
    assert ham(zc) <= 0.01


# ---- errors -------------------------------------------------------------------------------------
def test_errors_leave_the_engine_usable():
    rng = np.random.default_rng(0)
    T, K, D = 300, 4, 3
    obs = rng.normal(size=(T, D))
    e = _fresh()
    try:
        def bad(msg, fn, *a, **k):                        # the whole message, as the C ABI words it
            e.profile_reset()
            with pytest.raises(RuntimeError, match="^" + re.escape("svihmm_viterbi failed: svihmm_viterbi: " + msg) + "$"):
                fn(*a, **k)
            assert not e.profile_read()                   # nothing was launched or copied
        host = "SVIHMM_USE_HOST_LLIKS without uploaded lliks of shape [B, Lm, K] (svihmm_set_lliks)"
        outside = "window %d reaches outside [0, T)"
        e.profile(True)
        bad("no globals: call svihmm_set_globals first", e.viterbi, [0], 5)
        mi, lt = np.log(rng.dirichlet(np.ones(K))), _tran(rng, K, "random")
        e.set_globals(mi, lt)
        bad("no observations: call svihmm_set_obs first", e.viterbi, [0], 5)
        bad(host, e.viterbi, [0], 5, flags=L.USE_HOST_LLIKS)    # no host lliks either
        e.set_obs(obs)
        bad("no emission family: call svihmm_set_emission_niw / _diag / _cat first", e.viterbi, [0], 5)
        A = rng.normal(size=(K, D, D))
        niw = (rng.normal(size=(K, D)), np.einsum('kij,klj->kil', A, A) + D * np.eye(D), np.ones(K), D + 2.0 + np.zeros(K))
        e.set_emission_niw(*niw)
        z, s = e.viterbi([0, 7], 5)
        bad("B and Lm must be positive", e.viterbi, [], 5)
        bad("B and Lm must be positive", e.viterbi, [0], 0)
        bad(outside % 0, e.viterbi, [T - 4], 5)           # window past the end
        bad(outside % 1, e.viterbi, [0, -1], 5)           # ... and before the start
        score = np.empty(1)
        bad("starts is NULL", lambda: L.check(                # (C ABI)
            e._lib.svihmm_viterbi(e._h, None, 1, 5, 0, None, L.dptr(score)), "svihmm_viterbi"))
        e.set_obs(rng.normal(size=(T, D + 1)))
        bad("emission D does not match obs D", e.viterbi, [0], 5)
        e.set_obs(obs)
        e.set_emission_niw(*niw)
        e.set_lliks(rng.normal(size=(2, 6, K)))
        bad(host, e.viterbi, [0, 0], 5, flags=L.USE_HOST_LLIKS)     # host lliks of another shape
        bad(host, e.viterbi, [0], 6, flags=L.USE_HOST_LLIKS)
        e.set_globals(np.log(rng.dirichlet(np.ones(K + 1))), _tran(rng, K + 1, "random"))
        bad("K of the globals (%d) differs from the emission family's K (%d)" % (K + 1, K), e.viterbi, [0], 5)
        Kw = 257
        e.set_globals(np.zeros(Kw), np.zeros((Kw, Kw)))
        e.set_lliks(np.zeros((1, 3, Kw)))
        bad("K = 257 > 256 not supported (one-byte back-pointers)", e.viterbi, [0], 3, flags=L.USE_HOST_LLIKS)
        bad("neither out_z nor out_score given", lambda: L.check(      # nothing to return (C ABI)
            e._lib.svihmm_viterbi(e._h, L.i64ptr(np.zeros(1, np.int64)), 1, 3, 0, None, None), "svihmm_viterbi"))
        # still usable
        e.profile(False)
        e.set_globals(mi, lt)
        z2, s2 = e.viterbi([0, 7], 5)
        np.testing.assert_array_equal(z2, z)
        np.testing.assert_array_equal(s2, s)
    finally:
        e.close()
