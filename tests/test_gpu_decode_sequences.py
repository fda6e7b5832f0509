"""svihmm_viterbi_sequences / svihmm_ffbs_sequences on the MI355X: all declared sequences decoded in one call.

Viterbi: given identical lliks, z and score EQUAL the NumPy recursion of tests/viterbi_helpers.py on each sequence's
rows, and the single-sequence call svihmm_viterbi on that sequence.  Lengths: psi stays in LDS up to 1008 rows
(K <= 64) / 240 rows (K > 64); longer sequences share one HBM run of padded chunks.
  (1, 1009, 2, 2017, 3, 63, 64, 65, 257, 1008, 1): one-row sequences at both ends, the wave width, the LDS limit and
  one above it, three chunks with a one-row tail, two long sequences separated by a short one (pad_off matters).
FFBS: every step of the device paths is recomputed from the call's own lalpha (tests/ffbs_helpers.check_paths), at
most ONE excused step per test -- after NumPy has shown that no step of the NumPy paths lies near a boundary."""
import functools
import re

import numpy as np
import pytest

from oracle import ref_c
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from sequences_helpers import LENGTHS, build_model, class_data, niw_problem, offsets
from tests.decode_sequences_helpers import (backward_sample_sequences, check_paths_sequences, near_boundary_sequences,
                                            philox_uniforms, viterbi_sequences_numpy)
from tests.ffbs_helpers import check_paths
from tests.test_gpu_viterbi import _chunk_map, _push, _synthetic_model, _tran
from tests.viterbi_helpers import path_score, viterbi_numpy

pytestmark = pytest.mark.gpu

HOST = L.USE_HOST_LLIKS
NARROW = (1, 1009, 2, 2017, 3, 63, 64, 65, 257, 1008, 1)
WIDE = (1, 241, 2, 481, 239, 240, 1)
D = 3


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _fresh():
    from pysvihmm_amd.engine import HipEngine
    return HipEngine(0)


def _declare(e, lengths):
    """Dummy observations, so that a declaration can exist (the lliks come from set_lliks)."""
    e.set_obs(np.zeros((int(sum(lengths)), 1)))
    e.set_sequences(lengths)


def _lengths(K):
    return NARROW if K <= 64 else WIDE


@functools.lru_cache(maxsize=None)
def _host_problem(K, kind, lengths, seed):
    """(ll [T, K], mod_init, ltran, z_ref [T], score_ref [N]) -- computed once, read-only."""
    rng = np.random.default_rng(seed)
    scale = {"random": 2.0, "flat": 0.05, "cycle": 0.01}[kind]
    T = int(sum(lengths))
    ll = rng.normal(size=(T, K)) * scale
    mod_init = np.log(rng.dirichlet(np.ones(K)))
    ltran = _tran(rng, K, kind)
    zr, sr = viterbi_sequences_numpy(ll, offsets(lengths), mod_init, ltran)
    for a in (ll, mod_init, ltran, zr, sr):
        a.setflags(write=False)
    return ll, mod_init, ltran, zr, sr


def _decode_host(e, ll, mod_init, ltran, lengths, declare=True):
    if declare:
        _declare(e, lengths)
    e.set_globals(mod_init, ltran)
    e.set_lliks(ll[None])
    z, score = e.viterbi_sequences(flags=HOST)
    assert z.dtype == np.int32 and z.shape == (ll.shape[0],) and score.shape == (len(lengths),)
    return z, score


# ---- Viterbi, exact, host-lliks route ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["random", "flat", "cycle"])
@pytest.mark.parametrize("K", [5, 16, 17, 64, 65, 130, 256])
def test_viterbi_exact_host_lliks(eng, K, kind):
    lengths = _lengths(K)
    off = offsets(lengths)
    ll, mod_init, ltran, zr, sr = _host_problem(K, kind, lengths, 7000 + K)
    if kind == "cycle" and K <= 64:
        # a whole interior chunk's map of the 2017-row sequence is not constant: composing the maps matters
        a = int(off[3])
        assert lengths[3] == 2017
        assert len(np.unique(_chunk_map(ll[a:a + 2017], mod_init, ltran, 1008, 2016))) > 1
    z, score = _decode_host(eng, ll, mod_init, ltran, lengths)
    np.testing.assert_array_equal(z, zr)
    np.testing.assert_array_equal(score, sr)                  # bit-equal
    # after the call the lliks of all T rows are the readable intermediate
    np.testing.assert_array_equal(eng.read_rows("lliks", 0, ll.shape[0]), ll)
    # ... and the single-sequence call on each sequence's slice, uploaded as its own [1, len, K] batch
    for s, ln in enumerate(lengths):
        a = int(off[s])
        eng.set_lliks(ll[None, a:a + ln])
        z1, s1 = eng.viterbi([a], ln, flags=HOST)
        np.testing.assert_array_equal(z[a:a + ln], z1[0])
        assert score[s] == s1[0]


@pytest.mark.parametrize("K,lengths", [(5, (1, 1009, 63, 2)), (64, (1009, 70)), (100, (1, 241, 30))])
def test_all_ties_give_the_zero_path(eng, K, lengths):
    T = sum(lengths)
    z, score = _decode_host(eng, np.zeros((T, K)), np.zeros(K), np.zeros((K, K)), lengths)
    assert not z.any() and not score.any()


@pytest.mark.parametrize("K,lengths", [(4, (60, 1, 1100)), (64, (70, 1010, 3)), (90, (300, 7, 240))])
def test_integer_inputs_with_many_ties(eng, K, lengths):
    rng = np.random.default_rng(K)
    T = sum(lengths)
    ll = rng.integers(-1, 2, size=(T, K)).astype(float)
    mi, lt = np.zeros(K), rng.integers(-1, 1, size=(K, K)).astype(float)
    z, score = _decode_host(eng, ll, mi, lt, lengths)
    zr, sr = viterbi_sequences_numpy(ll, offsets(lengths), mi, lt)
    np.testing.assert_array_equal(z, zr)
    np.testing.assert_array_equal(score, sr)


@pytest.mark.parametrize("K,lengths", [(6, (40, 1, 1100)), (64, (1100, 5)), (80, (30, 250, 1))])
def test_transition_range(eng, K, lengths):
    """ltran at -1000 and -inf (one finite entry kept per column), mod_init[0] = -inf: exact, finite scores."""
    rng = np.random.default_rng(K)
    ltran = _tran(rng, K, "random")
    ltran[rng.random((K, K)) < 0.3] = -1000.0
    ltran[rng.random((K, K)) < 0.3] = -np.inf
    ltran[rng.integers(0, K, size=K), np.arange(K)] = np.log(0.5)
    assert np.isneginf(ltran).any() and (ltran == -1000.0).any()
    ll = rng.normal(size=(sum(lengths), K))
    mod_init = np.log(rng.dirichlet(np.ones(K)))
    mod_init[0] = -np.inf
    z, score = _decode_host(eng, ll, mod_init, ltran, lengths)
    zr, sr = viterbi_sequences_numpy(ll, offsets(lengths), mod_init, ltran)
    np.testing.assert_array_equal(z, zr)
    np.testing.assert_array_equal(score, sr)
    assert np.all(np.isfinite(score))


@pytest.mark.parametrize("K,lengths,pick", [(5, (300, 7, 1500, 2017, 64), (0, 2)), (80, (100, 5, 300, 481), (0, 2))])
def test_viterbi_independent_of_the_other_sequences(eng, K, lengths, pick):
    """A sequence decoded inside the forward launch and one of the HBM run, each declared alone, in the full list and
    in the reversed list: the same bits for z and score."""
    off = offsets(lengths)
    ll, mod_init, ltran, zr, sr = _host_problem(K, "random", lengths, 55 + K)
    zf, sf = _decode_host(eng, ll, mod_init, ltran, lengths)
    blocks = [ll[off[s]:off[s + 1]] for s in range(len(lengths))]
    rl = lengths[::-1]
    roff = offsets(rl)
    zv, sv = _decode_host(eng, np.concatenate(blocks[::-1]), mod_init, ltran, rl)
    for s in pick:
        za, sa = _decode_host(eng, blocks[s], mod_init, ltran, (lengths[s],))
        r = len(lengths) - 1 - s
        for z, sc in ((zf[off[s]:off[s + 1]], sf[s]), (zv[roff[r]:roff[r + 1]], sv[r])):
            np.testing.assert_array_equal(z, za)
            assert sc == sa[0]
        np.testing.assert_array_equal(za, zr[off[s]:off[s + 1]])


# ---- Viterbi, device emission --------------------------------------------------------------------------
def _check_device_viterbi(e, ora, lengths, mod_init, ltran, flags, what):
    T, off = int(sum(lengths)), offsets(lengths)
    z, score = e.viterbi_sequences(flags=flags)
    ll = e.read_rows("lliks", 0, T)                          # the lliks the call itself evaluated
    zr, sr = viterbi_sequences_numpy(ll, off, mod_init, ltran)
    np.testing.assert_array_equal(z, zr)
    np.testing.assert_array_equal(score, sr)
    # optimality under the CPU oracle's lliks of each sequence ALONE (the bounds of tests/test_gpu_viterbi.py)
    for s, ln in enumerate(lengths):
        llo = ora.loglik([int(off[s])], ln, flags=flags)[0]
        _, opt = viterbi_numpy(llo, mod_init, ltran)
        got = path_score(z[off[s]:off[s + 1]], llo, mod_init, ltran)
        print("%s sequence %d (%d rows): oracle optimum %.12g, device path re-scored %.12g" % (what, s, ln, opt, got))
        assert got <= opt + 1e-9 * abs(opt)
        assert opt - got <= 1e-6 * abs(opt)
    # score-only and z-only calls
    z0, s0 = e.viterbi_sequences(flags=flags, want_z=False)
    assert z0 is None
    np.testing.assert_array_equal(s0, score)
    out = np.empty(T, dtype=np.int32)
    L.check(e._lib.svihmm_viterbi_sequences(e._h, int(flags), out.ctypes.data, None), "svihmm_viterbi_sequences")
    np.testing.assert_array_equal(out, z)
    return z, score


DEV_LENGTHS = (1, 1009, 2, 63, 257, 240, 1)


@pytest.mark.parametrize("K", [5, 64, 80])
def test_viterbi_niw_emission(eng, K):
    pb = niw_problem(K, D, DEV_LENGTHS, 400 + K)
    ora = OracleEngine()
    for e in (eng, ora):
        e.set_obs(pb["obs"], pb["mask"])
        e.set_globals(pb["mod_init"], pb["ltran"])
        e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    eng.set_sequences(DEV_LENGTHS)
    _check_device_viterbi(eng, ora, DEV_LENGTHS, pb["mod_init"], pb["ltran"], L.MASK_AS_NAN, "niw K=%d" % K)


@pytest.mark.parametrize("family", ["diag", "cat"])
def test_viterbi_diag_and_categorical_emission(eng, family):
    lengths = (1, 2, 63, 257, 376, 1)
    obs, mask, mod_init, ltran, em, _ = _synthetic_model(family)
    assert obs.shape[0] == sum(lengths)
    ora = OracleEngine()
    _push(eng, obs, mask, mod_init, ltran, em)
    _push(ora, obs, mask, mod_init, ltran, em)
    eng.set_sequences(lengths)
    _check_device_viterbi(eng, ora, lengths, mod_init, ltran, L.MASK_AS_NAN, family)


def test_packed_statistics_and_precision_survive():
    K, lengths = 16, (300, 1, 1100, 40)
    pb = niw_problem(K, D, lengths, 77)
    e = _fresh()
    try:
        e.set_obs(pb["obs"], pb["mask"])
        e.set_globals(pb["mod_init"], pb["ltran"])
        e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        e.set_sequences(lengths)
        e.estep_sequences(read=False)
        want = e.read_packed().buf.copy()
        mode = e.precision()
        z, score = e.viterbi_sequences(flags=L.MASK_AS_NAN)
        assert e.precision() == mode
        np.testing.assert_array_equal(e.read_packed().buf, want)
        with pytest.raises(RuntimeError, match="svihmm_viterbi_sequences keeps the lliks of all T rows only"):
            e.read_rows("var_x", 0, 5)
        logA = np.array(pb["ltran"])
        zf, _ = e.ffbs_sequences(logA, n_draws=2, seed=3, flags=L.MASK_AS_NAN)
        assert e.precision() == mode
        np.testing.assert_array_equal(e.read_packed().buf, want)
        for what in ("lalpha", "lbeta", "var_x"):
            with pytest.raises(RuntimeError, match="svihmm_ffbs_sequences keeps the lliks of all T rows only"):
                e.read_rows(what, 0, 5)
        assert e.read_rows("lliks", 0, sum(lengths)).shape == (sum(lengths), K)
        assert z.shape == (sum(lengths),) and zf.shape == (2, sum(lengths)) and np.all(np.isfinite(score))
    finally:
        e.close()


# ---- FFBS ------------------------------------------------------------------------------------------------
T_F = int(sum(LENGTHS))
OFF_F = offsets(LENGTHS)


def _logA(K, seed):
    return np.log(np.random.default_rng(seed).dirichlet(np.ones(K), size=K))


@functools.lru_cache(maxsize=None)
def _oracle_lalpha(K, sparse=False):
    """ref_c lliks -> forward of every sequence ALONE, concatenated (read-only)."""
    pb = niw_problem(K, D, LENGTHS, 900 + K, sparse=sparse)
    mi, lt = np.array(pb["mod_init"]), np.array(pb["ltran"])
    la = np.empty((T_F, K))
    for s in range(len(LENGTHS)):
        a, b = int(OFF_F[s]), int(OFF_F[s + 1])
        ll = ref_c.lliks_niw(np.array(pb["obs"][a:b]), pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        la[a:b] = ref_c.forward(ll, mi, lt)
    la.setflags(write=False)
    return la


def _load_ffbs(e, K, sparse=False):
    pb = niw_problem(K, D, LENGTHS, 900 + K, sparse=sparse)
    e.set_obs(pb["obs"], pb["mask"])
    e.set_globals(pb["mod_init"], pb["ltran"])
    e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    e.set_sequences(LENGTHS)
    return pb


def _ffbs_checked(e, K, S, sparse=False):
    la_ref = _oracle_lalpha(K, sparse)
    logA = _logA(K, K + S)
    u = np.random.default_rng(31 * K + S).random((S, T_F))
    # CPU first: no step of the NumPy paths lies near a CDF boundary, so an excused step would be a finding
    z_np = backward_sample_sequences(la_ref, logA, u, OFF_F)
    assert near_boundary_sequences(z_np, la_ref, logA, u, OFF_F) == 0
    _load_ffbs(e, K, sparse)
    z, la = e.ffbs_sequences(logA, n_draws=S, uniforms=u, want_lalpha=True)
    assert z.shape == (S, T_F) and z.dtype == np.int32 and la.shape == (T_F, K)
    excused = check_paths_sequences(z, la, logA, u, OFF_F)
    print("K=%d S=%d sparse=%s: %d steps, %d excused, %d differ from the NumPy paths on the oracle's lalpha"
          % (K, S, sparse, z.size, excused, int((z != z_np).sum())))
    assert excused <= 1
    for s in range(len(LENGTHS)):                            # lalpha of each sequence alone, the project's bound
        a, b = int(OFF_F[s]), int(OFF_F[s + 1])
        np.testing.assert_allclose(la[a:b], la_ref[a:b], rtol=1e-9, atol=1e-6)
    return z, la, logA, u


@pytest.mark.parametrize("S", [1, 3, 70])
@pytest.mark.parametrize("K", [5, 17, 64, 80])
def test_ffbs_paths_and_lalpha(eng, K, S):
    _ffbs_checked(eng, K, S)


def test_ffbs_sparse_globals(eng):
    _ffbs_checked(eng, 16, 3, sparse=True)


def test_ffbs_philox_equals_caller_uniforms(eng):
    K, S, seed = 5, 3, 0x1234567890ABCDEF
    logA = _logA(K, 1)
    _load_ffbs(eng, K)
    u = philox_uniforms(seed, S, T_F)
    zu, _ = eng.ffbs_sequences(logA, n_draws=S, uniforms=u)
    zp, _ = eng.ffbs_sequences(logA, n_draws=S, seed=seed)
    np.testing.assert_array_equal(zp, zu)


@pytest.mark.parametrize("K", [5, 80])
def test_ffbs_placement_independence(eng, K):
    S = 3
    z, la, logA, u = _ffbs_checked(eng, K, S)
    # a draw alone equals the same draw of the S-draw call
    z1, _ = eng.ffbs_sequences(logA, n_draws=1, uniforms=u[1:2])
    np.testing.assert_array_equal(z1[0], z[1])
    # a sequence declared alone: the same path, up to the excuse rule where the emission batch shape changed the
    # lliks' last bit (sequence 6: 257 rows, lanes; sequence 9: 2311 rows, whole-chain filter + composition)
    pb = niw_problem(K, D, LENGTHS, 900 + K)
    for s in (6, 9):
        sl = slice(int(OFF_F[s]), int(OFF_F[s + 1]))
        eng.set_obs(pb["obs"][sl], pb["mask"][sl])
        eng.set_sequences([LENGTHS[s]])
        za, laa = eng.ffbs_sequences(logA, n_draws=S, uniforms=u[:, sl], want_lalpha=True)
        n1 = check_paths(za, laa, logA, u[:, sl])
        n2 = check_paths(z[:, sl], laa, logA, u[:, sl])
        assert n1 + n2 <= 1
        if n1 + n2 == 0:
            np.testing.assert_array_equal(za, z[:, sl])


# ---- errors ------------------------------------------------------------------------------------------------
def test_errors_leave_the_engine_usable():
    rng = np.random.default_rng(0)
    K, lengths = 4, (20, 1, 300)
    T = sum(lengths)
    obs = rng.normal(size=(T, D))
    e = _fresh()
    try:
        def bad(fn_name, msg, fn, *a, **k):                  # the whole message, as the C ABI words it
            e.profile_reset()
            with pytest.raises(RuntimeError, match="^" + re.escape("%s failed: %s: %s" % (fn_name, fn_name, msg)) + "$"):
                fn(*a, **k)
            assert not e.profile_read()                      # nothing was launched or copied
        vit, ffb = "svihmm_viterbi_sequences", "svihmm_ffbs_sequences"
        host = "SVIHMM_USE_HOST_LLIKS without uploaded lliks of shape [1, T, K] (svihmm_set_lliks)"
        none = "no sequences declared: call svihmm_set_sequences first"
        mi, lt = np.log(rng.dirichlet(np.ones(K))), _tran(rng, K, "random")
        logA = lt.copy()
        out = np.empty((1, T), dtype=np.int32)

        def ffbs_c(flags=0):                                 # (C ABI: the wrapper sizes logA by the globals' K)
            L.check(e._lib.svihmm_ffbs_sequences(e._h, int(flags), L.dptr(logA), 1, None, 0, out.ctypes.data, None), ffb)
        both = [(vit, lambda **k: e.viterbi_sequences(**k)), (ffb, ffbs_c)]
        e.profile(True)
        for name, call in both:
            bad(name, none, call)
        e.set_obs(obs)
        for name, call in both:
            bad(name, none, call)
        e.set_sequences(lengths)
        for name, call in both:
            bad(name, "no globals: call svihmm_set_globals first", call)
        e.set_globals(mi, lt)
        for name, call in both:
            bad(name, "no emission family: call svihmm_set_emission_niw / _diag / _cat first", call)
            bad(name, host, call, flags=HOST)                # no host lliks either
        A = rng.normal(size=(K, D, D))
        niw = (rng.normal(size=(K, D)), np.einsum('kij,klj->kil', A, A) + D * np.eye(D), np.ones(K), D + 2.0 + np.zeros(K))
        e.set_emission_niw(*niw)
        z, s = e.viterbi_sequences()
        u = rng.random((2, T))
        zf, _ = e.ffbs_sequences(logA, n_draws=2, uniforms=u)
        e.set_lliks(rng.normal(size=(2, T // 2, K)))         # host lliks of another shape
        for name, call in both:
            bad(name, host, call, flags=HOST)
        e.set_lliks(rng.normal(size=(1, T - 1, K)))
        for name, call in both:
            bad(name, host, call, flags=HOST)
        # C ABI: nothing to return / nothing to draw with
        bad(vit, "neither out_z nor out_score given", lambda: L.check(
            e._lib.svihmm_viterbi_sequences(e._h, 0, None, None), vit))
        bad(vit, "NULL handle", lambda: L.check(e._lib.svihmm_viterbi_sequences(None, 0, None, L.dptr(np.empty(3))), vit))
        bad(ffb, "NULL handle", lambda: L.check(
            e._lib.svihmm_ffbs_sequences(None, 0, L.dptr(logA), 1, None, 0, out.ctypes.data, None), ffb))
        bad(ffb, "logA and out_z must be given", lambda: L.check(
            e._lib.svihmm_ffbs_sequences(e._h, 0, None, 1, None, 0, out.ctypes.data, None), ffb))
        bad(ffb, "logA and out_z must be given", lambda: L.check(
            e._lib.svihmm_ffbs_sequences(e._h, 0, L.dptr(logA), 1, None, 0, None, None), ffb))
        bad(ffb, "S must be positive", e.ffbs_sequences, logA, n_draws=0)
        la2 = logA.copy(); la2[1, 2] = np.nan
        bad(ffb, "logA[1][2] is NaN or +inf", e.ffbs_sequences, la2)
        la2 = logA.copy(); la2[0, 3] = np.inf
        bad(ffb, "logA[0][3] is NaN or +inf", e.ffbs_sequences, la2)
        la2 = logA.copy(); la2[:, 1] = -np.inf
        bad(ffb, "column 1 of logA has no finite entry", e.ffbs_sequences, la2)
        # model side
        e.set_globals(np.log(rng.dirichlet(np.ones(K + 1))), _tran(rng, K + 1, "random"))
        mism = "K of the globals (%d) differs from the emission family's K (%d)" % (K + 1, K)
        bad(vit, mism, e.viterbi_sequences)
        bad(ffb, mism, e.ffbs_sequences, np.zeros((K + 1, K + 1)))
        Kw = 257
        e.set_globals(np.zeros(Kw), np.zeros((Kw, Kw)))
        e.set_lliks(np.zeros((1, T, Kw)))
        bad(vit, "K = 257 > 256 not supported", e.viterbi_sequences, flags=HOST)
        bad(ffb, "K = 257 > 256 not supported", e.ffbs_sequences, np.zeros((Kw, Kw)), flags=HOST)
        # still usable
        e.profile(False)
        e.set_globals(mi, lt)
        z2, s2 = e.viterbi_sequences()
        np.testing.assert_array_equal(z2, z)
        np.testing.assert_array_equal(s2, s)
        zf2, _ = e.ffbs_sequences(logA, n_draws=2, uniforms=u)
        np.testing.assert_array_equal(zf2, zf)
    finally:
        e.close()


# ---- classes -------------------------------------------------------------------------------------------------
def test_classes_on_a_list():
    from pysvihmm_amd import hmmbatchcd
    lengths = (40, 1, 300, 17)
    off = offsets(lengths)
    T = sum(lengths)
    seqs, masks = class_data(lengths)
    e = _fresh()
    try:
        hmm = build_model(hmmbatchcd, seqs, masks, e, maxit=4)
        hmm.infer()
        zs, score = hmm.viterbi()
        assert [z.shape for z in zs] == [(n,) for n in lengths] and score.shape == (len(lengths),)
        for s, ln in enumerate(lengths):                     # (the engine still holds viterbi()'s globals and factors)
            z1, s1 = e.viterbi([int(off[s])], ln, flags=L.MASK_AS_NAN)
            np.testing.assert_array_equal(zs[s], z1[0])
            assert score[s] == s1[0]
        S = 3
        u = np.random.default_rng(2).random((S, T))
        fs = hmm.ffbs_windows(n_draws=S, uniforms=u)
        assert [f.shape for f in fs] == [(S, n) for n in lengths] and all(f.dtype == np.int32 for f in fs)
        logA = np.log(hmm.var_tran + np.finfo(np.float64).eps)
        zz, la = e.ffbs_sequences(logA, n_draws=S, uniforms=u, want_lalpha=True)
        np.testing.assert_array_equal(np.concatenate(fs, axis=1), zz)
        assert check_paths_sequences(zz, la, logA, u, off) <= 1

        # an emission plugin without a device family: the same paths through the host-lliks route
        class Plug(object):
            def __init__(self, g):
                self.g = g

            def expected_log_likelihood(self, x):
                return self.g.expected_log_likelihood(x)

            def get_vlb(self):
                return 0.0

        plug = hmmbatchcd.VBHMM(seqs, np.ones(4), np.ones((4, 4)), np.array([Plug(g) for g in hmm.var_emit]),
                                mask=masks, maxit=1, engine=e)
        plug.var_tran, plug.var_init = hmm.var_tran.copy(), hmm.var_init.copy()
        zp, sp = plug.viterbi()
        for a, b in zip(zs, zp):
            np.testing.assert_array_equal(a, b)
        np.testing.assert_allclose(sp, score, rtol=1e-9)
        fp = plug.ffbs_windows(n_draws=S, uniforms=u)
        n = check_paths_sequences(np.concatenate(fp, axis=1), la, logA, u, off)
        assert n <= 1
        if n == 0:
            for a, b in zip(fs, fp):
                np.testing.assert_array_equal(a, b)
    finally:
        e.close()
