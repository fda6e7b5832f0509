"""svihmm_set_state_sets: allowed-state sets per row on the device.

The contract is the labels' (tests/test_gpu_labels.py): a call under sets gives what the same call gives under
``USE_HOST_LLIKS`` on the clamped lliks, so the main referee of every E-step here is that call on the same handle, fed
with the lliks ``loglik`` hands out under the sets (bit for bit where both sides ran the same sweep and statistics
kernels, else at the tolerances of tests/test_gpu_sequences.py and the label tests' atols), and next to it
``OracleEngine`` on the same lliks.  The set generator (tests/state_sets_helpers.py) constrains about 30 % of the rows
to the argmax of the unclamped llik row plus 0-3 other states and adds the edge rows it documents; no set is infeasible,
since every transition expectation of the problems is finite."""
import ctypes

import numpy as np
import pytest

from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from pysvihmm_amd.util import pack_state_sets
from tests import heldout_helpers as HH
from tests import svi_family_helpers as SH
from tests.helpers import make_problem
from tests.labels_helpers import clamp, window_labels
from tests.state_sets_helpers import check_cases, clamp_sets, make_sets, singleton_labels, window_sets
from tests.test_gpu_family_switch import FAMILIES
from tests.test_gpu_labels import (LOG_MFMA, SCALED, WAVE, _fused, _poisson_emitters, enter, kernels, problem,
                                   same_or_close)
from tests.test_gpu_sequences import RTOL, check_packed
from tests.viterbi_helpers import viterbi_batch, viterbi_numpy

pytestmark = pytest.mark.gpu


def sets_for(e, p, starts, Lm, seed=3, frac=0.3, inside_windows=True, full=True):
    """Sets over the T resident rows from the handle's own unclamped lliks of the whole chain; the generator's edge
    rows lie inside the windows.  ``full``: the middle window is constrained in every row."""
    T = len(p["x"])
    ll = e.loglik([0], T, 0)[0]
    K = ll.shape[1]
    inside = np.zeros(T, bool)
    for s in starts:
        inside[int(s):int(s) + Lm] = True
    masked = np.flatnonzero(p["mask"] & inside)
    kw = dict(windows=[(int(s), Lm) for s in starts],
              full_window=(int(starts[len(starts) // 2]), Lm) if full else None,
              masked_row=int(masked[0]) if len(masked) else None, inside=inside if inside_windows else None)
    a = make_sets(ll, K, np.random.default_rng(seed), frac=frac, **kw)
    if frac >= 0.3:
        check_cases(a, K, **kw)
    return a


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def check_constrained(q, allowed_rows):
    """var_x exactly 0.0 at forbidden pairs; the allowed entries of every row sum to 1 within 1e-12."""
    q = q.reshape(-1, q.shape[-1])
    a = np.asarray(allowed_rows).reshape(q.shape)
    assert np.all(q[~a] == 0.0)
    assert np.max(np.abs(np.where(a, q, 0.0).sum(axis=1) - 1.0)) <= 1e-12


def estep_against_host_lliks(e, p, name, starts, Lm, allowed, wrap, oracle=True):
    """The call under sets against the host-lliks call on the same handle and the oracle on the same lliks."""
    B, K = len(starts), p["K"]
    rows = B * Lm
    aw = window_sets(allowed, starts, Lm)
    fl = L.MASK_AS_NAN | (L.TRANS_WRAP if wrap else 0)
    if wrap:
        st_d = e.estep(starts, Lm, flags=fl)
        q_d = e.read_intermediate("var_x", B, Lm)
        lb_d = np.array([st_d.lb[0]])
    else:
        r = e.forward_backward(starts, Lm, flags=fl, want=("var_x", "local_lb"))
        st_d, q_d, lb_d = None, r["var_x"], r["local_lb"]
    kd = kernels(e)
    assert e.precision()[1] is False
    ll = e.loglik(starts, Lm, L.MASK_AS_NAN)
    assert np.array_equal(np.isneginf(ll), ~aw)
    e.set_lliks(ll)
    if wrap:
        st_h = e.estep(starts, Lm, flags=fl | L.USE_HOST_LLIKS)
        q_h = e.read_intermediate("var_x", B, Lm)
        lb_h = np.array([st_h.lb[0]])
    else:
        r = e.forward_backward(starts, Lm, flags=fl | L.USE_HOST_LLIKS, want=("var_x", "local_lb"))
        st_h, q_h, lb_h = None, r["var_x"], r["local_lb"]
    kh = kernels(e)
    same_or_close(kd, kh, q_d, q_h, 1e-12, what="var_x")
    same_or_close(kd, kh, lb_d, lb_h, 0.0, rtol=1e-10, what="lb")
    if wrap:
        same_or_close(kd, kh, st_d.buf, st_h.buf, 1e-7 * rows, what="packed")
    check_constrained(q_d, aw)
    if oracle:
        o = OracleEngine()
        o.set_obs(p["x"][:, :1] if name == "cat" else p["x"], p["mask"])
        o.set_globals(p["mod_init"], p["ltran"])
        o.set_lliks(ll)
        if wrap and name == "niw":
            ref = o.estep(starts, Lm, flags=fl | L.USE_HOST_LLIKS)
            check_packed(st_d, ref.buf, K, p["x"].shape[1], rows)
            q_o, lb_o = o.read_intermediate("var_x", B, Lm), np.array([ref.lb[0]])
        else:
            r = o.forward_backward(None, Lm, flags=L.USE_HOST_LLIKS, want=("var_x", "local_lb"), B=B)
            q_o, lb_o = r["var_x"], (np.array([r["local_lb"].sum()]) if wrap else r["local_lb"])
        np.testing.assert_allclose(q_d, q_o, rtol=RTOL, atol=1e-12)
        np.testing.assert_allclose(lb_d, lb_o, rtol=1e-10)
    return kd, (None if st_d is None else st_d.buf.copy()), q_d, lb_d


# ---- 1. the clamp is a select ----------------------------------------------------------------------------------------
K1, D1, T1, LM1 = 5, 3, 400, 37
STARTS1 = np.array([0, 50, 120, 363], dtype=np.int64)


def _select_check(e, p, starts, Lm, K):
    plain = {fl: e.loglik(starts, Lm, fl) for fl in (0, L.MASK_AS_NAN)}
    a = sets_for(e, p, starts, Lm)
    e.set_state_sets(a)
    aw = window_sets(a, starts, Lm)
    for fl, ll in plain.items():
        got = e.loglik(starts, Lm, fl)
        assert np.array_equal(np.isneginf(got), ~aw)              # -inf exactly at the forbidden pairs
        np.testing.assert_array_equal(got, clamp_sets(ll, aw))     # the bits of the unclamped call elsewhere
    # a masked constrained row: "state in this set, observation missing"
    t = int(np.flatnonzero(p["mask"] & (a.sum(axis=1) < K))[0])
    row = e.loglik([t], 1, L.MASK_AS_NAN)[0, 0]
    assert np.all(row[a[t]] == 0.0) and np.all(np.isneginf(row[~a[t]]))
    e.set_state_sets(pack_state_sets(a), K=K)                      # the packed form gives the same
    np.testing.assert_array_equal(e.loglik(starts, Lm, 0), clamp_sets(plain[0], aw))
    e.set_state_sets(None)
    np.testing.assert_array_equal(e.loglik(starts, Lm, 0), plain[0])


@pytest.mark.parametrize("name", FAMILIES)
def test_clamp_is_a_select(eng, name):
    p = problem(K1, D1, T1)
    enter(eng, p, name)
    _select_check(eng, p, STARTS1, LM1, K1)


# ---- 2. word boundaries: bit 63, a second word of one state, four words ----------------------------------------------
STARTS2 = np.array([0, 50, 163], dtype=np.int64)


@pytest.mark.parametrize("name", ["mcat", "niw"])
@pytest.mark.parametrize("K", [64, 65, 256])
def test_word_boundaries(eng, K, name):
    p = problem(K, D1, 200, seed=19)
    enter(eng, p, name)
    _select_check(eng, p, STARTS2, LM1, K)


# ---- 3. window E-steps against the host-lliks call on the same handle -----------------------------------------------
@pytest.mark.parametrize("wrap", [True, False], ids=["estep", "fb"])
@pytest.mark.parametrize("var", [WAVE, LOG_MFMA, SCALED], ids=["wave", "logmfma", "scaled"])
@pytest.mark.parametrize("name", ["niw", "diag", "poisson", "pgauss"])
def test_window_estep_small(eng, name, var, wrap):
    p = problem(K1, D1, T1)
    enter(eng, p, name)
    a = sets_for(eng, p, STARTS1, LM1)
    eng.set_state_sets(a)
    eng.set_variant("fb", var)
    try:
        estep_against_host_lliks(eng, p, name, STARTS1, LM1, a, wrap)
    finally:
        eng.set_variant("fb", 0)


def test_window_estep_wide_two_pass(eng):
    K, D, Lm = 65, 4, 18
    p = problem(K, D, 300, seed=12, ints=False)
    starts = np.array([0, 100, 282], dtype=np.int64)
    enter(eng, p, "niw")
    a = sets_for(eng, p, starts, Lm)
    assert np.any(~a[:, :64].any(axis=1))                          # a row that lives in the second word alone
    eng.set_state_sets(a)
    for wrap in (True, False):
        estep_against_host_lliks(eng, p, "niw", starts, Lm, a, wrap)


# ---- 4. singleton sets are labels, all-ones sets are no labels ------------------------------------------------------
def _estep_record(e, starts, Lm):
    fl = L.TRANS_WRAP | L.MASK_AS_NAN
    st = e.estep(starts, Lm, flags=fl)
    return (st.buf.copy(), e.read_intermediate("var_x", len(starts), Lm), float(st.lb[0]), kernels(e),
            e.loglik(starts, Lm, L.MASK_AS_NAN))


@pytest.mark.parametrize("name", ["niw", "mcat"])
def test_singleton_sets_equal_labels(eng, name):
    p = problem(K1, D1, T1)
    enter(eng, p, name)
    a = sets_for(eng, p, STARTS1, LM1)
    ll = eng.loglik([0], T1, 0)[0]
    lab = np.where(a.sum(axis=1) < K1, np.argmax(np.where(a, ll, -np.inf), axis=1), -1).astype(np.int32)
    single = np.ones((T1, K1), bool)
    rows = np.flatnonzero(lab >= 0)
    single[rows] = False
    single[rows, lab[rows]] = True
    assert np.array_equal(singleton_labels(single), lab)
    for sets, labels in ((single, lab), (np.ones((T1, K1), bool), np.full(T1, -1, dtype=np.int32))):
        eng.set_state_sets(sets)
        under_sets = _estep_record(eng, STARTS1, LM1)
        eng.set_labels(labels)
        under_labels = _estep_record(eng, STARTS1, LM1)
        for got, want in zip(under_sets, under_labels):
            assert np.array_equal(got, want)
    eng.set_labels(None)


# ---- 5. routing ------------------------------------------------------------------------------------------------------
def _before_during_after(e, p, starts, Lm, a):
    """The E-step before sets were ever set, under sets (against the host-lliks call), and after their removal:
    (fused before, fused under sets, fused after)."""
    B = len(starts)
    fl = L.TRANS_WRAP | L.MASK_AS_NAN
    st, f0 = _fused(e, lambda: e.estep(starts, Lm, flags=fl))
    before = (st.buf.copy(), e.read_intermediate("var_x", B, Lm))
    e.set_state_sets(a)
    _, buf, q, _ = estep_against_host_lliks(e, p, "niw", starts, Lm, a, True, oracle=False)
    st, f1 = _fused(e, lambda: e.estep(starts, Lm, flags=fl))
    assert np.array_equal(st.buf, buf) and np.array_equal(e.read_intermediate("var_x", B, Lm), q)
    e.set_state_sets(None)
    st, f2 = _fused(e, lambda: e.estep(starts, Lm, flags=fl))
    assert np.array_equal(st.buf, before[0]) and np.array_equal(e.read_intermediate("var_x", B, Lm), before[1])
    return f0, f1, f2


def test_constrained_batch_stays_off_the_fused_launch(eng):
    """K = 64, D = 32, 64 windows of 9 rows: the free batch takes the fused sweep + statistics launch, the one under
    sets does not, and after the sets' removal the batch takes it again with its earlier bits."""
    K, D, B, Lm = 64, 32, 64, 9
    p = problem(K, D, 1200, seed=13, ints=False)
    starts = (np.arange(B, dtype=np.int64) * 17) % (1200 - Lm)
    enter(eng, p, "niw")
    a = sets_for(eng, p, starts, Lm)
    assert _before_during_after(eng, p, starts, Lm, a) == (True, False, True)


def test_constrained_batch_above_the_wave_threshold(eng):
    """The label test's shape: K = 64, D = 8, 4 CUs' worth of windows + 2, of 8 rows -- the two-pass route of the
    large-batch sweeps."""
    K, D, Lm = 64, 8, 8
    B = 4 * 256 + 2
    p = problem(K, D, 3000, seed=14, ints=False)
    starts = (np.arange(B, dtype=np.int64) * 5) % (3000 - Lm)
    enter(eng, p, "niw")
    a = sets_for(eng, p, starts, Lm, frac=0.1)
    assert _before_during_after(eng, p, starts, Lm, a) == (False, False, False)


def test_constrained_batch_stays_off_the_step_major_layout(eng):
    """K = 64, D = 8, 1027 windows of 32 rows: the smallest kind of batch step_major_ok takes.  The batch under sets is
    row-major (it equals the host-lliks call, which never is step-major); after the sets' removal the batch gives its
    earlier bits again."""
    K, D, Lm = 64, 8, 32
    B = 4 * 256 + 3
    p = problem(K, D, 6000, seed=15, ints=False)
    starts = (np.arange(B, dtype=np.int64) * 5) % (6000 - Lm)
    enter(eng, p, "niw")
    a = sets_for(eng, p, starts, Lm, frac=0.1)
    assert _before_during_after(eng, p, starts, Lm, a) == (False, False, False)


def test_fp32_mode_runs_a_constrained_batch_in_fp64(eng):
    K, D, Lm = 8, 3, 37
    p = problem(K, D, T1, seed=16, ints=False)
    enter(eng, p, "niw")
    a = sets_for(eng, p, STARTS1, LM1)
    eng.set_precision("f32")
    eng.set_variant("fb", SCALED)
    try:
        eng.estep(STARTS1, Lm, flags=L.TRANS_WRAP)
        assert eng.precision() == ("f32", True)
        eng.set_state_sets(a)
        estep_against_host_lliks(eng, p, "niw", STARTS1, Lm, a, True)
        eng.estep(STARTS1, Lm, flags=L.TRANS_WRAP)
        assert eng.precision() == ("f32", False)          # the mode is left as set, the batch ran in fp64
        eng.set_state_sets(None)
        eng.estep(STARTS1, Lm, flags=L.TRANS_WRAP)
        assert eng.precision() == ("f32", True)
    finally:
        eng.set_variant("fb", 0)
        eng.set_precision("f64")


# ---- 6. the whole-chain scan and several sequences -------------------------------------------------------------------
def test_chain(eng):
    K, D, T = 6, 3, 5000
    p = problem(K, D, T, seed=17, ints=False)
    enter(eng, p, "niw")
    a = sets_for(eng, p, np.array([0], dtype=np.int64), T, frac=0.1, full=False)
    a[[0, T - 1]] = [[True, False, True, True, False, False], [False, True, True, False, False, True]]
    eng.set_state_sets(a)
    estep_against_host_lliks(eng, p, "niw", np.array([0], dtype=np.int64), T, a, False)


LENGTHS = (1, 2, 9, 40, 300, 2100)
OFF = np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)


def _sequence_case(e):
    K, D, T = 5, 3, int(OFF[-1])
    p = problem(K, D, T, seed=18, ints=False)
    enter(e, p, "niw")
    a = sets_for(e, p, OFF[:-1], 1, frac=0.3, inside_windows=False)   # (windows of one row: every sequence's first row)
    assert all(a[o].sum() < K for o in OFF[:-1])
    e.set_sequences(LENGTHS)
    e.set_state_sets(a)
    return p, a


def test_estep_sequences_and_subset(eng):
    p, a = _sequence_case(eng)
    T = int(OFF[-1])
    _, seq_lb, _ = eng.estep_sequences(flags=L.MASK_AS_NAN, read=False)
    q = eng.read_intermediate("var_x", 1, T)[0]
    check_constrained(q, a)
    idx = [4, 1, 1, 5]                                            # twice, and not ascending: the gather
    _, sub_lb, _ = eng.estep_sequence_subset(idx, flags=L.MASK_AS_NAN, read=False)
    R = sum(LENGTHS[s] for s in idx)
    qs = eng.read_rows("var_x", 0, R)
    o = 0
    for m, s in enumerate(idx):                                   # bit-identical to the full call
        assert np.array_equal(qs[o:o + LENGTHS[s]], q[OFF[s]:OFF[s + 1]]), s
        assert sub_lb[m] == seq_lb[s]
        o += LENGTHS[s]
    for s, ln in enumerate(LENGTHS):                              # per sequence: the host-lliks call
        ll = eng.loglik([OFF[s]], ln, L.MASK_AS_NAN)
        assert np.array_equal(np.isneginf(ll[0]), ~a[OFF[s]:OFF[s + 1]])
        eng.set_lliks(ll)
        r = eng.forward_backward([OFF[s]], ln, flags=L.MASK_AS_NAN | L.USE_HOST_LLIKS, want=("var_x", "local_lb"))
        np.testing.assert_allclose(q[OFF[s]:OFF[s + 1]], r["var_x"][0], rtol=1e-8, atol=1e-13)
        np.testing.assert_allclose(seq_lb[s], r["local_lb"][0], rtol=1e-12)


# ---- 7. decoders -----------------------------------------------------------------------------------------------------
def _in_sets(z, allowed_rows):
    return np.all(np.take_along_axis(allowed_rows, np.asarray(z)[..., None].astype(np.int64), axis=-1))


def test_window_decoders(eng):
    p = problem(K1, D1, T1)
    enter(eng, p, "poisson")
    a = sets_for(eng, p, STARTS1, LM1)
    eng.set_state_sets(a)
    aw = window_sets(a, STARTS1, LM1)
    B = len(STARTS1)
    z, score = eng.viterbi(STARTS1, LM1, flags=L.MASK_AS_NAN)
    ll = eng.read_intermediate("lliks", B, LM1)
    np.testing.assert_array_equal(ll, eng.loglik(STARTS1, LM1, L.MASK_AS_NAN))
    assert np.array_equal(np.isneginf(ll), ~aw)
    zr, sr = viterbi_batch(ll, p["mod_init"], p["ltran"])
    assert np.array_equal(z, zr) and np.array_equal(score, sr)
    assert _in_sets(z, aw)
    u = np.random.default_rng(8).random((3, B, LM1))
    zf, _ = eng.ffbs_windows(STARTS1, LM1, p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN)
    for d in range(3):
        assert _in_sets(zf[d], aw)
    eng.set_lliks(ll)
    zh, _ = eng.ffbs_windows(STARTS1, LM1, p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN | L.USE_HOST_LLIKS)
    assert np.array_equal(zf, zh)
    for d in range(3):                                            # the whole chain, one draw per call
        zc, _ = eng.ffbs(p["ltran"], np.random.default_rng(20 + d).random(T1), flags=L.MASK_AS_NAN, want_lalpha=False)
        assert _in_sets(zc, a)


def test_sequence_decoders(eng):
    p, a = _sequence_case(eng)
    T = int(OFF[-1])
    z, score = eng.viterbi_sequences(flags=L.MASK_AS_NAN)
    ll = eng.read_rows("lliks", 0, T)
    assert np.array_equal(np.isneginf(ll), ~a)
    for s in range(len(LENGTHS)):
        zr, sr = viterbi_numpy(ll[OFF[s]:OFF[s + 1]], p["mod_init"], p["ltran"])
        assert np.array_equal(z[OFF[s]:OFF[s + 1]], zr) and score[s] == sr
    assert _in_sets(z, a)
    u = np.random.default_rng(9).random((3, T))
    zf, _ = eng.ffbs_sequences(p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN)
    for d in range(3):
        assert _in_sets(zf[d], a)
    eng.set_lliks(ll[None])                                       # the host-lliks calls on those lliks [1, T, K]
    zh, _ = eng.ffbs_sequences(p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN | L.USE_HOST_LLIKS)
    assert np.array_equal(zf, zh)
    zv, sv = eng.viterbi_sequences(flags=L.MASK_AS_NAN | L.USE_HOST_LLIKS)
    assert np.array_equal(z, zv) and np.array_equal(score, sv)


# ---- 8. held-out rows ------------------------------------------------------------------------------------------------
def test_heldout_rows_score_the_unclamped_llik(eng):
    p = problem(K1, D1, T1)
    enter(eng, p, "pgauss")
    ll_true = eng.loglik(STARTS1, LM1, 0).reshape(-1, K1)
    a = sets_for(eng, p, STARTS1, LM1)
    eng.set_state_sets(a)
    eng.estep(STARTS1, LM1, flags=L.TRANS_WRAP | L.MASK_AS_NAN)
    n = len(STARTS1) * LM1
    mean, cnt, lp = eng.heldout_rows(want_lp=True)
    q = eng.read_rows("var_x", 0, n)
    check_constrained(q, window_sets(a, STARTS1, LM1))
    masked = p["mask"][HH.window_rows(STARTS1, LM1)]
    want = HH.heldout_rows_numpy(q, ll_true, masked)
    assert cnt == int(masked.sum()) > 0
    np.testing.assert_allclose(lp[masked], want[masked], rtol=1e-9)
    assert np.all(np.isnan(lp[~masked]))
    np.testing.assert_allclose(mean, HH.mean_count(want)[0], rtol=1e-9)


# ---- 9. lifecycle and refusals ---------------------------------------------------------------------------------------
def test_lifecycle(eng):
    p = problem(K1, D1, T1)
    enter(eng, p, "diag")
    plain = eng.loglik(STARTS1, LM1, 0)
    a = sets_for(eng, p, STARTS1, LM1)
    aw = window_sets(a, STARTS1, LM1)
    want = clamp_sets(plain, aw)
    eng.set_state_sets(a)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    # svihmm_set_obs_rows and svihmm_set_sequences keep the sets
    blk = np.ascontiguousarray(p["x"][:50])
    L.check(eng._lib.svihmm_set_obs_rows(eng._h, 0, 50, L.dptr(blk), None), "svihmm_set_obs_rows")
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    eng.set_sequences([T1])
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    eng.set_sequences(None)
    # refused at the call, with the row; the earlier sets stay in force
    bad = a.copy()
    bad[3] = False
    bad[9] = False
    with pytest.raises(RuntimeError, match="svihmm_set_state_sets: row 3 allows no state"):
        eng.set_state_sets(bad)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    packed = pack_state_sets(a)
    pad = packed.copy()
    pad[4, 0] |= np.uint64(1) << np.uint64(K1)
    pad[8, 0] |= np.uint64(1) << np.uint64(63)
    with pytest.raises(RuntimeError, match="svihmm_set_state_sets: row 4 has bit 5 set, at or beyond K = 5"):
        eng.set_state_sets(pad, K=K1)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    ptr = packed.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    for k in (0, 257, -1):
        assert eng._lib.svihmm_set_state_sets(eng._h, ptr, k) != 0
        assert "svihmm_set_state_sets: K = %d is outside [1, 256]" % k in L.last_error()
    with pytest.raises(RuntimeError, match="rows"):
        eng.set_state_sets(a[:-1])
    with pytest.raises(RuntimeError, match="K="):
        eng.set_state_sets(packed)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    # sets replace labels, labels replace sets, NULL removes only its own kind
    lab = np.full(T1, -1, dtype=np.int32)
    lab[STARTS1[1] + 2] = 1
    lw = window_labels(lab, STARTS1, LM1)
    eng.set_labels(lab)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), clamp(plain, lw))
    eng.set_state_sets(None)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), clamp(plain, lw))
    eng.set_state_sets(a)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    eng.set_labels(None)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), want)
    eng.set_labels(lab)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), clamp(plain, lw))
    eng.set_labels(None)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), plain)
    eng.set_state_sets(a)
    eng.set_state_sets(None)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), plain)
    # sets for another K are refused at the E-step-type call; the message names both
    eng.set_state_sets(np.ones((T1, K1 + 1), bool))
    for call in (lambda: eng.estep(STARTS1, LM1), lambda: eng.loglik(STARTS1, LM1, 0),
                 lambda: eng.viterbi(STARTS1, LM1)):
        with pytest.raises(RuntimeError, match="the sets were given for K = 6 states, the globals have K = 5"):
            call()
    # svihmm_set_obs removes them
    eng.set_state_sets(a)
    eng.set_obs(p["x"], p["mask"])
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), plain)
    # no observations: refused
    from pysvihmm_amd.engine import HipEngine
    e2 = HipEngine(0)
    try:
        assert e2._lib.svihmm_set_state_sets(e2._h, ptr, K1) != 0
        assert "svihmm_set_state_sets: no observations" in L.last_error()
    finally:
        e2.close()


def test_refusals_leave_the_resident_loop_intact():
    from pysvihmm_amd.engine import HipEngine
    K = 3
    c = SH.family_case("poisson", K, 2, 0.3, "counts")
    starts = np.array([0, 20, 40])
    T = len(c["obs"])
    a = np.ones((T, K), bool)
    a[::7, 0] = False
    out = []
    for disturbed in (False, True):
        e = HipEngine(0)
        try:
            e.set_variant("centring", 1)
            e.set_obs(c["obs"], None)
            e.svi_begin_poisson(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], SH.POIS_C, 8)
            e.svi_iteration(0, starts, 3, 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)
            if disturbed:
                e.set_state_sets(a)
                for fn, call in (
                        ("svihmm_svi_iteration", lambda: e.svi_iteration(1, starts, 3, 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)),
                        ("svihmm_svi_iteration_sequences", lambda: e.svi_iteration_sequences(1, [0], 0, 0.5, 1.0)),
                        ("svihmm_grow_windows", lambda: e.grow_windows([100], 5)),
                        ("svihmm_pred_logprob", lambda: e.pred_logprob(starts, 17))):
                    with pytest.raises(RuntimeError, match=fn + ": .*svihmm_set_state_sets"):
                        call()
                e.set_state_sets(None)
            e.svi_iteration(1, starts + 3, 3, 17, L.TRANS_WRAP, 0.4, 3.0, 3.0)
            vt, vi, fac = e.svi_read_factors()
            out.append((vt, vi) + tuple(fac) + (e.svi_read_elbo(2)[0],))
            assert e.svi_recoveries() == 0
        finally:
            e.close()
    for x, y in zip(*out):
        assert np.array_equal(x, y)


# ---- 10. the classes -------------------------------------------------------------------------------------------------
def _class_sets(sts, K, T, rng):
    """20 % of the rows (and row 0): the generating state plus one other."""
    a = np.ones((T, K), bool)
    rows = np.flatnonzero(rng.random(T) < 0.2)
    rows = np.union1d(rows, [0])
    a[rows] = False
    a[rows, sts[rows] % K] = True
    a[rows, (sts[rows] + 1 + rng.integers(0, K - 1, size=len(rows))) % K] = True
    a[rows[1]] = False
    a[rows[1], sts[rows[1]] % K] = True                            # one singleton
    return a


@pytest.mark.parametrize("fam", ["niw", "poisson"])
@pytest.mark.parametrize("multi", [False, True], ids=["array", "list"])
def test_batchcd_against_the_oracle_engine(fam, multi):
    from pysvihmm_amd import hmmbatchcd
    from tests.sequences_helpers import build_model, cut
    K, T = 4, 600
    lengths = (200, 1, 340, 59)
    rng = np.random.default_rng(21)
    pb = make_problem(K, 2, T, seed=31, miss=0.1)
    sts = pb["sts"]
    if fam == "niw":
        x = pb["obs"]
    else:
        lam = np.array([[1.0, 9.0, 30.0], [6.0, 1.5, 12.0], [15.0, 20.0, 2.0], [3.0, 40.0, 60.0]])
        x = rng.poisson(lam[sts % K]).astype(float)
    a = _class_sets(sts, K, T, rng)
    obs = [v.copy() for v in cut(x, lengths)] if multi else x
    msk = [v.copy() for v in cut(pb["mask"], lengths)] if multi else pb["mask"]
    sets = [v.copy() for v in cut(a, lengths)] if multi else a

    def make(engine):
        if fam == "niw":
            return build_model(hmmbatchcd, obs, msk, engine, K=K, maxit=3)
        np.random.seed(3)
        return hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), _poisson_emitters(K, 3), mask=msk, maxit=3,
                                engine=engine)
    hmm = make(None)
    hmm.set_state_sets(sets)
    assert hmm.engine.name == "hip" and hmm._device_family()
    hmm.infer()
    ref = make(OracleEngine())
    ref.set_state_sets(sets)
    assert not ref._device_family()
    if fam == "niw":
        ref.infer()
    elif not multi:
        ref.infer(fused=False)           # (the plugin's literal host path: the oracle engine packs NIW statistics only)
    else:
        ref = None                       # (several sequences have no literal host path)
    try:
        assert len(hmm.elbo_vec) == 3 and np.all(np.isfinite(hmm.elbo_vec))
        check_constrained(hmm.var_x, a)
        if ref is not None:
            np.testing.assert_allclose(hmm.var_tran, ref.var_tran, rtol=1e-6, atol=1e-9)
            np.testing.assert_allclose(hmm.elbo_vec, ref.elbo_vec, rtol=1e-8)
            np.testing.assert_allclose(hmm.var_x, ref.var_x, rtol=1e-6, atol=1e-11)
            np.testing.assert_allclose(hmm.lalpha, ref.lalpha, rtol=1e-9, atol=1e-8)
            np.testing.assert_allclose(hmm.var_init, ref.var_init, rtol=1e-6, atol=1e-9)
        z = hmm.viterbi()[0]
        z = np.concatenate(z) if multi else z
        assert _in_sets(z, a)
    finally:
        hmm.engine.close()


def test_batchsgd_sequence_minibatches_take_the_host_route():
    from pysvihmm_amd import hmmbatchsgd
    from tests.sequences_helpers import build_model, cut
    K, T = 4, 600
    lengths = (200, 1, 340, 59)
    pb = make_problem(K, 2, T, seed=31, miss=0.1)
    a = _class_sets(pb["sts"], K, T, np.random.default_rng(22))
    oracle_elbo = None
    for engine in (None, OracleEngine()):
        m = build_model(hmmbatchsgd, cut(pb["obs"], lengths), cut(pb["mask"], lengths), engine, K=K, maxit=3,
                        seq_minibatch=3)
        try:
            m.set_state_sets(cut(a, lengths))
            assert "set_state_sets" in m._svi_sequences_refusal()
            with pytest.raises(RuntimeError, match=r"infer\(device_loop=True\): allowed-state sets are set"):
                m.infer(device_loop=True)
            m.infer()
            assert len(m.elbo_vec) == 3 and np.all(np.isfinite(m.elbo_vec))
            if engine is None:
                assert m.engine.name == "hip"
                hip = (m.var_tran.copy(), m.var_init.copy(), np.array(m.elbo_vec))
            else:
                oracle_elbo = (m.var_tran.copy(), m.var_init.copy(), np.array(m.elbo_vec))
        finally:
            if engine is None:
                m.engine.close()
    np.testing.assert_allclose(hip[0], oracle_elbo[0], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(hip[1], oracle_elbo[1], rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(hip[2], oracle_elbo[2], rtol=1e-8)
