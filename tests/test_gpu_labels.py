"""svihmm_set_labels: partially labelled rows on the device.

A labelled call is defined to give what the same call gives under ``USE_HOST_LLIKS`` on the clamped lliks, so the main
referee of every E-step here is that call on the same handle, fed with the lliks ``loglik`` hands out under the labels
(bit for bit where both sides ran the same sweep and statistics kernels, else at the tolerances of
tests/test_gpu_sequences.py), and next to it ``OracleEngine`` on the same lliks at that file's oracle tolerances.
The label generator (tests/labels_helpers.py) labels about 30 % of the rows with the argmax of the unlabelled llik row
(always a window's first and last row, one fully labelled window, one masked row, one row labelled K - 1): no label is
infeasible, since every transition expectation of the problems is finite."""
import ctypes

import numpy as np
import pytest

from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from tests import heldout_helpers as HH
from tests import mcat_helpers as MH
from tests import pgauss_helpers as GH
from tests import poisson_helpers as PH
from tests import svi_family_helpers as SH
from tests.helpers import make_problem
from tests.labels_helpers import clamp, make_labels, window_labels
from tests.test_gpu_family_switch import FAMILIES
from tests.test_gpu_sequences import RTOL, check_packed
from tests.viterbi_helpers import viterbi_batch, viterbi_numpy

pytestmark = pytest.mark.gpu

C = 15
WAVE, LOG_MFMA, SCALED = 1, 2, 3
SLOTS = ("forward_backward", "posterior", "stats")


# ---- problems: the builder of tests/test_gpu_family_switch.py at other shapes -------------------------------------
_problems = {}


def problem(K, D, T, seed=11, miss=0.1, ints=True):
    """One data set for every family (entries 0..3 are reals, symbols of a 4-symbol column and counts alike) with the
    parameters of all six families.  Computed once per shape and left unchanged."""
    key = (K, D, T, seed, ints)
    if key in _problems:
        return _problems[key]
    rng = np.random.default_rng(2024 + seed)
    p = make_problem(K, D, T, seed=seed)
    if ints:
        p["x"] = (p["sts"][:, None] % 4 + (rng.random((T, D)) < 0.3) * rng.integers(0, 4, size=(T, D))) % 4 + 0.0
    else:
        p["x"] = p["obs"]
    p["mask"] = rng.random(T) < miss
    if ints:
        p["mu"] = 1.5 + rng.normal(size=(K, D))
    p["diag"] = (p["mu"], 0.5 + 4 * rng.random((K, D)), 2.0 + 5 * rng.random((K, D)), 1.0 + 6 * rng.random((K, D)))
    p["VS"] = (4,) * D
    p["logp"] = MH.make_model(K, p["VS"], rng)[0]
    pois = PH.make_model(K, D, rng, base=np.full(D, 1.5))
    p["elog"], p["erate"] = pois["elog"], pois["erate"]
    al = rng.uniform(2.0, 20.0, size=(K, D))
    p["pg"] = GH.tables(p["mu"], rng.uniform(1.0, 50.0, size=(K, D)), al, al * rng.uniform(0.5, 2.0, size=(K, D)))
    p["origin"] = GH.data_origin(p["x"])
    _problems[key] = p
    return p


def enter(e, p, name):
    """Rows, globals and the family ``name`` on the handle (the upload removes whatever labels it held)."""
    e.set_obs(p["x"][:, :1] if name == "cat" else p["x"], p["mask"])
    e.set_globals(p["mod_init"], p["ltran"])
    if name == "niw":
        e.set_emission_niw(p["mu"], p["sigma"], p["kappa"], p["nu"])
    elif name == "diag":
        e.set_emission_diag(*p["diag"])
    elif name == "cat":
        e.set_emission_cat(np.ascontiguousarray(p["logp"][:, :4]))
    elif name == "mcat":
        e.set_emission_mcat(MH.split_tables(p["logp"], p["VS"]))
    elif name == "poisson":
        e.set_emission_poisson(p["elog"], p["erate"], C)
    else:
        e.set_emission_pgauss(*p["pg"], origin=p["origin"])


def labels_for(e, p, starts, Lm, seed=3, frac=0.3):
    """Labels over the T resident rows from the handle's own unlabelled lliks of the whole chain."""
    T = len(p["x"])
    ll = e.loglik([0], T, 0)[0]
    inside = np.zeros(T, bool)
    for s in starts:
        inside[int(s):int(s) + Lm] = True
    masked = np.flatnonzero(p["mask"] & inside)
    return make_labels(ll, ll.shape[1], np.random.default_rng(seed), frac=frac,
                       windows=[(int(s), Lm) for s in starts], full_window=(int(starts[len(starts) // 2]), Lm),
                       masked_row=int(masked[0]) if len(masked) else None)


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def kernels(e):
    return tuple(e.last_kernel(s) for s in SLOTS)


def check_one_hot(q, lab_rows):
    """var_x exactly 0.0 at forbidden pairs, within 1e-12 of 1 at the label."""
    q = q.reshape(-1, q.shape[-1])
    lab = np.asarray(lab_rows).ravel()
    rows = np.flatnonzero(lab >= 0)
    forb = np.ones((len(rows), q.shape[1]), bool)
    forb[np.arange(len(rows)), lab[rows]] = False
    assert np.all(q[rows][forb] == 0.0)
    assert np.max(np.abs(q[rows, lab[rows]] - 1.0)) <= 1e-12


def same_or_close(kd, kh, got, want, atol, rtol=RTOL, what=""):
    if kd == kh:
        assert np.array_equal(got, want), "%s: same kernels %s, max diff %g" % (what, kd, np.max(np.abs(got - want)))
    else:
        np.testing.assert_allclose(got, want, rtol=rtol, atol=atol, err_msg=what)


def estep_against_host_lliks(e, p, name, starts, Lm, lab, wrap, oracle=True):
    """The labelled call against the host-lliks call on the same handle and the oracle on the same lliks."""
    B, K = len(starts), p["K"]
    rows = B * Lm
    lw = window_labels(lab, starts, Lm)
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
    assert np.array_equal(np.isneginf(ll), (lw[..., None] >= 0) & (np.arange(K) != lw[..., None]))
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
    check_one_hot(q_d, lw)
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
    return kd, (None if st_d is None else st_d.buf.copy()), q_d


# ---- 1. the clamp is a select ----------------------------------------------------------------------------------------
K1, D1, T1, LM1 = 5, 3, 400, 37
STARTS1 = np.array([0, 50, 120, 363], dtype=np.int64)


@pytest.mark.parametrize("name", FAMILIES)
def test_clamp_is_a_select(eng, name):
    p = problem(K1, D1, T1)
    enter(eng, p, name)
    plain = {fl: eng.loglik(STARTS1, LM1, fl) for fl in (0, L.MASK_AS_NAN)}
    lab = labels_for(eng, p, STARTS1, LM1)
    assert np.any(lab == K1 - 1) and 0.2 < np.mean(lab >= 0) < 0.6
    eng.set_labels(lab)
    lw = window_labels(lab, STARTS1, LM1)
    for fl, ll in plain.items():
        np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, fl), clamp(ll, lw))
    # a masked labelled row: "state known, observation missing"
    t = int(np.flatnonzero(p["mask"] & (lab >= 0))[0])
    row = eng.loglik([t], 1, L.MASK_AS_NAN)[0, 0]
    assert row[lab[t]] == 0.0 and np.all(np.isneginf(np.delete(row, lab[t])))
    eng.set_labels(None)
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), plain[0])


# ---- 2. window E-steps against the host-lliks call on the same handle -----------------------------------------------
@pytest.mark.parametrize("wrap", [True, False], ids=["estep", "fb"])
@pytest.mark.parametrize("var", [WAVE, LOG_MFMA, SCALED], ids=["wave", "logmfma", "scaled"])
@pytest.mark.parametrize("name", ["niw", "diag", "poisson", "pgauss"])
def test_window_estep_small(eng, name, var, wrap):
    p = problem(K1, D1, T1)
    enter(eng, p, name)
    lab = labels_for(eng, p, STARTS1, LM1)
    eng.set_labels(lab)
    eng.set_variant("fb", var)
    try:
        estep_against_host_lliks(eng, p, name, STARTS1, LM1, lab, wrap)
    finally:
        eng.set_variant("fb", 0)


def test_window_estep_wide_two_pass(eng):
    K, D, Lm = 70, 4, 18
    p = problem(K, D, 300, seed=12, ints=False)
    starts = np.array([0, 100, 282], dtype=np.int64)
    enter(eng, p, "niw")
    lab = labels_for(eng, p, starts, Lm)
    assert np.any(lab == K - 1)
    eng.set_labels(lab)
    for wrap in (True, False):
        estep_against_host_lliks(eng, p, "niw", starts, Lm, lab, wrap)


def _fused(e, call):
    """Whether ``call`` ran the fused sweep + statistics launch: the slot's last kernel is k_sweep_stats and no
    statistics kernel of its own was launched (the slots' names outlive calls that do not set them, so the launch
    counts of the profiling hook decide)."""
    e.profile(True)
    e.profile_reset()
    try:
        res = call()
        counts = e.profile_read()
    finally:
        e.profile(False)
    return res, ("k_sweep_stats" in e.last_kernel("forward_backward") and "stats" not in counts)


def _before_during_after(e, p, starts, Lm, lab):
    """The E-step before labels were ever set, under labels (against the host-lliks call), and after their removal:
    (fused before, fused under labels, fused after)."""
    B = len(starts)
    fl = L.TRANS_WRAP | L.MASK_AS_NAN
    st, f0 = _fused(e, lambda: e.estep(starts, Lm, flags=fl))
    before = (st.buf.copy(), e.read_intermediate("var_x", B, Lm))
    e.set_labels(lab)
    _, buf, q = estep_against_host_lliks(e, p, "niw", starts, Lm, lab, True, oracle=False)
    st, f1 = _fused(e, lambda: e.estep(starts, Lm, flags=fl))
    assert np.array_equal(st.buf, buf) and np.array_equal(e.read_intermediate("var_x", B, Lm), q)
    e.set_labels(None)
    st, f2 = _fused(e, lambda: e.estep(starts, Lm, flags=fl))
    assert np.array_equal(st.buf, before[0]) and np.array_equal(e.read_intermediate("var_x", B, Lm), before[1])
    return f0, f1, f2


def test_labelled_batch_stays_off_the_fused_launch(eng):
    """K = 64, D = 32, 64 windows of 9 rows: the unlabelled batch takes the fused sweep + statistics launch, the
    labelled one does not, and after the labels' removal the batch takes it again with its earlier bits."""
    K, D, B, Lm = 64, 32, 64, 9
    p = problem(K, D, 1200, seed=13, ints=False)
    starts = (np.arange(B, dtype=np.int64) * 17) % (1200 - Lm)
    enter(eng, p, "niw")
    lab = labels_for(eng, p, starts, Lm)
    assert _before_during_after(eng, p, starts, Lm, lab) == (True, False, True)


def test_labelled_batch_above_the_wave_threshold(eng):
    """K = 64, D = 8, 4 CUs' worth of windows + 2, of 8 rows: the two-pass route of the large-batch sweeps (at 8208
    rows neither the fused launch, which ends at one window per CU, nor the step-major layout, which needs a 128-row
    emission workgroup per CU, takes the unlabelled batch either)."""
    K, D, Lm = 64, 8, 8
    B = 4 * 256 + 2
    p = problem(K, D, 3000, seed=14, ints=False)
    starts = (np.arange(B, dtype=np.int64) * 5) % (3000 - Lm)
    enter(eng, p, "niw")
    lab = labels_for(eng, p, starts, Lm, frac=0.1)
    assert _before_during_after(eng, p, starts, Lm, lab) == (False, False, False)


def test_labelled_batch_stays_off_the_step_major_layout(eng):
    """K = 64, D = 8, 1027 windows of 32 rows: the smallest kind of batch step_major_ok takes (4 CUs' worth of windows
    + 1 and a 128-row emission workgroup per CU).  The labelled batch is row-major (it equals the host-lliks call, which
    never is step-major); after the labels' removal the batch gives its earlier bits again."""
    K, D, Lm = 64, 8, 32
    B = 4 * 256 + 3
    p = problem(K, D, 6000, seed=15, ints=False)
    starts = (np.arange(B, dtype=np.int64) * 5) % (6000 - Lm)
    enter(eng, p, "niw")
    lab = labels_for(eng, p, starts, Lm, frac=0.1)
    assert _before_during_after(eng, p, starts, Lm, lab) == (False, False, False)


def test_fp32_mode_runs_a_labelled_batch_in_fp64(eng):
    K, D, Lm = 8, 3, 37
    p = problem(K, D, T1, seed=16, ints=False)
    enter(eng, p, "niw")
    lab = labels_for(eng, p, STARTS1, LM1)
    eng.set_precision("f32")
    eng.set_variant("fb", SCALED)
    try:
        eng.estep(STARTS1, Lm, flags=L.TRANS_WRAP)
        assert eng.precision() == ("f32", True)
        eng.set_labels(lab)
        estep_against_host_lliks(eng, p, "niw", STARTS1, Lm, lab, True)
        eng.estep(STARTS1, Lm, flags=L.TRANS_WRAP)
        assert eng.precision() == ("f32", False)          # the mode is left as set, the batch ran in fp64
        eng.set_labels(None)
        eng.estep(STARTS1, Lm, flags=L.TRANS_WRAP)
        assert eng.precision() == ("f32", True)
    finally:
        eng.set_variant("fb", 0)
        eng.set_precision("f64")


# ---- 3. the whole-chain scan ---------------------------------------------------------------------------------------
def test_chain(eng):
    K, D, T = 6, 3, 5000
    p = problem(K, D, T, seed=17, ints=False)
    enter(eng, p, "niw")
    best = np.argmax(eng.loglik([0], T, 0)[0], axis=1)            # 10 % of the rows, each with its best state
    keep = np.random.default_rng(2).random(T) < 0.1
    keep[[0, T - 1, int(np.flatnonzero(p["mask"])[0]), int(np.flatnonzero(best == K - 1)[0])]] = True
    lab = np.where(keep, best, -1).astype(np.int32)
    eng.set_labels(lab)
    estep_against_host_lliks(eng, p, "niw", np.array([0], dtype=np.int64), T, lab, False)


# ---- 4. several sequences -------------------------------------------------------------------------------------------
LENGTHS = (1, 2, 9, 40, 300, 2100)
OFF = np.concatenate(([0], np.cumsum(LENGTHS))).astype(np.int64)


def _sequence_case(e):
    K, D, T = 5, 3, int(OFF[-1])
    p = problem(K, D, T, seed=18, ints=False)
    enter(e, p, "niw")
    lab = labels_for(e, p, OFF[:-1], 1, frac=0.3)                 # (windows of one row: every sequence's first row)
    assert lab[0] >= 0 and all(lab[o] >= 0 for o in OFF[:-1])
    e.set_sequences(LENGTHS)
    e.set_labels(lab)
    return p, lab


def test_estep_sequences_and_subset(eng):
    p, lab = _sequence_case(eng)
    T = int(OFF[-1])
    _, seq_lb, _ = eng.estep_sequences(flags=L.MASK_AS_NAN, read=False)
    q = eng.read_intermediate("var_x", 1, T)[0]
    check_one_hot(q, lab)
    idx = [4, 1, 1, 5]
    _, sub_lb, _ = eng.estep_sequence_subset(idx, flags=L.MASK_AS_NAN, read=False)
    R = sum(LENGTHS[s] for s in idx)
    qs = eng.read_rows("var_x", 0, R)
    o = 0
    for m, s in enumerate(idx):                                   # the label gather: bit-identical to the full call
        assert np.array_equal(qs[o:o + LENGTHS[s]], q[OFF[s]:OFF[s + 1]]), s
        assert sub_lb[m] == seq_lb[s]
        o += LENGTHS[s]
    for s, ln in enumerate(LENGTHS):
        r = eng.forward_backward([OFF[s]], ln, flags=L.MASK_AS_NAN, want=("var_x", "local_lb"))
        np.testing.assert_allclose(q[OFF[s]:OFF[s + 1]], r["var_x"][0], rtol=1e-8, atol=1e-13)
        np.testing.assert_allclose(seq_lb[s], r["local_lb"][0], rtol=1e-12)


# ---- 5. decoders ----------------------------------------------------------------------------------------------------
def test_window_decoders(eng):
    p = problem(K1, D1, T1)
    enter(eng, p, "poisson")
    lab = labels_for(eng, p, STARTS1, LM1)
    eng.set_labels(lab)
    lw = window_labels(lab, STARTS1, LM1)
    B = len(STARTS1)
    z, score = eng.viterbi(STARTS1, LM1, flags=L.MASK_AS_NAN)
    ll = eng.read_intermediate("lliks", B, LM1)
    np.testing.assert_array_equal(ll, eng.loglik(STARTS1, LM1, L.MASK_AS_NAN))
    zr, sr = viterbi_batch(ll, p["mod_init"], p["ltran"])
    assert np.array_equal(z, zr) and np.array_equal(score, sr)
    assert np.array_equal(z[lw >= 0], lw[lw >= 0])
    u = np.random.default_rng(8).random((3, B, LM1))
    zf, _ = eng.ffbs_windows(STARTS1, LM1, p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN)
    for d in range(3):
        assert np.array_equal(zf[d][lw >= 0], lw[lw >= 0])
    eng.set_lliks(ll)
    zh, _ = eng.ffbs_windows(STARTS1, LM1, p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN | L.USE_HOST_LLIKS)
    assert np.array_equal(zf, zh)
    for d in range(3):                                            # the whole chain, one draw per call
        zc, _ = eng.ffbs(p["ltran"], np.random.default_rng(20 + d).random(T1), flags=L.MASK_AS_NAN, want_lalpha=False)
        assert np.array_equal(zc[lab >= 0], lab[lab >= 0])


def test_sequence_decoders(eng):
    p, lab = _sequence_case(eng)
    T = int(OFF[-1])
    z, score = eng.viterbi_sequences(flags=L.MASK_AS_NAN)
    ll = eng.read_rows("lliks", 0, T)
    assert np.array_equal(np.isneginf(ll), (lab[:, None] >= 0) & (np.arange(p["K"]) != lab[:, None]))
    for s in range(len(LENGTHS)):
        zr, sr = viterbi_numpy(ll[OFF[s]:OFF[s + 1]], p["mod_init"], p["ltran"])
        assert np.array_equal(z[OFF[s]:OFF[s + 1]], zr) and score[s] == sr
    assert np.array_equal(z[lab >= 0], lab[lab >= 0])
    u = np.random.default_rng(9).random((3, T))
    zf, _ = eng.ffbs_sequences(p["ltran"], n_draws=3, uniforms=u, flags=L.MASK_AS_NAN)
    for d in range(3):
        assert np.array_equal(zf[d][lab >= 0], lab[lab >= 0])


# ---- 6. held-out rows ------------------------------------------------------------------------------------------------
def test_heldout_rows_score_the_unclamped_llik(eng):
    p = problem(K1, D1, T1)
    enter(eng, p, "pgauss")
    ll_true = eng.loglik(STARTS1, LM1, 0).reshape(-1, K1)
    lab = labels_for(eng, p, STARTS1, LM1)
    eng.set_labels(lab)
    eng.estep(STARTS1, LM1, flags=L.TRANS_WRAP | L.MASK_AS_NAN)
    n = len(STARTS1) * LM1
    mean, cnt, lp = eng.heldout_rows(want_lp=True)
    q = eng.read_rows("var_x", 0, n)
    masked = p["mask"][HH.window_rows(STARTS1, LM1)]
    want = HH.heldout_rows_numpy(q, ll_true, masked)
    assert cnt == int(masked.sum()) > 0
    np.testing.assert_allclose(lp[masked], want[masked], rtol=1e-9)
    assert np.all(np.isnan(lp[~masked]))
    np.testing.assert_allclose(mean, HH.mean_count(want)[0], rtol=1e-9)


# ---- 7. lifecycle and refusals -------------------------------------------------------------------------------------
def test_lifecycle(eng):
    p = problem(K1, D1, T1)
    enter(eng, p, "diag")
    plain = eng.loglik(STARTS1, LM1, 0)
    lab = labels_for(eng, p, STARTS1, LM1)
    lw = window_labels(lab, STARTS1, LM1)
    eng.set_labels(lab)
    # svihmm_set_obs_rows keeps the labels
    blk = np.ascontiguousarray(p["x"][:50])
    L.check(eng._lib.svihmm_set_obs_rows(eng._h, 0, 50, L.dptr(blk), None), "svihmm_set_obs_rows")
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), clamp(plain, lw))
    # a refused call leaves the earlier set in force
    bad = lab.copy()
    bad[3] = -5
    with pytest.raises(RuntimeError, match=r"svihmm_set_labels: labels\[3\] = -5"):
        eng.set_labels(bad)
    with pytest.raises(RuntimeError, match="shape"):
        eng.set_labels(lab[:-1])
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), clamp(plain, lw))
    # a label at or above K is refused at the call, with the row
    big = lab.copy()
    big[11] = 7
    eng.set_labels(big)
    for call in (lambda: eng.estep(STARTS1, LM1), lambda: eng.loglik(STARTS1, LM1, 0),
                 lambda: eng.viterbi(STARTS1, LM1)):
        with pytest.raises(RuntimeError, match="row 11 is labelled with state 7, the globals have K = 5"):
            call()
    # svihmm_set_obs removes them
    eng.set_obs(p["x"], p["mask"])
    np.testing.assert_array_equal(eng.loglik(STARTS1, LM1, 0), plain)
    # no observations: refused
    from pysvihmm_amd.engine import HipEngine
    e2 = HipEngine(0)
    try:
        rc = e2._lib.svihmm_set_labels(e2._h, lab.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert rc != 0 and "svihmm_set_labels: no observations" in L.last_error()
    finally:
        e2.close()


def test_refusals_leave_the_resident_loop_intact():
    from pysvihmm_amd.engine import HipEngine
    K = 3
    c = SH.family_case("poisson", K, 2, 0.3, "counts")
    starts = np.array([0, 20, 40])
    T = len(c["obs"])
    lab = np.full(T, -1, dtype=np.int32)
    lab[::7] = 1
    out = []
    for disturbed in (False, True):
        e = HipEngine(0)
        try:
            e.set_variant("centring", 1)
            e.set_obs(c["obs"], None)
            e.svi_begin_poisson(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], SH.POIS_C, 8)
            e.svi_iteration(0, starts, 3, 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)
            if disturbed:
                e.set_labels(lab)
                for fn, call in (
                        ("svihmm_svi_iteration", lambda: e.svi_iteration(1, starts, 3, 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)),
                        ("svihmm_svi_iteration_sequences", lambda: e.svi_iteration_sequences(1, [0], 0, 0.5, 1.0)),
                        ("svihmm_grow_windows", lambda: e.grow_windows([100], 5)),
                        ("svihmm_pred_logprob", lambda: e.pred_logprob(starts, 17))):
                    with pytest.raises(RuntimeError, match=fn + ": .*svihmm_set_labels"):
                        call()
                e.set_labels(None)
            e.svi_iteration(1, starts + 3, 3, 17, L.TRANS_WRAP, 0.4, 3.0, 3.0)
            vt, vi, fac = e.svi_read_factors()
            out.append((vt, vi) + tuple(fac) + (e.svi_read_elbo(2)[0],))
            assert e.svi_recoveries() == 0
        finally:
            e.close()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---- 8. the classes --------------------------------------------------------------------------------------------------
def _class_labels(sts, K, T, rng):
    lab = np.where(rng.random(T) < 0.2, sts % K, -1).astype(np.int32)
    lab[0] = sts[0] % K
    return lab


def _poisson_emitters(K, D):
    from pysvihmm_amd.distributions import ProductPoisson
    rng = np.random.default_rng(9)
    return np.array([ProductPoisson(np.ones(D), np.full(D, 0.2), alpha_mf=rng.uniform(1.0, 40.0, size=D) * 2.0,
                                    beta_mf=np.full(D, 2.0), max_count=255) for _ in range(K)])


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
    lab = _class_labels(sts, K, T, rng)
    obs = [a.copy() for a in cut(x, lengths)] if multi else x
    msk = [a.copy() for a in cut(pb["mask"], lengths)] if multi else pb["mask"]
    labs = [a.copy() for a in cut(lab, lengths)] if multi else lab

    def make(engine):
        if fam == "niw":
            return build_model(hmmbatchcd, obs, msk, engine, K=K, maxit=3)
        np.random.seed(3)
        return hmmbatchcd.VBHMM(obs, np.ones(K), np.ones((K, K)), _poisson_emitters(K, 3), mask=msk, maxit=3,
                                engine=engine)
    hmm = make(None)
    hmm.set_labels(labs)
    assert hmm.engine.name == "hip" and hmm._device_family()
    hmm.infer()
    ref = make(OracleEngine())
    ref.set_labels(labs)
    assert not ref._device_family()
    if fam == "niw":
        ref.infer()
    elif not multi:
        ref.infer(fused=False)           # (the plugin's literal host path: the oracle engine packs NIW statistics only)
    else:
        ref = None                       # (several sequences have no literal host path)
    try:
        assert len(hmm.elbo_vec) == 3 and np.all(np.isfinite(hmm.elbo_vec))
        rows = np.flatnonzero(lab >= 0)
        check_one_hot(hmm.var_x, lab)
        if ref is not None:
            np.testing.assert_allclose(hmm.var_tran, ref.var_tran, rtol=1e-6, atol=1e-9)
            np.testing.assert_allclose(hmm.elbo_vec, ref.elbo_vec, rtol=1e-8)
            np.testing.assert_allclose(hmm.var_x, ref.var_x, rtol=1e-6, atol=1e-11)
            np.testing.assert_allclose(hmm.lalpha, ref.lalpha, rtol=1e-9, atol=1e-8)
            np.testing.assert_allclose(hmm.var_init, ref.var_init, rtol=1e-6, atol=1e-9)
        z = hmm.viterbi()[0]
        z = np.concatenate(z) if multi else z
        assert np.array_equal(z[rows], lab[rows])
    finally:
        hmm.engine.close()


def test_batchsgd_sequence_minibatches_take_the_host_route():
    from pysvihmm_amd import hmmbatchsgd
    from tests.sequences_helpers import build_model, cut
    K, T = 4, 600
    lengths = (200, 1, 340, 59)
    pb = make_problem(K, 2, T, seed=31, miss=0.1)
    lab = _class_labels(pb["sts"], K, T, np.random.default_rng(22))
    m = build_model(hmmbatchsgd, cut(pb["obs"], lengths), cut(pb["mask"], lengths), None, K=K, maxit=3, seq_minibatch=3)
    try:
        m.set_labels(cut(lab, lengths))
        assert "labels" in m._svi_sequences_refusal()
        with pytest.raises(RuntimeError, match=r"infer\(device_loop=True\): labels are set"):
            m.infer(device_loop=True)
        m.infer()
        assert len(m.elbo_vec) == 3 and np.all(np.isfinite(m.elbo_vec))
    finally:
        m.engine.close()
