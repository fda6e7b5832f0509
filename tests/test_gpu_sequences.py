"""svihmm_set_sequences / svihmm_estep_sequences: the E-step of several sequences of unequal length in one
device call, against the per-sequence sums of the oracle (tests/sequences_helpers.py).  Tolerances: those
tests/test_gpu_chain.py holds the whole-chain scan to.

Lengths (1, 2, 3, 63, 64, 65, 257, 2047, 2048, 2311, 1), 6862 rows: both ends a one-row sequence, one sequence
either side of the wave width, one just below the chain threshold, one chain-routed with a tail chunk."""
import numpy as np
import pytest

from helpers import make_problem, unpack
from sequences_helpers import (LENGTHS, MASK_AS_NAN, TRANS_WRAP, build_model, class_data, niw_packed,
                               niw_posteriors, niw_problem, offsets, oracle_engine_sum)

pytestmark = pytest.mark.gpu
RTOL = 1e-6
D = 3
T = int(sum(LENGTHS))
OFF = offsets(LENGTHS)
KS = [5, 16, 64, 80, 256]
FLAGS = [0, MASK_AS_NAN, TRANS_WRAP]


def seed_of(K):
    return 900 + K


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def load_niw(eng, K, lengths=LENGTHS, sparse=False, declare=True):
    pb = niw_problem(K, D, lengths, seed_of(K), sparse=sparse)
    eng.set_obs(pb["obs"], pb["mask"])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    if declare:
        eng.set_sequences(lengths)
    return pb


def check_packed(st, ref_buf, K, Dd, rows, kind="niw"):
    np.testing.assert_allclose(st.A_raw, ref_buf[:K * K].reshape(K, K), rtol=RTOL, atol=1e-9 * rows)
    if kind == "cat":
        np.testing.assert_allclose(st.counts.ravel(), ref_buf[K * K:-1], rtol=RTOL, atol=1e-9 * rows)
    elif kind == "diag":
        o = K * K
        np.testing.assert_allclose(st.xbar.ravel(), ref_buf[o:o + K * Dd], rtol=RTOL, atol=1e-8 * rows)
        np.testing.assert_allclose(st.neff, ref_buf[o + K * Dd:o + K * Dd + K], rtol=RTOL, atol=1e-9 * rows)
        np.testing.assert_allclose(st.xsq.ravel(), ref_buf[o + K * Dd + K:-1], rtol=RTOL, atol=1e-7 * rows)
    else:
        A, xbar, neff, S, lb = unpack(ref_buf, K, Dd)
        np.testing.assert_allclose(st.neff, neff, rtol=RTOL, atol=1e-9 * rows)
        np.testing.assert_allclose(st.xbar, xbar, rtol=RTOL, atol=1e-8 * rows)
        np.testing.assert_allclose(st.S, S, rtol=RTOL, atol=1e-7 * rows)
    np.testing.assert_allclose(st.lb[0], ref_buf[-1], rtol=1e-10)


# ---- 1, 1a, 1b: NIW against the per-sequence oracle sum ---------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("K", KS)
def test_niw_packed_q0_and_rows_vs_oracle(eng, K, flags):
    load_niw(eng, K)
    ref_buf, ref_lb = niw_packed(K, D, LENGTHS, seed_of(K), flags)
    ref_q, ref_lb2, ref_q0 = niw_posteriors(K, D, LENGTHS, seed_of(K), bool(flags & MASK_AS_NAN))
    st, seq_lb, q0 = eng.estep_sequences(flags=flags)
    check_packed(st, ref_buf, K, D, T)                                          # 1
    assert seq_lb.shape == (len(LENGTHS),)
    np.testing.assert_allclose(seq_lb, ref_lb, rtol=1e-10)
    np.testing.assert_allclose(q0, ref_q0, rtol=RTOL, atol=1e-12)               # 1a
    q = eng.read_rows("var_x", 0, T)                                            # 1b
    np.testing.assert_allclose(q, ref_q, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(q.sum(-1), 1.0, rtol=1e-11)


# ---- 2: against the device's own per-sequence forward_backward on the same handle ---------------
@pytest.mark.parametrize("K", [5, 64, 80, 256])
def test_rows_and_lb_vs_device_forward_backward(eng, K):
    load_niw(eng, K)
    _, seq_lb, _ = eng.estep_sequences(flags=MASK_AS_NAN, read=False)
    q = eng.read_intermediate("var_x", 1, T)[0]
    for s, ln in enumerate(LENGTHS):
        r = eng.forward_backward([OFF[s]], ln, flags=MASK_AS_NAN, want=("var_x", "local_lb"))
        np.testing.assert_allclose(q[OFF[s]:OFF[s + 1]], r["var_x"][0], rtol=1e-8, atol=1e-13)
        np.testing.assert_allclose(seq_lb[s], r["local_lb"][0], rtol=1e-12)


# ---- 3, 3a: independence of the other sequences, reproducibility --------------------------------
def test_a_sequence_does_not_depend_on_the_others():
    """The 257-row (ragged sweeps) and the 2311-row (whole-chain scan) sequence declared alone, in the full list
    and in the reversed list: their posterior rows and local_lb are the same bits.  The handle's automatic
    centring is off (its shift is the mean of a sample of ALL resident rows, so three different uploads would
    hold three different roundings of the same observations)."""
    from pysvihmm_amd.engine import HipEngine
    K = 16
    pb = niw_problem(K, D, LENGTHS, seed_of(K))
    e = HipEngine(0)
    try:
        e.set_variant("centring", 1)
        e.set_globals(pb["mod_init"], pb["ltran"])
        e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        got = {}
        for s in (6, 9):
            sl = slice(OFF[s], OFF[s + 1])
            runs = []
            # (a) alone
            e.set_obs(pb["obs"][sl], pb["mask"][sl])
            e.set_sequences([LENGTHS[s]])
            _, lb, _ = e.estep_sequences(flags=MASK_AS_NAN, read=False)
            runs.append((e.read_rows("var_x", 0, LENGTHS[s]), lb[0]))
            # (b) the full list, (c) the reversed list
            for order in (list(range(len(LENGTHS))), list(range(len(LENGTHS)))[::-1]):
                rows = np.concatenate([np.arange(OFF[i], OFF[i + 1]) for i in order])
                lens = [LENGTHS[i] for i in order]
                e.set_obs(pb["obs"][rows], pb["mask"][rows])
                e.set_sequences(lens)
                _, lb, _ = e.estep_sequences(flags=MASK_AS_NAN, read=False)
                pos = order.index(s)
                runs.append((e.read_rows("var_x", int(offsets(lens)[pos]), LENGTHS[s]), lb[pos]))
            got[s] = runs
        for s, runs in got.items():
            for q, lb in runs[1:]:
                assert np.array_equal(q, runs[0][0]), "rows of sequence %d" % s
                assert lb == runs[0][1], "local_lb of sequence %d" % s
    finally:
        e.close()


@pytest.mark.parametrize("K", [16, 80])
def test_two_identical_calls_are_bit_identical(eng, K):
    load_niw(eng, K)
    a = eng.estep_sequences(flags=TRANS_WRAP)
    qa = eng.read_rows("var_x", 0, T)
    b = eng.estep_sequences(flags=TRANS_WRAP)
    qb = eng.read_rows("var_x", 0, T)
    assert np.array_equal(a[0].buf, b[0].buf)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(qa, qb)


# ---- 4: diagonal and Categorical families -------------------------------------------------------
LEN4 = (1, 64, 65, 2100)


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("family", ["diag", "cat"])
def test_diag_and_categorical_vs_oracle_engine(eng, family, flags):
    from oracle.engine import OracleEngine
    rows = int(sum(LEN4))
    rng = np.random.default_rng(5)
    oe = OracleEngine()
    if family == "diag":
        K, Dd = 6, 4
        pb = make_problem(K, Dd, rows, seed=77, miss=0.1)
        fam = (pb["mu"], 0.5 + rng.random((K, Dd)), 2.0 + rng.random((K, Dd)), 1.0 + rng.random((K, Dd)))
        obs = pb["obs"]
    else:
        K, V, Dd = 3, 5, 1
        pb = make_problem(K, 1, rows, seed=78, miss=0.1)
        obs = rng.integers(0, V, size=(rows, 1)).astype(np.float64)
        logp = np.log(rng.dirichlet(np.ones(V), size=K))
    for e in (oe, eng):
        e.set_obs(obs, pb["mask"])
        e.set_globals(pb["mod_init"], pb["ltran"])
        if family == "diag":
            e.set_emission_diag(*fam)
        else:
            e.set_emission_cat(logp)
    eng.set_sequences(LEN4)
    ref_buf, ref_lb, ref_q, ref_q0 = oracle_engine_sum(oe, LEN4, flags)
    st, seq_lb, q0 = eng.estep_sequences(flags=flags)
    check_packed(st, ref_buf, K, Dd, rows, kind=family)
    np.testing.assert_allclose(seq_lb, ref_lb, rtol=1e-10)
    np.testing.assert_allclose(q0, ref_q0, rtol=RTOL, atol=1e-12)
    q = eng.read_rows("var_x", 0, rows)
    np.testing.assert_allclose(q, ref_q, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(q.sum(-1), 1.0, rtol=1e-11)


# ---- 5: sparse globals (the literal logaddexp form) ----------------------------------------------
LEN5 = (1, 65, 2100)


@pytest.mark.parametrize("flags", FLAGS)
def test_sparse_globals_vs_oracle(eng, flags):
    K = 6
    rows = int(sum(LEN5))
    pb = load_niw(eng, K, LEN5, sparse=True)
    assert pb["ltran"].min() < -600.0
    ref_buf, ref_lb = niw_packed(K, D, LEN5, seed_of(K), flags, sparse=True)
    ref_q, _, ref_q0 = niw_posteriors(K, D, LEN5, seed_of(K), bool(flags & MASK_AS_NAN), sparse=True)
    st, seq_lb, q0 = eng.estep_sequences(flags=flags)
    check_packed(st, ref_buf, K, D, rows)
    np.testing.assert_allclose(seq_lb, ref_lb, rtol=1e-10)
    np.testing.assert_allclose(q0, ref_q0, rtol=RTOL, atol=1e-12)
    q = eng.read_rows("var_x", 0, rows)
    np.testing.assert_allclose(q, ref_q, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(q.sum(-1), 1.0, rtol=1e-11)


# ---- 6: boundary check of the window entry points --------------------------------------------------
def test_windows_must_stay_inside_one_sequence(eng):
    from pysvihmm_amd import _lib as L
    K = 5
    pb = load_niw(eng, K)
    rng = np.random.default_rng(3)
    inside, Lin = [200], 100            # rows 200 .. 299 of sequence 6 (rows 198 .. 454)
    across, Lac = [60], 20              # rows 60 .. 79: sequence 3 ends at row 68
    vx = rng.dirichlet(np.ones(K), size=(1, Lin))
    vx2 = rng.dirichlet(np.ones(K), size=(1, Lac))
    calls = {
        "estep": lambda s, n, v: eng.estep(s, n, flags=L.TRANS_WRAP).buf,
        "forward_backward": lambda s, n, v: eng.forward_backward(s, n)["var_x"],
        "viterbi": lambda s, n, v: np.concatenate([a.ravel().astype(float) for a in eng.viterbi(s, n)]),
        "suffstats": lambda s, n, v: eng.suffstats(s, n, v, flags=0).buf,
    }
    with_decl = {}
    for name, f in calls.items():
        with pytest.raises(RuntimeError, match="window 0 .*two sequences"):
            f(across, Lac, vx2)
        with_decl[name] = f(inside, Lin, vx)
    # two windows, the second one straddles: the message names it
    with pytest.raises(RuntimeError, match="window 1 "):
        eng.estep([200, 4540], 20)
    eng.set_sequences(None)
    for name, f in calls.items():
        assert np.array_equal(f(inside, Lin, vx), with_decl[name]), name
        f(across, Lac, vx2)                                   # no declaration: nothing is rejected
    # set_obs removes a declaration
    eng.set_sequences(LENGTHS)
    eng.set_obs(pb["obs"], pb["mask"])
    eng.estep(across, Lac)
    with pytest.raises(RuntimeError, match="no sequences declared"):
        eng.estep_sequences()


# ---- 7: errors leave the handle usable --------------------------------------------------------------
def _case1(eng):
    K = 5
    load_niw(eng, K)
    ref_buf, ref_lb = niw_packed(K, D, LENGTHS, seed_of(K), 0)
    st, seq_lb, _ = eng.estep_sequences(flags=0)
    check_packed(st, ref_buf, K, D, T)
    np.testing.assert_allclose(seq_lb, ref_lb, rtol=1e-10)


@pytest.mark.parametrize("what", ["first_offset", "repeated_offset", "last_offset", "no_declaration",
                                  "host_lliks", "K300"])
def test_errors_leave_the_handle_usable(eng, what):
    from pysvihmm_amd import _lib as L
    load_niw(eng, 5, declare=False)
    off = OFF.copy()
    if what == "first_offset":
        off[0] = 1
        with pytest.raises(RuntimeError, match=r"seq_off\[0\]"):
            eng.set_sequence_offsets(off)
    elif what == "repeated_offset":
        off[4] = off[3]
        with pytest.raises(RuntimeError, match="strictly increasing"):
            eng.set_sequence_offsets(off)
    elif what == "last_offset":
        off[-1] = T + 1
        with pytest.raises(RuntimeError, match="must equal T"):
            eng.set_sequence_offsets(off)
    elif what == "no_declaration":
        with pytest.raises(RuntimeError, match="no sequences declared"):
            eng.estep_sequences()
    elif what == "host_lliks":
        eng.set_sequences(LENGTHS)
        with pytest.raises(RuntimeError, match="HOST_LLIKS"):
            eng.estep_sequences(flags=L.USE_HOST_LLIKS)
    else:
        pb = make_problem(300, D, T, seed=3)
        eng.set_globals(pb["mod_init"], pb["ltran"])
        eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        eng.set_sequences(LENGTHS)
        with pytest.raises(RuntimeError, match="K = 300 > 256"):
            eng.estep_sequences()
    _case1(eng)


# ---- 8: after the call --------------------------------------------------------------------------------
def test_intermediates_after_the_call(eng):
    K = 5
    pb = load_niw(eng, K)
    ref_q, _, _ = niw_posteriors(K, D, LENGTHS, seed_of(K), True)
    st, _, _ = eng.estep_sequences(flags=MASK_AS_NAN)
    true_sts = (pb["sts"] % K).astype(np.int32)
    z, conf = eng.state_argmax(true_sts)
    want = np.argmax(ref_q, axis=1)
    assert np.array_equal(z, want)
    ref_conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(ref_conf, (want, true_sts), 1)
    assert np.array_equal(conf, ref_conf)
    for name in ("lliks", "lalpha", "lbeta"):
        with pytest.raises(RuntimeError, match="svihmm_estep_sequences keeps var_x only"):
            eng.read_rows(name, 0, 4)
    with pytest.raises(RuntimeError, match="svihmm_estep_sequences keeps var_x only"):
        eng.read_intermediate("lalpha", 1, T)
    assert np.array_equal(eng.read_packed().buf, st.buf)
    # an ordinary E-step afterwards has all four again
    eng.forward_backward([200], 100, want=())
    assert eng.read_rows("lalpha", 0, 4).shape == (4, K)


# ---- 9: the batch classes on the device against the oracle engine -------------------------------------
@pytest.mark.parametrize("name", ["cd", "sgd"])
def test_batch_classes_on_a_list(name):
    from oracle.engine import OracleEngine
    from pysvihmm_amd import hmmbatchcd, hmmbatchsgd
    mod = hmmbatchsgd if name == "sgd" else hmmbatchcd
    lengths = (40, 1, 2100, 17)
    seqs, masks = class_data(lengths)
    ref = build_model(mod, seqs, masks, OracleEngine(), maxit=5)
    ref.infer()
    hmm = build_model(mod, seqs, masks, None, maxit=5)
    calls = []
    est = hmm.engine.estep_sequences
    hmm.engine.estep_sequences = lambda *a, **k: (calls.append(1), est(*a, **k))[1]
    hmm.infer()
    assert len(calls) == 5                                  # one device call per iteration
    assert len(hmm.elbo_vec) == len(ref.elbo_vec) == 5
    np.testing.assert_allclose(hmm.var_tran, ref.var_tran, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(hmm.elbo_vec, ref.elbo_vec, rtol=1e-8)
    np.testing.assert_allclose(hmm.var_x, ref.var_x, rtol=1e-6, atol=1e-11)
    np.testing.assert_allclose(hmm.lalpha, ref.lalpha, rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(hmm.var_init, ref.var_init, rtol=1e-6, atol=1e-9)
    hmm.engine.close()
