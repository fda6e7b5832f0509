"""svihmm_estep_sequence_subset / Engine.estep_sequence_subset / hmmbatchsgd.VBHMM(seq_minibatch=M): the E-step of
a minibatch of whole sequences in one device call, against the per-sequence oracle results summed over the list with
multiplicity (tests/seq_minibatch_helpers.py).  Data and tolerances: those of test_gpu_sequences.py.

Lengths (1, 2, 3, 63, 64, 65, 257, 2047, 2048, 2311, 1): both ends a one-row sequence, one sequence either side of
the wave width, one just below the chain threshold, one chain-routed with a tail chunk."""
import numpy as np
import pytest

from helpers import make_problem
from seq_minibatch_helpers import niw_sequence_results, oracle_sequence_results, subset_rows, subset_sum
from sequences_helpers import (LENGTHS, MASK_AS_NAN, TRANS_WRAP, build_model, class_data, niw_problem, offsets)
from test_gpu_sequences import D, LEN4, LEN5, check_packed, load_niw, seed_of

pytestmark = pytest.mark.gpu
RTOL = 1e-6
T = int(sum(LENGTHS))
OFF = offsets(LENGTHS)
N = len(LENGTHS)
FLAGS = [0, MASK_AS_NAN, TRANS_WRAP]
MIXED = (9, 0, 6, 6, 10, 3)      # chain-routed, both one-row sequences, a duplicate, ragged


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def rows_of(lengths, idx):
    return int(sum(lengths[s] for s in idx))


def check_subset(eng, per_seq, lengths, idx, flags, K, Dd, kind="niw"):
    """One subset call against the reference: packed, seq_lb in the order of idx, q0, the R posterior rows."""
    R = rows_of(lengths, idx)
    ref_buf, ref_lb, ref_q, ref_q0 = subset_sum(per_seq, idx)
    st, seq_lb, q0 = eng.estep_sequence_subset(idx, flags=flags)
    check_packed(st, ref_buf, K, Dd, R, kind=kind)
    assert seq_lb.shape == (len(idx),)
    np.testing.assert_allclose(seq_lb, ref_lb, rtol=1e-10)
    np.testing.assert_allclose(q0, ref_q0, rtol=RTOL, atol=1e-12)
    q = eng.read_rows("var_x", 0, R)
    np.testing.assert_allclose(q, ref_q, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(q.sum(-1), 1.0, rtol=1e-11)
    with pytest.raises(RuntimeError, match="out of range"):
        eng.read_rows("var_x", R, 1)
    return st, seq_lb, q0, q


# ---- 1: a mixed subset -----------------------------------------------------------------------------
@pytest.mark.parametrize("K,flags", [(K, f) for K in (5, 64, 80) for f in FLAGS] + [(256, 0)])
def test_mixed_subset_vs_oracle(eng, K, flags):
    load_niw(eng, K)
    check_subset(eng, niw_sequence_results(K, D, LENGTHS, seed_of(K), flags), LENGTHS, MIXED, flags, K, D)


# ---- 2: the smallest cases ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("idx", [(0,), (8, 9), (3, 4, 5)], ids=["one_row", "chain_only", "ragged_only"])
def test_smallest_subsets_vs_oracle(eng, idx, flags):
    K = 5
    load_niw(eng, K)
    st, _, q0, q = check_subset(eng, niw_sequence_results(K, D, LENGTHS, seed_of(K), flags), LENGTHS, idx, flags, K, D)
    if idx == (0,):
        # R = 1: no transition pair without the wrap; with it the row is its own predecessor
        want = np.outer(q[0], q[0]) if flags & TRANS_WRAP else np.zeros((K, K))
        np.testing.assert_allclose(st.A_raw, want, rtol=1e-12, atol=0)
        assert np.array_equal(q0, q[0])


# ---- 3: the whole list is svihmm_estep_sequences, bit for bit ------------------------------------------
@pytest.mark.parametrize("K", [16, 80])
def test_the_whole_list_is_the_full_call(eng, K):
    load_niw(eng, K)
    a = eng.estep_sequences(flags=TRANS_WRAP)
    qa = eng.read_rows("var_x", 0, T)
    b = eng.estep_sequence_subset(range(N), flags=TRANS_WRAP)
    qb = eng.read_rows("var_x", 0, T)
    assert np.array_equal(a[0].buf, b[0].buf)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(qa, qb)
    c = eng.estep_sequence_subset(np.arange(N), flags=TRANS_WRAP)          # two identical calls
    assert np.array_equal(b[0].buf, c[0].buf) and np.array_equal(b[1], c[1]) and np.array_equal(b[2], c[2])
    assert np.array_equal(qb, eng.read_rows("var_x", 0, T))


# ---- 4: a listed sequence does not depend on the rest of the list ---------------------------------------
@pytest.mark.parametrize("K", [16, 80])
def test_a_listed_sequence_does_not_depend_on_the_list(eng, K):
    """Sequences 6 (257 rows, ragged sweeps) and 9 (2311 rows, whole-chain scan): listed alone, in the mixed list
    and in the full call their posterior rows and local_lb are the same bits; so are the two occurrences of 6."""
    load_niw(eng, K)
    _, lb_full, _ = eng.estep_sequences(flags=MASK_AS_NAN, read=False)
    q_full = eng.read_rows("var_x", 0, T)
    _, lb_mix, _ = eng.estep_sequence_subset(MIXED, flags=MASK_AS_NAN, read=False)
    q_mix = eng.read_rows("var_x", 0, rows_of(LENGTHS, MIXED))
    off_mix = offsets([LENGTHS[s] for s in MIXED])
    for s in (6, 9):
        _, lb_one, _ = eng.estep_sequence_subset((s,), flags=MASK_AS_NAN, read=False)
        q_one = eng.read_rows("var_x", 0, LENGTHS[s])
        assert np.array_equal(q_one, q_full[OFF[s]:OFF[s + 1]]), "rows of sequence %d, alone / full call" % s
        assert lb_one[0] == lb_full[s]
        for m in [m for m, v in enumerate(MIXED) if v == s]:
            assert np.array_equal(q_mix[off_mix[m]:off_mix[m + 1]], q_one), "rows of sequence %d at %d" % (s, m)
            assert lb_mix[m] == lb_one[0]


# ---- 5: nothing is disturbed ------------------------------------------------------------------------------
def test_the_resident_state_is_not_disturbed(eng):
    K = 5
    load_niw(eng, K)
    a = eng.estep_sequences(flags=TRANS_WRAP)
    qa = eng.read_rows("var_x", 0, T)
    st, _, _ = eng.estep_sequence_subset(MIXED, flags=MASK_AS_NAN)
    assert np.array_equal(eng.read_packed().buf, st.buf)
    with pytest.raises(RuntimeError, match="window 0 .*two sequences"):
        eng.estep([60], 20)                                   # rows 60 .. 79: sequence 3 ends at row 68
    eng.estep_sequence_subset(MIXED, flags=MASK_AS_NAN, read=False)
    b = eng.estep_sequences(flags=TRANS_WRAP)
    qb = eng.read_rows("var_x", 0, T)
    assert np.array_equal(a[0].buf, b[0].buf)
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and np.array_equal(qa, qb)
    assert eng.T == T and len(eng.seq_off) == N + 1


# ---- 6: diagonal and Categorical families -------------------------------------------------------------------
@pytest.fixture(scope="module")
def family_refs():
    """Per family: the inputs and, per flag word, the oracle engine's per-sequence results (computed once)."""
    from oracle.engine import OracleEngine
    rows = int(sum(LEN4))
    out = {}
    for family in ("diag", "cat"):
        rng = np.random.default_rng(5)
        oe = OracleEngine()
        if family == "diag":
            K, Dd = 6, 4
            pb = make_problem(K, Dd, rows, seed=77, miss=0.1)
            par = (pb["mu"], 0.5 + rng.random((K, Dd)), 2.0 + rng.random((K, Dd)), 1.0 + rng.random((K, Dd)))
            obs = pb["obs"]
        else:
            K, V, Dd = 3, 5, 1
            pb = make_problem(K, 1, rows, seed=78, miss=0.1)
            obs = rng.integers(0, V, size=(rows, 1)).astype(np.float64)
            par = (np.log(rng.dirichlet(np.ones(V), size=K)),)
        oe.set_obs(obs, pb["mask"])
        oe.set_globals(pb["mod_init"], pb["ltran"])
        (oe.set_emission_diag if family == "diag" else oe.set_emission_cat)(*par)
        out[family] = dict(K=K, Dd=Dd, pb=pb, obs=obs, par=par,
                           ref={f: oracle_sequence_results(oe, LEN4, f) for f in FLAGS})
    return out


@pytest.mark.parametrize("flags", FLAGS)
@pytest.mark.parametrize("family", ["diag", "cat"])
def test_diag_and_categorical_vs_oracle_engine(eng, family_refs, family, flags):
    r = family_refs[family]
    eng.set_obs(r["obs"], r["pb"]["mask"])
    eng.set_globals(r["pb"]["mod_init"], r["pb"]["ltran"])
    (eng.set_emission_diag if family == "diag" else eng.set_emission_cat)(*r["par"])
    eng.set_sequences(LEN4)
    check_subset(eng, r["ref"][flags], LEN4, (3, 0, 2, 0), flags, r["K"], r["Dd"], kind=family)


# ---- 7: sparse globals (the literal logaddexp form) -------------------------------------------------------------
@pytest.mark.parametrize("flags", FLAGS)
def test_sparse_globals_vs_oracle(eng, flags):
    K = 6
    pb = load_niw(eng, K, LEN5, sparse=True)
    assert pb["ltran"].min() < -600.0
    check_subset(eng, niw_sequence_results(K, D, LEN5, seed_of(K), flags, sparse=True), LEN5, (2, 0, 2), flags, K, D)


# ---- 8: errors leave the handle usable ----------------------------------------------------------------------------
@pytest.mark.parametrize("what", ["no_declaration", "empty", "entry_N", "entry_minus_1", "host_lliks", "K300"])
def test_errors_leave_the_handle_usable(eng, what):
    from pysvihmm_amd import _lib as L
    load_niw(eng, 5, declare=(what != "no_declaration"))
    if what == "no_declaration":
        with pytest.raises(RuntimeError, match="no sequences declared"):
            eng.estep_sequence_subset(MIXED)
    elif what == "empty":
        with pytest.raises(RuntimeError, match="idx is empty"):
            eng.estep_sequence_subset([])
    elif what == "entry_N":
        with pytest.raises(RuntimeError, match=r"idx\[2\] = %d is outside \[0, N = %d\)" % (N, N)):
            eng.estep_sequence_subset((9, 0, N, 3))
    elif what == "entry_minus_1":
        with pytest.raises(RuntimeError, match=r"idx\[1\] = -1 is outside"):
            eng.estep_sequence_subset((9, -1))
    elif what == "host_lliks":
        with pytest.raises(RuntimeError, match="HOST_LLIKS"):
            eng.estep_sequence_subset(MIXED, flags=L.USE_HOST_LLIKS)
    else:
        pb = make_problem(300, D, T, seed=3)
        eng.set_globals(pb["mod_init"], pb["ltran"])
        eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        with pytest.raises(RuntimeError, match="K = 300 > 256"):
            eng.estep_sequence_subset(MIXED)
    K = 5
    load_niw(eng, K)
    check_subset(eng, niw_sequence_results(K, D, LENGTHS, seed_of(K), 0), LENGTHS, MIXED, 0, K, D)


def test_intermediates_after_the_call(eng):
    K = 5
    pb = load_niw(eng, K)
    per_seq = niw_sequence_results(K, D, LENGTHS, seed_of(K), MASK_AS_NAN)
    eng.estep_sequence_subset(MIXED, flags=MASK_AS_NAN, read=False)
    R = rows_of(LENGTHS, MIXED)
    true_sts = (pb["sts"] % K).astype(np.int32)[subset_rows(LENGTHS, MIXED)]
    z, conf = eng.state_argmax(true_sts)
    want = np.argmax(subset_sum(per_seq, MIXED)[2], axis=1)
    assert z.shape == (R,) and np.array_equal(z, want)
    ref_conf = np.zeros((K, K), dtype=np.int64)
    np.add.at(ref_conf, (want, true_sts), 1)
    assert np.array_equal(conf, ref_conf)
    for name in ("lliks", "lalpha", "lbeta"):
        with pytest.raises(RuntimeError, match="svihmm_estep_sequence_subset keeps var_x"):
            eng.read_rows(name, 0, 4)
    with pytest.raises(RuntimeError, match="svihmm_estep_sequence_subset keeps var_x"):
        eng.read_intermediate("lalpha", 1, R)
    # an ordinary E-step afterwards has all four again
    eng.forward_backward([200], 100, want=())
    for name in ("lliks", "lalpha", "lbeta", "var_x"):
        assert eng.read_rows(name, 0, 4).shape == (4, K)


# ---- 9: the class on the device against the oracle engine -------------------------------------------------------------
def test_minibatch_class_on_the_device():
    from oracle.engine import OracleEngine
    from pysvihmm_amd import hmmbatchsgd
    lengths = (40, 1, 2100, 17)
    seqs, masks = class_data(lengths)
    ref = build_model(hmmbatchsgd, seqs, masks, OracleEngine(), maxit=5, seq_minibatch=2)
    np.random.seed(2024)
    ref.infer()
    hmm = build_model(hmmbatchsgd, seqs, masks, None, maxit=5, seq_minibatch=2)
    calls = {"subset": 0, "full": 0}
    sub, full = hmm.engine.estep_sequence_subset, hmm.engine.estep_sequences

    def count(name, f):
        def g(*a, **k):
            calls[name] += 1
            return f(*a, **k)
        return g
    hmm.engine.estep_sequence_subset = count("subset", sub)
    hmm.engine.estep_sequences = count("full", full)
    np.random.seed(2024)
    hmm.infer()
    assert calls == {"subset": 5, "full": 1}
    assert len(hmm.elbo_vec) == len(ref.elbo_vec) == 5 and hmm.batchfactor == 2.0
    np.testing.assert_allclose(hmm.var_tran, ref.var_tran, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(hmm.elbo_vec, ref.elbo_vec, rtol=1e-8)
    np.testing.assert_allclose(hmm.var_x, ref.var_x, rtol=1e-6, atol=1e-11)
    np.testing.assert_allclose(hmm.var_init, ref.var_init, rtol=1e-6, atol=1e-9)
    assert hmm.var_x.shape == (sum(lengths), 4)
    hmm.engine.close()
