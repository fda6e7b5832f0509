"""svihmm_set_emission_mcat on the MI355X: D symbol columns, independent given the state.

The lookup (k_emission_mcat) is held to the contract's loop bit for bit; the counts (k_stats_onehot, a GEMM
with a one-hot operand on v_mfma_f64_16x16x4_f64) to the tolerances tests/test_categorical.py applies to the one-column
family: statistics rtol 1e-6 with atol 1e-9 x (rows of the batch), lb rtol 1e-10.  Shapes: K = 3 (one ragged state
tile), 16 with F = 21 (F no multiple of 16), 64, 65 (a second state group of one state; a one-symbol column), 256
with F = 96 (the table beyond 64 KB: read through L2; four state groups) and, for the lookup and the caller's
posteriors, K = 16 with F = 260 (thirteen columns of twenty symbols: four feature tiles per wave, a second feature
group of four features; the 33 KB table is staged).  Every data set holds single NaN entries,
whole NaN rows, a row whose every column is absent, masked rows, one entry equal to V[d] and one negative entry."""
import re

import numpy as np
import pytest

from oracle import ref_c
from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from tests.decode_sequences_helpers import (backward_sample_sequences, check_paths_sequences,
                                            near_boundary_sequences, offsets)
from tests.grow_helpers import grow_batch, grow_direct
from tests.mcat_helpers import (IDS, LENGTHS, SHAPES, T, mcat_counts, mcat_lliks, present, problem, split_tables,
                                window_rows)
from tests.viterbi_helpers import viterbi_numpy

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def push(e, p, x=None, mask=None):
    e.set_obs(p["x"] if x is None else x, p["mask"] if mask is None else mask)
    e.set_globals(p["mod_init"], p["ltran"])
    e.set_emission_mcat(split_tables(p["logp"], p["V"]))


def packed_len(e):
    return int(e._lib.svihmm_packed_len(e._h))


def tran_batch(q):
    return q[:-1].T.dot(q[1:]) if len(q) > 1 else np.zeros((q.shape[1], q.shape[1]))


def check_stats(st, A, counts, lb, scale):
    np.testing.assert_allclose(st.A_raw, A, rtol=1e-6, atol=1e-9 * scale)
    np.testing.assert_allclose(st.flat, counts, rtol=1e-6, atol=1e-9 * scale)
    if lb is not None:
        np.testing.assert_allclose(st.lb[0], lb, rtol=1e-10)


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_loglik_is_the_contract_loop_bit_for_bit(eng, i):
    p = problem(i)
    push(eng, p)
    B, Lm = 5, 37
    starts = (np.arange(B) * 131) % (T - Lm + 1)
    rows = window_rows(starts, Lm)
    for flags in (0, L.MASK_AS_NAN):
        ll = eng.loglik(starts, Lm, flags=flags)
        want = mcat_lliks(p["x"][rows], p["mask"][rows], p["V"], p["logp"], flags).reshape(B, Lm, p["K"])
        np.testing.assert_array_equal(ll, want)
    assert packed_len(eng) == p["K"] ** 2 + p["K"] * sum(p["V"]) + 1


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_one_column_equals_the_categorical_family(eng, i):
    p = problem(i)
    K, V0 = p["K"], p["V"][0]
    x1 = np.ascontiguousarray(p["x"][:, :1])
    tab = np.ascontiguousarray(p["logp"][:, :V0])
    starts = np.array([0, 300, T - 37])
    eng.set_obs(x1, p["mask"])
    eng.set_globals(p["mod_init"], p["ltran"])
    for flags in (0, L.MASK_AS_NAN):
        eng.set_emission_mcat([tab])
        a = eng.loglik(starts, 37, flags=flags)
        eng.set_emission_cat(tab)
        b = eng.loglik(starts, 37, flags=flags)
        np.testing.assert_array_equal(a, b)
        np.testing.assert_array_equal(a[1], mcat_lliks(x1[300:337], p["mask"][300:337], (V0,), tab, flags))


def oracle_estep(p, starts, Lm, flags, inner=None):
    """Referee: the NumPy lliks through the oracle's recursions (``OracleEngine.set_lliks`` + USE_HOST_LLIKS):
    var_x, A_raw and lb as ``OracleEngine.estep`` forms them -- its own statements, without the loop over the
    K NIW factors that call also runs (7 s at K = 256) --, counts of the oracle's posteriors.  The recursions run
    once per distinct window and lliks (the oracle takes 70 ms per 16-row window at K = 256) and are shared by the
    flag words that only change the statistics."""
    starts = np.asarray(starts, dtype=np.int64)
    B, K = len(starts), p["K"]
    us, inv, cnt = np.unique(starts, return_inverse=True, return_counts=True)
    key = (id(p["x"]), id(p["logp"]), flags & L.MASK_AS_NAN, us.tobytes(), Lm)
    if key not in _fb:
        rows = window_rows(us, Lm)
        ll = mcat_lliks(p["x"][rows], p["mask"][rows], p["V"], p["logp"], flags).reshape(len(us), Lm, K)
        o = OracleEngine()
        o.set_globals(p["mod_init"], p["ltran"])
        o.set_lliks(ll)
        _fb.clear()                     # (one entry: the cases of a test follow each other)
        _fb[key] = o.forward_backward(None, Lm, flags=flags | L.USE_HOST_LLIKS, want=("var_x", "local_lb"), B=len(us))
    res = _fb[key]
    off, ln = (0, Lm) if inner is None else inner
    qu = res["var_x"][:, off:off + ln]
    tran = R.transition_stat_wrap if flags & L.TRANS_WRAP else R.transition_stat_batch
    A = sum(cnt[u] * tran(qu[u]) for u in range(len(us)))
    r = window_rows(starts + off, ln)
    return A, mcat_counts(p["x"][r], p["mask"][r], p["V"], qu[inv].reshape(B * ln, K)), float(res["local_lb"][inv].sum())


_fb = {}


@pytest.mark.parametrize("B,Lm", [(6, 37), (192, 16)], ids=["log", "scaled"])
@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_estep_against_the_oracle(eng, i, B, Lm):
    p = problem(i)
    push(eng, p)
    # (24 distinct windows, each eight times in the large batch: the device sweeps all 192, the referee 24)
    starts = np.tile((np.arange(min(B, 24)) * 29) % (T - Lm + 1), max(1, B // 24))
    assert len(starts) == B
    for flags in (0, L.TRANS_WRAP, L.TRANS_WRAP | L.MASK_AS_NAN):
        st = eng.estep(starts, Lm, flags=flags)
        check_stats(st, *oracle_estep(p, starts, Lm, flags), scale=B * Lm)
    inner = (5, Lm - 9)
    st = eng.estep(starts, Lm, flags=L.TRANS_WRAP, inner=inner)
    check_stats(st, *oracle_estep(p, starts, Lm, L.TRANS_WRAP, inner), scale=B * Lm)


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_suffstats_row_count_edges_and_reproducibility(eng, i):
    p = problem(i)
    push(eng, p)
    K = p["K"]
    rng = np.random.default_rng(7 + i)
    for B, Lm in [(1, 1), (3, 1), (2, 2), (1, 5), (9, 7), (1, 64), (5, 13)]:       # 1, 3, 4, 5, 63, 64, 65 rows
        starts = (np.arange(B) * 97 + 11) % (T - Lm + 1)
        q = rng.dirichlet(np.ones(K), size=(B, Lm))
        q[rng.random((B, Lm)) < 0.2] = 0.0
        rows = window_rows(starts, Lm)
        a = eng.suffstats(starts, Lm, q, flags=0)
        b = eng.suffstats(starts, Lm, q, flags=0)
        np.testing.assert_array_equal(a.buf, b.buf)
        A = sum(tran_batch(q[w]) for w in range(B))
        check_stats(a, A, mcat_counts(p["x"][rows], p["mask"][rows], p["V"], q.reshape(B * Lm, K)), None, B * Lm)
        assert a.lb[0] == 0.0


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_suffstats_ignores_posteriors_of_rows_that_do_not_count(eng, i):
    """A masked row and a row without a present entry add nothing, whatever the caller left in their posterior
    rows (the rule of the one-column family, which never reads them): NaN and Inf there stay out of the counts."""
    p = problem(i)
    push(eng, p)
    K, B, Lm = p["K"], 4, 150
    starts = np.array([0, 150, 300, 450])
    rows = window_rows(starts, Lm)
    _, ok = present(p["x"][rows], p["V"])
    dead = p["mask"][rows] | ~ok.any(1)
    assert dead.sum() >= 5 and (~ok.any(1) & ~p["mask"][rows]).any() and p["mask"][rows].any()
    q = np.random.default_rng(50 + i).dirichlet(np.ones(K), size=B * Lm)
    clean = q.copy()
    clean[dead] = 0.0
    q[dead] = np.where(np.arange(dead.sum())[:, None] % 2 == 0, np.nan, np.inf)
    st = eng.suffstats(starts, Lm, q.reshape(B, Lm, K), flags=0)
    assert np.all(np.isfinite(st.flat))
    np.testing.assert_allclose(st.flat, mcat_counts(p["x"][rows], p["mask"][rows], p["V"], clean), rtol=1e-6,
                               atol=1e-9 * B * Lm)


def seq_problem(i):
    p = dict(problem(i))
    Ts = sum(LENGTHS)
    p["x"], p["mask"] = p["x"][:Ts], p["mask"][:Ts]
    return p, offsets(LENGTHS), Ts


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_estep_sequences_and_subset(eng, i):
    p, off, Ts = seq_problem(i)
    K, V = p["K"], p["V"]
    push(eng, p)
    per = []
    for s, ln in enumerate(LENGTHS):
        a = int(off[s])
        r = eng.forward_backward([a], ln, flags=0, want=("var_x", "local_lb"))
        q = r["var_x"][0]
        per.append((tran_batch(q), mcat_counts(p["x"][a:a + ln], p["mask"][a:a + ln], V, q), float(r["local_lb"][0]),
                    q[0].copy()))
    eng.set_sequences(LENGTHS)
    st, seq_lb, q0 = eng.estep_sequences(flags=0)
    check_stats(st, sum(x[0] for x in per), sum(x[1] for x in per), sum(x[2] for x in per), Ts)
    np.testing.assert_allclose(seq_lb, [x[2] for x in per], rtol=1e-10)
    np.testing.assert_allclose(q0, sum(x[3] for x in per), rtol=1e-6, atol=1e-9)
    idx = (4, 0, 4)
    st, seq_lb, q0 = eng.estep_sequence_subset(idx, flags=0)
    check_stats(st, sum(per[s][0] for s in idx), sum(per[s][1] for s in idx), sum(per[s][2] for s in idx),
                sum(LENGTHS[s] for s in idx))
    np.testing.assert_allclose(seq_lb, [per[s][2] for s in idx], rtol=1e-10)


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_viterbi_sequences_equals_numpy_on_its_own_lliks(eng, i):
    p, off, Ts = seq_problem(i)
    push(eng, p)
    eng.set_sequences(LENGTHS)
    z, score = eng.viterbi_sequences(flags=L.MASK_AS_NAN)
    ll = eng.read_rows("lliks", 0, Ts)
    np.testing.assert_array_equal(ll, mcat_lliks(p["x"], p["mask"], p["V"], p["logp"], L.MASK_AS_NAN))
    for s in range(len(LENGTHS)):
        a, b = int(off[s]), int(off[s + 1])
        zr, sr = viterbi_numpy(ll[a:b], p["mod_init"], p["ltran"])
        np.testing.assert_array_equal(z[a:b], zr)
        assert score[s] == sr


FFBS_SEED = 0       # for every shape the NumPy paths of this seed have no step near a CDF boundary (asserted on the CPU)


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_ffbs_sequences_paths(eng, i):
    p, off, Ts = seq_problem(i)
    K, S = p["K"], 3
    logA = p["ltran"]
    ll = mcat_lliks(p["x"], p["mask"], p["V"], p["logp"], 0)
    la_ref = np.concatenate([ref_c.forward(np.ascontiguousarray(ll[int(a):int(b)]), p["mod_init"], p["ltran"])
                             for a, b in zip(off[:-1], off[1:])])
    u = np.random.default_rng(FFBS_SEED).random((S, Ts))
    z_np = backward_sample_sequences(la_ref, logA, u, off)
    assert near_boundary_sequences(z_np, la_ref, logA, u, off) == 0         # CPU first
    push(eng, p)
    eng.set_sequences(LENGTHS)
    z, la = eng.ffbs_sequences(logA, n_draws=S, uniforms=u, want_lalpha=True)
    assert z.shape == (S, Ts) and la.shape == (Ts, K)
    assert check_paths_sequences(z, la, logA, u, off) <= 1


def grow_case():
    """K = 16, seven three-symbol tracks from a sticky chain; the states overlap, so the widths differ."""
    K, V = SHAPES[1]
    rng = np.random.default_rng(5)
    Tg = 600
    theta = [rng.dirichlet(np.ones(v), size=K) for v in V]
    sts = np.repeat(rng.integers(0, K, size=Tg // 25 + 1), 25)[:Tg]
    x = np.stack([[rng.choice(v, p=th[s]) for s in sts] for v, th in zip(V, theta)], axis=1).astype(float)
    logp = np.log(np.concatenate(theta, axis=1) * 0.97 + 0.01)
    A = np.full((K, K), 0.1 / (K - 1))
    np.fill_diagonal(A, 0.9)
    return dict(K=K, V=V, x=x, mask=np.zeros(Tg, bool), logp=logp, mod_init=np.log(np.ones(K) / K), ltran=np.log(A)), Tg


def test_grow_windows_products_equals_literal(eng):
    p, Tg = grow_case()
    centers = np.array([93, 116, 139, 162, 208, 231, 277, 300, 323, 346], dtype=np.int64)
    rule = dict(half0=4, m=0, inc=2, cutoff=60, eps=1e-5, rule=0)
    ll = mcat_lliks(p["x"], None, p["V"], p["logp"], 0)
    compared = []
    for c in centers:
        grow_direct(ll, p["mod_init"], p["ltran"], Tg, int(c), compared=compared, **rule)
    compared = np.array(compared)
    # margin, on the CPU: every residual the rule compares is a factor 3 away from epsilon (the two routes differ by rounding)
    assert len(compared) and np.all((compared < rule["eps"] / 3) | (compared > rule["eps"] * 3))
    want = grow_batch(grow_direct, [ll] * len(centers), [0] * len(centers), p["mod_init"], p["ltran"], Tg, centers, **rule)
    push(eng, p)
    kw = dict(probe_off=rule["m"], increment=rule["inc"], cutoff=rule["cutoff"], epsilon=rule["eps"], rule=0)
    h_lit, s_lit, _ = eng.grow_windows(centers, rule["half0"], method="literal", **kw)
    h_pro, s_pro, _ = eng.grow_windows(centers, rule["half0"], method="products", **kw)
    np.testing.assert_array_equal(h_lit, h_pro)
    np.testing.assert_array_equal(s_lit, s_pro)
    np.testing.assert_array_equal(h_lit, want[0])
    assert len(set(h_lit.tolist())) > 1


def test_hand_over_between_families(eng):
    """A symbol matrix uploaded under the NIW family is centred; the table family that follows must see exact
    integers again, and a Gaussian family after it its centred copy."""
    p = problem(0)
    K, V, D = p["K"], p["V"], len(p["V"])
    x = np.nan_to_num(p["x"], nan=1.0)                               # (finite rows: the NIW family evaluates them)
    rng = np.random.default_rng(3)
    niw = (rng.normal(size=(K, D)) + 1.0, np.stack([np.eye(D) * 2.0] * K), np.ones(K), np.full(K, D + 3.0))
    starts, Lm = np.array([0, 99, 500]), 37
    rows = window_rows(starts, Lm)
    want = mcat_lliks(x[rows], p["mask"][rows], V, p["logp"], 0).reshape(3, Lm, K)
    eng.set_globals(p["mod_init"], p["ltran"])
    eng.set_emission_niw(*niw)
    eng.set_obs(x, p["mask"])
    assert np.any(eng.get_shift() != 0.0)                            # the copy is centred
    ll_niw = eng.loglik(starts, Lm)
    assert packed_len(eng) == K * K + K * D + K + K * D * D + 1
    for _ in range(2):
        eng.set_emission_mcat(split_tables(p["logp"], V))
        assert packed_len(eng) == K * K + K * sum(V) + 1
        np.testing.assert_array_equal(eng.loglik(starts, Lm), want)
        st = eng.estep(starts, Lm, flags=0)
        check_stats(st, *oracle_estep(dict(p, x=x), starts, Lm, 0), scale=3 * Lm)
        eng.set_emission_niw(*niw)
        assert packed_len(eng) == K * K + K * D + K + K * D * D + 1
        np.testing.assert_allclose(eng.loglik(starts, Lm), ll_niw, rtol=1e-9, atol=1e-9)


def test_packed_round_trip(eng):
    p = problem(3)
    push(eng, p)
    starts = np.arange(4) * 50
    st = eng.estep(starts, 40, flags=L.TRANS_WRAP)
    buf = st.buf.copy()
    wire = eng.export_packed()
    np.testing.assert_array_equal(wire, buf)                         # counts carry no coordinates
    eng.import_packed(wire)
    np.testing.assert_array_equal(eng.read_packed().buf, buf)


def test_failures_leave_the_handle_usable(eng):
    p = problem(0)
    push(eng, p)
    K, V = p["K"], p["V"]
    starts = np.array([3, 200])
    want = eng.loglik(starts, 20)
    lib, h = eng._lib, eng._h
    import ctypes as C

    def call(K_, D_, Vs, logp, msg):
        v = None if Vs is None else np.ascontiguousarray(Vs, dtype=np.int32)
        t = None if logp is None else np.ascontiguousarray(logp, dtype=np.float64)
        with pytest.raises(RuntimeError, match="^" + re.escape("svihmm_set_emission_mcat failed: svihmm_set_emission_mcat: ") + ".*" + msg):
            L.check(lib.svihmm_set_emission_mcat(h, K_, D_, None if v is None else v.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 L.dptr(t)), "svihmm_set_emission_mcat")
        np.testing.assert_array_equal(eng.loglik(starts, 20), want)  # the family set before is still in force
    ok = p["logp"]
    call(K, 2, None, ok, "NULL")
    call(K, 2, V, None, "NULL")
    call(0, 2, V, ok, "K = 0")
    call(257, 2, V, np.zeros((257, 7)), "K = 257")
    call(K, 0, V, ok, "D = 0")
    call(K, L.MCAT_MAX_D + 1, np.ones(L.MCAT_MAX_D + 1), np.zeros((K, L.MCAT_MAX_D + 1)), "SVIHMM_MCAT_MAX_D")
    call(K, 2, (2, 0), ok, re.escape("V[1] = 0"))
    call(K, 2, (1000, 25), np.zeros((K, 1025)), "SVIHMM_MCAT_MAX_F")
    for bad in (np.nan, np.inf, -np.inf):
        t = ok.copy()
        t[1, 4] = bad
        call(K, 2, V, t, re.escape("logp[1][4] is not finite"))
    # resident observations of another width: refused at the first E-step-type call, before any device work
    eng.set_obs(np.zeros((50, 3)))
    for fn in (lambda: eng.loglik([0], 20), lambda: eng.estep([0], 20), lambda: eng.viterbi([0], 20)):
        with pytest.raises(RuntimeError, match="svihmm_set_emission_mcat: the family has D = 2 symbol columns, the "
                                               "resident observations have 3"):
            fn()
    eng.set_obs(p["x"], p["mask"])
    np.testing.assert_array_equal(eng.loglik(starts, 20), want)


def test_refusals(eng):
    p = problem(0)
    push(eng, p)
    with pytest.raises(RuntimeError, match="svihmm_pred_logprob: NIW emission only"):
        eng.pred_logprob([0, 40], 30)
    with pytest.raises(RuntimeError, match="svihmm_svi_iteration: the resident SVI loop does not take the multi-column"):
        eng.svi_iteration(0, [0, 40], 2, 30, L.TRANS_WRAP, 0.5, 1.0, 1.0)
    np.testing.assert_array_equal(eng.loglik([0], 20)[0], mcat_lliks(p["x"][:20], None, p["V"], p["logp"], 0))


def test_fp32_mode_is_not_taken():
    from pysvihmm_amd.engine import HipEngine
    p = problem(2)
    e = HipEngine(0)
    try:
        e.set_precision("f32")
        push(e, p)
        B, Lm = 192, 16
        starts = (np.arange(B) * 13) % (T - Lm + 1)
        st = e.estep(starts, Lm, flags=L.TRANS_WRAP)
        assert e.precision() == ("f32", False)
        check_stats(st, *oracle_estep(p, starts, Lm, L.TRANS_WRAP), scale=B * Lm)
    finally:
        e.close()
