"""svihmm_set_emission_poisson on the MI355X: D count columns, independent Poisson rates given the state.

The lookup (k_emission_poisson) is held to the contract's loop bit for bit; the statistics (k_stats_columns, a GEMM on
v_mfma_f64_16x16x4_f64 whose A operand is the count or one) to the project's tolerances for count statistics
(tests/test_categorical.py, tests/test_gpu_mcat.py): A_raw and n rtol 1e-6 with atol 1e-9 x (rows of the batch), sx the
same with atol additionally x the largest present count of the data set (the scale of its summands), lb rtol 1e-10.
Shapes (tests/poisson_helpers.py): K = 3 and 16 (ragged state tiles, F = 4 and 14), 64 (one column of base rate 3000),
65 (a second state group of one state), (256, 40) (F = 80, tables beyond 64 KB: read through L2) and, for the lliks
and the suffstats tests, (16, 128) (D at the limit, F = 256).  Every data set holds single NaN entries, whole NaN rows,
a row whose every column is absent, masked rows, an entry equal to C, one equal to C + 1, a +inf, a -0.5 and a 3.7."""
import ctypes as C
import re

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from tests import poisson_helpers as H
from tests.decode_sequences_helpers import check_paths_sequences, near_boundary_sequences
from tests.grow_helpers import grow_batch, grow_direct
from tests.poisson_helpers import (IDS, LENGTHS, T, lliks_of, poisson_stats, present, problem, seq_problem,
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
    e.set_emission_poisson(p["elog"], p["erate"], p["C"])


def packed_len(e):
    return int(e._lib.svihmm_packed_len(e._h))


def tran_batch(q):
    return q[:-1].T.dot(q[1:]) if len(q) > 1 else np.zeros((q.shape[1], q.shape[1]))


def max_count(p):
    c, ok = present(p["x"], p["C"])
    return float(c[ok].max())


def check_stats(st, A, stat, lb, scale, cmax):
    D = st.D
    np.testing.assert_allclose(st.A_raw, A, rtol=1e-6, atol=1e-9 * scale)
    np.testing.assert_allclose(st.n, stat[:, D:], rtol=1e-6, atol=1e-9 * scale)
    np.testing.assert_allclose(st.sx, stat[:, :D], rtol=1e-6, atol=1e-9 * scale * cmax)
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
        want = lliks_of(p, p["x"][rows], p["mask"][rows], flags).reshape(B, Lm, p["K"])
        np.testing.assert_array_equal(ll, want)
    assert packed_len(eng) == p["K"] ** 2 + 2 * p["K"] * p["D"] + 1


def test_every_kind_of_entry_is_looked_up(eng):
    """The whole data set of the K = 64 shape in one window: the rows with C, C + 1, +inf, -0.5, 3.7 and the row
    without a present entry are all inside it, and the column of base rate 3000 reaches the table's upper range."""
    p = problem(2)
    c, ok = present(p["x"], p["C"])
    assert c[ok].max() == p["C"] and np.sum(c[ok] > 2500) > 100
    push(eng, p)
    for flags in (0, L.MASK_AS_NAN):
        np.testing.assert_array_equal(eng.loglik([0], T, flags=flags)[0], lliks_of(p, flags=flags))


_fb = {}


def oracle_estep(p, starts, Lm, flags, inner=None):
    """Referee: the NumPy lliks through the oracle's recursions (``OracleEngine.set_lliks`` + USE_HOST_LLIKS), then
    ``poisson_stats`` of its posteriors; the scheme of tests/test_gpu_mcat.py (one recursion per distinct window)."""
    starts = np.asarray(starts, dtype=np.int64)
    B, K = len(starts), p["K"]
    us, inv, cnt = np.unique(starts, return_inverse=True, return_counts=True)
    key = (id(p["x"]), id(p["elog"]), flags & L.MASK_AS_NAN, us.tobytes(), Lm)
    if key not in _fb:
        rows = window_rows(us, Lm)
        ll = lliks_of(p, p["x"][rows], p["mask"][rows], flags).reshape(len(us), Lm, K)
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
    return (A, poisson_stats(p["x"][r], p["mask"][r], p["C"], qu[inv].reshape(B * ln, K)),
            float(res["local_lb"][inv].sum()))


@pytest.mark.parametrize("B,Lm", [(6, 37), (192, 16)], ids=["log", "scaled"])
@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_estep_against_the_oracle(eng, i, B, Lm):
    p = problem(i)
    push(eng, p)
    cmax = max_count(p)
    # (24 distinct windows, each eight times in the large batch: the device sweeps all 192, the referee 24)
    starts = np.tile((np.arange(min(B, 24)) * 29) % (T - Lm + 1), max(1, B // 24))
    assert len(starts) == B
    for flags in (0, L.TRANS_WRAP, L.TRANS_WRAP | L.MASK_AS_NAN):
        st = eng.estep(starts, Lm, flags=flags)
        want = oracle_estep(p, starts, Lm, flags)
        if flags == 0:      # the referee's posteriors are soft: the statistics compare more than one-hot rows
            q = next(iter(_fb.values()))["var_x"].reshape(-1, p["K"])
            assert np.mean(q.max(1) < 0.99) >= 0.1
        check_stats(st, *want, scale=B * Lm, cmax=cmax)
    inner = (5, Lm - 9)
    st = eng.estep(starts, Lm, flags=L.TRANS_WRAP, inner=inner)
    check_stats(st, *oracle_estep(p, starts, Lm, L.TRANS_WRAP, inner), scale=B * Lm, cmax=cmax)


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_suffstats_row_count_edges_and_reproducibility(eng, i):
    p = problem(i)
    push(eng, p)
    K = p["K"]
    cmax = max_count(p)
    rng = np.random.default_rng(7 + i)
    # 1, 3, 4, 5, 63, 64, 65 rows (65: a second chunk of the count GEMM), 600 rows
    for B, Lm in [(1, 1), (3, 1), (2, 2), (1, 5), (9, 7), (1, 64), (5, 13), (3, 200)]:
        starts = (np.arange(B) * 97 + 11) % (T - Lm + 1)
        q = rng.dirichlet(np.ones(K), size=(B, Lm))
        q[rng.random((B, Lm)) < 0.2] = 0.0
        rows = window_rows(starts, Lm)
        a = eng.suffstats(starts, Lm, q, flags=0)
        b = eng.suffstats(starts, Lm, q, flags=0)
        np.testing.assert_array_equal(a.buf, b.buf)
        A = sum(tran_batch(q[w]) for w in range(B))
        check_stats(a, A, poisson_stats(p["x"][rows], p["mask"][rows], p["C"], q.reshape(B * Lm, K)), None, B * Lm, cmax)
        assert a.lb[0] == 0.0


@pytest.mark.parametrize("i", range(6), ids=IDS)
def test_suffstats_ignores_posteriors_of_rows_that_do_not_count(eng, i):
    """A masked row and a row without a present entry add nothing, whatever the caller left in their posterior
    rows: NaN and Inf there stay out of the statistics, which do not change by a bit."""
    p = problem(i)
    push(eng, p)
    K, B, Lm = p["K"], 4, 175
    starts = np.array([0, 175, 350, 525])
    rows = window_rows(starts, Lm)
    _, ok = present(p["x"][rows], p["C"])
    dead = p["mask"][rows] | ~ok.any(1)
    assert dead.sum() >= 5 and (~ok.any(1) & ~p["mask"][rows]).any() and p["mask"][rows].any()
    q = np.random.default_rng(50 + i).dirichlet(np.ones(K), size=B * Lm)
    clean = q.copy()
    clean[dead] = 0.0
    q[dead] = np.where(np.arange(dead.sum())[:, None] % 2 == 0, np.nan, np.inf)
    st = eng.suffstats(starts, Lm, q.reshape(B, Lm, K), flags=0)
    assert np.all(np.isfinite(st.flat))
    ref = eng.suffstats(starts, Lm, clean.reshape(B, Lm, K), flags=0)
    np.testing.assert_array_equal(st.flat, ref.flat)
    # (A_raw pairs every row with the next, whatever the mask says: the NaN rows reach it, so it is not compared)
    check_stats(st, st.A_raw, poisson_stats(p["x"][rows], p["mask"][rows], p["C"], clean), None, B * Lm, max_count(p))


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_estep_sequences_and_subset(eng, i):
    p, off, Ts = seq_problem(i)
    cmax = max_count(p)
    push(eng, p)
    per = []
    for s, ln in enumerate(LENGTHS):
        a = int(off[s])
        r = eng.forward_backward([a], ln, flags=0, want=("var_x", "local_lb"))
        q = r["var_x"][0]
        per.append((tran_batch(q), poisson_stats(p["x"][a:a + ln], p["mask"][a:a + ln], p["C"], q),
                    float(r["local_lb"][0]), q[0].copy()))
    eng.set_sequences(LENGTHS)
    st, seq_lb, q0 = eng.estep_sequences(flags=0)
    check_stats(st, sum(x[0] for x in per), sum(x[1] for x in per), sum(x[2] for x in per), Ts, cmax)
    np.testing.assert_allclose(seq_lb, [x[2] for x in per], rtol=1e-10)
    np.testing.assert_allclose(q0, sum(x[3] for x in per), rtol=1e-6, atol=1e-9)
    idx = (4, 0, 4)
    st, seq_lb, q0 = eng.estep_sequence_subset(idx, flags=0)
    check_stats(st, sum(per[s][0] for s in idx), sum(per[s][1] for s in idx), sum(per[s][2] for s in idx),
                sum(LENGTHS[s] for s in idx), cmax)
    np.testing.assert_allclose(seq_lb, [per[s][2] for s in idx], rtol=1e-10)


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_viterbi_sequences_equals_numpy_on_its_own_lliks(eng, i):
    p, off, Ts = seq_problem(i)
    push(eng, p)
    eng.set_sequences(LENGTHS)
    z, score = eng.viterbi_sequences(flags=L.MASK_AS_NAN)
    ll = eng.read_rows("lliks", 0, Ts)
    np.testing.assert_array_equal(ll, lliks_of(p, flags=L.MASK_AS_NAN))
    for s in range(len(LENGTHS)):
        a, b = int(off[s]), int(off[s + 1])
        zr, sr = viterbi_numpy(ll[a:b], p["mod_init"], p["ltran"])
        np.testing.assert_array_equal(z[a:b], zr)
        assert score[s] == sr


@pytest.mark.parametrize("i", range(5), ids=IDS[:5])
def test_ffbs_sequences_paths(eng, i):
    p, off, Ts = seq_problem(i)
    K, logA = p["K"], p["ltran"]
    la_ref, u, z_np, _ = H.ffbs_reference(i)
    assert near_boundary_sequences(z_np, la_ref, logA, u, off) == 0         # CPU first
    push(eng, p)
    eng.set_sequences(LENGTHS)
    z, la = eng.ffbs_sequences(logA, n_draws=H.FFBS_DRAWS, uniforms=u, want_lalpha=True)
    assert z.shape == (H.FFBS_DRAWS, Ts) and la.shape == (Ts, K)
    assert check_paths_sequences(z, la, logA, u, off) <= 1


def test_grow_windows_products_equals_literal(eng):
    p, Tg = H.grow_case()
    centers, rule = H.GROW_CENTERS, H.GROW_RULE
    ll = lliks_of(p)
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
    """A count matrix uploaded under the NIW family is centred; the Poisson family that follows must see the exact
    counts again, and a Gaussian family after it its centred copy."""
    p = problem(0)
    K, D = p["K"], p["D"]
    c, ok = present(p["x"], p["C"])
    x = np.where(ok, np.minimum(c, 50), 1).astype(np.float64)        # (finite rows: the NIW family evaluates them)
    mask = p["mask"].copy()
    # entries that only the count-preserving way back keeps right, all inside the windows below: after centring and
    # un-centring a 3.7 must still count as 3 and a -0.5 stay absent (plain rounding gives 4 and a present 0); a NaN
    # (on a masked row: the NIW family does not evaluate it) stays a NaN
    x[5, 0], x[7, 1], x[104, 1], x[510, 0] = 3.7, -0.5, 3.7, -0.5
    x[9, 0] = np.nan
    mask[9] = True
    mask[[5, 7, 104, 510]] = False
    p = dict(p, x=x, mask=mask)
    rng = np.random.default_rng(3)
    niw = (rng.normal(size=(K, D)) + 1.0, np.stack([np.eye(D) * 2.0] * K), np.ones(K), np.full(K, D + 3.0))
    starts, Lm = np.array([0, 99, 500]), 37
    rows = window_rows(starts, Lm)
    want = lliks_of(p, x[rows], mask[rows], 0).reshape(3, Lm, K)
    _, okw = present(x[rows], p["C"])
    assert (~okw).sum() == 3                                         # the two -0.5 and the NaN, nothing else
    eng.set_globals(p["mod_init"], p["ltran"])
    eng.set_emission_niw(*niw)
    eng.set_obs(x, mask)
    assert np.any(eng.get_shift() != 0.0)                            # the copy is centred
    ll_niw = eng.loglik(starts, Lm, flags=L.MASK_AS_NAN)
    assert packed_len(eng) == K * K + K * D + K + K * D * D + 1
    for _ in range(2):
        eng.set_emission_poisson(p["elog"], p["erate"], p["C"])
        assert packed_len(eng) == K * K + 2 * K * D + 1
        np.testing.assert_array_equal(eng.loglik(starts, Lm), want)
        st = eng.estep(starts, Lm, flags=0)
        check_stats(st, *oracle_estep(p, starts, Lm, 0), scale=3 * Lm, cmax=50.0)
        eng.set_emission_niw(*niw)
        assert packed_len(eng) == K * K + K * D + K + K * D * D + 1
        np.testing.assert_allclose(eng.loglik(starts, Lm, flags=L.MASK_AS_NAN), ll_niw, rtol=1e-9, atol=1e-9)


def test_another_family_after_poisson_on_one_engine(eng):
    """Every other setter ends the family, in the library and in the engine object: the statistics that come back
    after a switch have the new family's length and views (a stale Poisson length would be too short for them)."""
    from pysvihmm_amd.engine import PackedMCatStats, PackedPoissonStats
    p = problem(0)
    K, D = p["K"], p["D"]
    push(eng, p)
    starts, Lm = np.array([0, 200]), 30
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedPoissonStats and st.buf.size == packed_len(eng) == K * K + 2 * K * D + 1
    Vs = (10, 10)                                                    # F = 20 > 2 D = 4
    tabs = [np.log(np.full((K, v), 1.0 / v)) for v in Vs]
    eng.set_emission_mcat(tabs)
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedMCatStats and st.buf.size == packed_len(eng) == K * K + K * sum(Vs) + 1
    assert eng.read_packed().buf.size == packed_len(eng) and eng.export_packed().size == packed_len(eng)
    eng.set_emission_cat(tabs[0])
    eng.set_obs(np.ascontiguousarray(np.nan_to_num(p["x"][:, :1], nan=0.0, posinf=0.0) % Vs[0]), p["mask"])   # symbols in range
    assert eng.estep(starts, Lm, flags=0).buf.size == packed_len(eng) == K * K + K * Vs[0] + 1
    eng.set_obs(p["x"], p["mask"])
    eng.set_emission_poisson(p["elog"], p["erate"], p["C"])
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedPoissonStats and st.buf.size == packed_len(eng) == K * K + 2 * K * D + 1


def test_packed_round_trip(eng):
    p = problem(3)
    push(eng, p)
    starts = np.arange(4) * 50
    st = eng.estep(starts, 40, flags=L.TRANS_WRAP)
    buf = st.buf.copy()
    wire = eng.export_packed()
    np.testing.assert_array_equal(wire, buf)                         # the statistics carry no coordinates
    eng.import_packed(np.zeros_like(wire))
    assert not np.any(eng.read_packed().buf)
    eng.import_packed(wire)
    np.testing.assert_array_equal(eng.read_packed().buf, buf)


def test_failures_leave_the_handle_usable(eng):
    p = problem(0)
    push(eng, p)
    K, D = p["K"], p["D"]
    starts = np.array([3, 200])
    want = eng.loglik(starts, 20)
    lib, h = eng._lib, eng._h

    def call(K_, D_, elog, erate, logfact, C_, msg):
        arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (elog, erate, logfact)]
        with pytest.raises(RuntimeError, match="^" + re.escape("svihmm_set_emission_poisson failed: "
                                                               "svihmm_set_emission_poisson: ") + ".*" + msg):
            L.check(lib.svihmm_set_emission_poisson(h, K_, D_, L.dptr(arr[0]), L.dptr(arr[1]), L.dptr(arr[2]), C_),
                    "svihmm_set_emission_poisson")
        np.testing.assert_array_equal(eng.loglik(starts, 20), want)  # the family set before is still in force
    el, er, lf, Cc = p["elog"], p["erate"], p["logfact"], p["C"]
    call(K, D, None, er, lf, Cc, "NULL")
    call(K, D, el, None, lf, Cc, "NULL")
    call(K, D, el, er, None, Cc, "NULL")
    call(0, D, el, er, lf, Cc, "K = 0")
    call(257, D, np.zeros((257, D)), np.zeros((257, D)), lf, Cc, "K = 257")
    call(K, 0, el, er, lf, Cc, "D = 0")
    big = np.zeros((K, L.POISSON_MAX_D + 1))
    call(K, L.POISSON_MAX_D + 1, big, big, lf, Cc, "SVIHMM_POISSON_MAX_D")
    call(K, D, el, er, lf, -1, "C = -1")
    call(K, D, el, er, lf, L.POISSON_MAX_COUNT + 1, "SVIHMM_POISSON_MAX_COUNT")
    for bad in (np.nan, np.inf, -np.inf):
        t = el.copy()
        t[1, 1] = bad
        call(K, D, t, er, lf, Cc, re.escape("elog[1][1] is not finite"))
        t = er.copy()
        t[2, 0] = bad
        call(K, D, el, t, lf, Cc, re.escape("erate[2][0] is not finite"))
        t = lf.copy()
        t[17] = bad
        call(K, D, el, er, t, Cc, re.escape("logfact[17] is not finite"))
    # resident observations of another width: refused at the first E-step-type call, before any device work
    eng.set_obs(np.zeros((50, 3)))
    for fn in (lambda: eng.loglik([0], 20), lambda: eng.estep([0], 20), lambda: eng.viterbi([0], 20)):
        with pytest.raises(RuntimeError, match="svihmm_set_emission_poisson: the family has D = 2 count columns, the "
                                               "resident observations have 3"):
            fn()
    eng.set_obs(p["x"], p["mask"])
    np.testing.assert_array_equal(eng.loglik(starts, 20), want)


def test_refusals(eng):
    p = problem(0)
    push(eng, p)
    with pytest.raises(RuntimeError, match="svihmm_pred_logprob: NIW emission only"):
        eng.pred_logprob([0, 40], 30)
    with pytest.raises(RuntimeError, match="svihmm_svi_iteration: the resident SVI loop does not take the Poisson"):
        eng.svi_iteration(0, [0, 40], 2, 30, L.TRANS_WRAP, 0.5, 1.0, 1.0)
    np.testing.assert_array_equal(eng.loglik([0], 20)[0], lliks_of(p, p["x"][:20], None, 0))


def test_fp32_mode_is_not_taken(eng):
    from pysvihmm_amd.engine import HipEngine
    p = problem(2)
    B, Lm = 192, 16
    starts = (np.arange(B) * 13) % (T - Lm + 1)
    push(eng, p)
    want = eng.estep(starts, Lm, flags=L.TRANS_WRAP).buf.copy()
    e = HipEngine(0)
    try:
        e.set_precision("f32")
        push(e, p)
        st = e.estep(starts, Lm, flags=L.TRANS_WRAP)
        assert e.precision() == ("f32", False)
        np.testing.assert_array_equal(st.buf, want)
    finally:
        e.close()
