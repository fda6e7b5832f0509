"""svihmm_set_emission_pgauss on the MI355X: D real-valued columns, single entries may be missing.

The lookup (k_emission_pgauss) is held to the contract's loop bit for bit; the statistics (k_stats_columns, a GEMM on
v_mfma_f64_16x16x4_f64 whose A operand is r * r, r or one, r = x - origin[d]) to the project's tolerances for summed
statistics (tests/test_gpu_poisson.py): A_raw and n rtol 1e-6 with atol 1e-9 x (rows of the batch), sx the same with
atol additionally x the largest |r| of the data set, sxx x its square (the scales of their summands), lb rtol 1e-10.
Shapes (tests/pgauss_helpers.py): (3, 1), (16, 5), (64, 21), (65, 22), (17, 43), (256, 33), (64, 128): every branch of
the two kernels.  Every data set has means about 1e3, about 10 % NaN entries, +-Inf, 1e308 and -1e200 sentinels, one
column without a present entry (D > 1), rows without a present entry and masked rows."""
import re

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from tests import pgauss_helpers as H
from tests.grow_helpers import grow_batch, grow_direct
from tests.pgauss_helpers import IDS, LENGTHS, T, lliks_of, pgauss_stats, present, problem, seq_problem, window_rows
from tests.viterbi_helpers import viterbi_numpy

pytestmark = pytest.mark.gpu
N = len(IDS)
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def push(e, p, x=None, mask=None):
    e.set_emission_pgauss(p["mu"], p["hprec"], p["cst"], p["origin"])
    e.set_obs(p["x"] if x is None else x, p["mask"] if mask is None else mask)
    e.set_globals(p["mod_init"], p["ltran"])


def packed_len(e):
    return int(e._lib.svihmm_packed_len(e._h))


def tran_batch(q):
    return q[:-1].T.dot(q[1:]) if len(q) > 1 else np.zeros((q.shape[1], q.shape[1]))


def rmax_of(p):
    return H.residual_scale(p["x"], p["mask"], p["origin"])


def check_stats(st, A, stat, lb, scale, rmax):
    D = st.D
    np.testing.assert_allclose(st.A_raw, A, rtol=1e-6, atol=1e-9 * scale)
    np.testing.assert_allclose(st.n, stat[:, 2 * D:], rtol=1e-6, atol=1e-9 * scale)
    np.testing.assert_allclose(st.sx, stat[:, D:2 * D], rtol=1e-6, atol=1e-9 * scale * rmax)
    np.testing.assert_allclose(st.sxx, stat[:, :D], rtol=1e-6, atol=1e-9 * scale * rmax * rmax)
    if lb is not None:
        np.testing.assert_allclose(st.lb[0], lb, rtol=1e-10)


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_loglik_is_the_contract_loop_bit_for_bit(eng, i):
    p = problem(i)
    push(eng, p)
    assert not np.any(eng.get_shift())                               # uploaded under the family: not centred
    B, Lm = 5, 37          # (37 rows: a partial block of 32 in every workgroup's range)
    starts = (np.arange(B) * 131) % (T - Lm + 1)
    rows = window_rows(starts, Lm)
    for flags in (0, L.MASK_AS_NAN):
        ll = eng.loglik(starts, Lm, flags=flags)
        want = lliks_of(p, p["x"][rows], p["mask"][rows], flags).reshape(B, Lm, p["K"])
        np.testing.assert_array_equal(ll, want)
    for flags in (0, L.MASK_AS_NAN):                                 # the whole data set as one window
        np.testing.assert_array_equal(eng.loglik([0], T, flags=flags)[0], lliks_of(p, flags=flags))
    assert packed_len(eng) == p["K"] ** 2 + 3 * p["K"] * p["D"] + 1


@pytest.mark.parametrize("i", [1, 3, 5], ids=[IDS[1], IDS[3], IDS[5]])
def test_every_kind_of_entry_is_looked_up(eng, i):
    """NaN, +-Inf, +-1e150 exactly (absent), the doubles just inside the bound (present: squares near 1e300), -0.0
    and 0.0 (present), 1e308 and -1e200 (absent), alone in a row and beside ordinary values."""
    p = problem(i)
    K, D = p["K"], p["D"]
    inside = np.nextafter(1e150, 0.0)
    kinds = np.array([np.nan, np.inf, -np.inf, 1e150, -1e150, inside, -inside, -0.0, 0.0, 1e308, -1e200, 1e3])
    want_ok = [False, False, False, False, False, True, True, True, True, False, False, True]
    assert present(kinds[None, :]).tolist() == [want_ok]
    rng = np.random.default_rng(11)
    n = 3 * len(kinds) * 2 + 5
    x = p["means"][rng.integers(0, K, size=n)] + p["sig"][None, :] * rng.normal(size=(n, D))
    for j, v in enumerate(kinds):
        x[2 * j] = np.nan
        x[2 * j, j % D] = v                                          # alone in its row
        x[2 * j + 1, (j + 1) % D] = v                                # beside ordinary values
        x[2 * len(kinds) + j, :] = v                                 # a whole row of it
    mask = np.zeros(n, bool)
    mask[-2:] = True
    eng.set_emission_pgauss(p["mu"], p["hprec"], p["cst"], p["origin"])
    eng.set_obs(x, mask)
    eng.set_globals(p["mod_init"], p["ltran"])
    for flags in (0, L.MASK_AS_NAN):
        want = H.pgauss_lliks(x, mask, p["mu"], p["hprec"], p["cst"], flags)
        assert np.all(np.isfinite(want)) and want.min() < -1e290
        got = eng.loglik([0], n, flags=flags)[0]
        np.testing.assert_array_equal(got, want)
        dead = ~present(x).any(1) | (mask if flags else False)
        assert dead.sum() >= 6 and not np.any(got[dead]) and not np.any(np.signbit(got[dead]))


_fb = {}


def oracle_estep(p, starts, Lm, flags, inner=None):
    """Referee: the NumPy lliks through the oracle's recursions (``OracleEngine.set_lliks`` + USE_HOST_LLIKS), then
    ``pgauss_stats`` of its posteriors (one recursion per distinct window)."""
    starts = np.asarray(starts, dtype=np.int64)
    B, K = len(starts), p["K"]
    us, inv, cnt = np.unique(starts, return_inverse=True, return_counts=True)
    key = (id(p["x"]), id(p["mu"]), flags & L.MASK_AS_NAN, us.tobytes(), Lm)
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
    return (A, pgauss_stats(p["x"][r], p["mask"][r], p["origin"], qu[inv].reshape(B * ln, K)),
            float(res["local_lb"][inv].sum()))


@pytest.mark.parametrize("B,Lm", [(1, 70), (24, 37), (192, 16)], ids=["B1", "B24", "B192"])
@pytest.mark.parametrize("i", range(N - 1), ids=IDS[:-1])
def test_estep_against_the_oracle(eng, i, B, Lm):
    p = problem(i)
    push(eng, p)
    rmax = rmax_of(p)
    # (24 distinct windows, each eight times in the large batch: the device sweeps all 192, the referee 24)
    starts = np.tile((np.arange(min(B, 24)) * 29 + 3) % (T - Lm + 1), max(1, B // 24))
    assert len(starts) == B
    inner = (5, Lm - 9)
    # (the referee keeps one recursion: the three unmasked cases share it)
    for flags, inn in ((0, None), (L.TRANS_WRAP, None), (L.TRANS_WRAP, inner), (L.TRANS_WRAP | L.MASK_AS_NAN, None)):
        st = eng.estep(starts, Lm, flags=flags, inner=inn)
        check_stats(st, *oracle_estep(p, starts, Lm, flags, inn), scale=B * Lm, rmax=rmax)
        assert np.array_equal(st.origin, p["origin"])


def test_estep_at_the_widest_shape(eng):
    """(64, 128): two feature groups and a stage of 106 KB of LDS, one batch."""
    p = problem(N - 1)
    push(eng, p)
    starts, Lm = (np.arange(24) * 27) % (T - 37 + 1), 37
    st = eng.estep(starts, Lm, flags=L.TRANS_WRAP)
    check_stats(st, *oracle_estep(p, starts, Lm, L.TRANS_WRAP), scale=24 * Lm, rmax=rmax_of(p))


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_suffstats_row_count_edges_and_reproducibility(eng, i):
    p = problem(i)
    push(eng, p)
    K = p["K"]
    rmax = rmax_of(p)
    rng = np.random.default_rng(7 + i)
    # 1, 3, 4, 5, 63, 64, 65 rows (65: a second stage of the GEMM, partial), 600 rows
    for B, Lm in [(1, 1), (3, 1), (2, 2), (1, 5), (9, 7), (1, 64), (5, 13), (3, 200)]:
        starts = (np.arange(B) * 97 + 11) % (T - Lm + 1)
        q = rng.dirichlet(np.ones(K), size=(B, Lm))
        q[rng.random((B, Lm)) < 0.2] = 0.0
        rows = window_rows(starts, Lm)
        a = eng.suffstats(starts, Lm, q, flags=0)
        b = eng.suffstats(starts, Lm, q, flags=0)
        np.testing.assert_array_equal(a.buf, b.buf)
        A = sum(tran_batch(q[w]) for w in range(B))
        check_stats(a, A, pgauss_stats(p["x"][rows], p["mask"][rows], p["origin"], q.reshape(B * Lm, K)), None,
                    B * Lm, rmax)
        assert a.lb[0] == 0.0
        if p["D"] > 1:                   # the column without a present entry collects nothing
            d = p["D"] // 2
            assert not np.any(a.n[:, d]) and not np.any(a.sx[:, d]) and not np.any(a.sxx[:, d])


@pytest.mark.parametrize("i", range(N), ids=IDS)
def test_suffstats_ignores_posteriors_of_rows_that_do_not_count(eng, i):
    """A masked row and a row without a present entry add nothing, whatever the caller left in their posterior
    rows: NaN and Inf there stay out of the statistics, which do not change by a bit."""
    p = problem(i)
    push(eng, p)
    K, B, Lm = p["K"], 4, 175
    starts = np.array([0, 175, 350, 525])
    rows = window_rows(starts, Lm)
    ok = present(p["x"][rows])
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
    check_stats(st, st.A_raw, pgauss_stats(p["x"][rows], p["mask"][rows], p["origin"], clean), None, B * Lm, rmax_of(p))


@pytest.mark.parametrize("i", range(N - 1), ids=IDS[:-1])
def test_estep_sequences_and_subset(eng, i):
    p, off, Ts = seq_problem(i)
    rmax = rmax_of(p)
    push(eng, p)
    per = []
    for s, ln in enumerate(LENGTHS):
        a = int(off[s])
        r = eng.forward_backward([a], ln, flags=0, want=("var_x", "local_lb"))
        q = r["var_x"][0]
        per.append((tran_batch(q), pgauss_stats(p["x"][a:a + ln], p["mask"][a:a + ln], p["origin"], q),
                    float(r["local_lb"][0]), q[0].copy()))
    eng.set_sequences(LENGTHS)
    st, seq_lb, q0 = eng.estep_sequences(flags=0)
    check_stats(st, sum(x[0] for x in per), sum(x[1] for x in per), sum(x[2] for x in per), Ts, rmax)
    np.testing.assert_allclose(seq_lb, [x[2] for x in per], rtol=1e-10)
    np.testing.assert_allclose(q0, sum(x[3] for x in per), rtol=1e-6, atol=1e-9)
    idx = (4, 0, 4)
    st, seq_lb, q0 = eng.estep_sequence_subset(idx, flags=0)
    check_stats(st, sum(per[s][0] for s in idx), sum(per[s][1] for s in idx), sum(per[s][2] for s in idx),
                sum(LENGTHS[s] for s in idx), rmax)
    np.testing.assert_allclose(seq_lb, [per[s][2] for s in idx], rtol=1e-10)


@pytest.mark.parametrize("i", range(N - 1), ids=IDS[:-1])
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


def test_ffbs_sequences_smoke(eng):
    p, off, Ts = seq_problem(1)
    push(eng, p)
    eng.set_sequences(LENGTHS)
    u = np.random.default_rng(0).random((3, Ts))
    z, la = eng.ffbs_sequences(p["ltran"], n_draws=3, uniforms=u, want_lalpha=True)
    assert z.shape == (3, Ts) and la.shape == (Ts, p["K"]) and z.min() >= 0 and z.max() < p["K"]
    assert np.all(np.isfinite(la)) and len(np.unique(z)) > 1


def test_grow_windows_products_equals_literal(eng):
    p, Tg = H.grow_case()
    centers, rule = H.GROW_CENTERS, H.GROW_RULE
    compared, ll = H.grow_compared(p, Tg)
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
    """Rows uploaded under the NIW family are centred; the family that follows gets them back by the plain shift --
    to rounding, so its lliks agree with the host's to rtol 1e-9 --, a fresh upload under the family is bit-exact, and
    a Gaussian family after it centres again."""
    p = dict(problem(1))
    K, D = p["K"], p["D"]
    rng = np.random.default_rng(5)
    x = p["means"][rng.integers(0, K, size=T)] + p["sig"][None, :] * rng.normal(size=(T, D))     # (finite rows: the NIW family evaluates them)
    mask = p["mask"].copy()
    x[9, 0] = np.nan                     # (on a masked row: the NIW family does not evaluate it) stays a NaN
    mask[9] = True
    p.update(x=x, mask=mask, origin=H.data_origin(x))
    niw = (p["means"].copy(), np.stack([np.diag(p["sig"] ** 2 * (D + 3.0))] * K), np.ones(K), np.full(K, D + 3.0))
    starts, Lm = np.array([0, 99, 500]), 37
    rows = window_rows(starts, Lm)
    want = lliks_of(p, x[rows], mask[rows], 0).reshape(3, Lm, K)
    eng.set_globals(p["mod_init"], p["ltran"])
    eng.set_emission_niw(*niw)
    eng.set_obs(x, mask)
    assert np.any(eng.get_shift() != 0.0)                            # the copy is centred
    ll_niw = eng.loglik(starts, Lm, flags=L.MASK_AS_NAN)
    assert packed_len(eng) == K * K + K * D + K + K * D * D + 1
    for _ in range(2):
        eng.set_emission_pgauss(p["mu"], p["hprec"], p["cst"], p["origin"])
        assert packed_len(eng) == K * K + 3 * K * D + 1
        got = eng.loglik(starts, Lm)
        assert not np.any(eng.get_shift())
        np.testing.assert_allclose(got, want, rtol=1e-9)
        st = eng.estep(starts, Lm, flags=0)
        check_stats(st, *oracle_estep(p, starts, Lm, 0), scale=3 * Lm, rmax=H.residual_scale(x, mask, p["origin"]))
        eng.set_emission_niw(*niw)
        assert packed_len(eng) == K * K + K * D + K + K * D * D + 1
        np.testing.assert_allclose(eng.loglik(starts, Lm, flags=L.MASK_AS_NAN), ll_niw, rtol=1e-9, atol=1e-9)
    eng.set_emission_pgauss(p["mu"], p["hprec"], p["cst"], p["origin"])
    eng.set_obs(x, mask)                                             # a fresh upload under the family: the caller's bits
    np.testing.assert_array_equal(eng.loglik(starts, Lm), want)


def test_another_family_after_pgauss_on_one_engine(eng):
    from pysvihmm_amd.engine import PackedDiagStats, PackedGaussTrackStats, PackedPoissonStats
    p = problem(1)
    K, D = p["K"], p["D"]
    push(eng, p)
    starts, Lm = np.array([0, 200]), 30
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedGaussTrackStats and st.buf.size == packed_len(eng) == K * K + 3 * K * D + 1
    eng.set_emission_poisson(np.zeros((K, D)), np.ones((K, D)), 15)
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedPoissonStats and st.buf.size == packed_len(eng) == K * K + 2 * K * D + 1
    assert eng.read_packed().buf.size == packed_len(eng) and eng.export_packed().size == packed_len(eng)
    push(eng, p)
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedGaussTrackStats and st.buf.size == packed_len(eng)
    eng.set_obs(np.nan_to_num(p["x"], nan=1e3, posinf=1e3, neginf=1e3).clip(-1e4, 1e4), p["mask"])
    eng.set_emission_diag(p["means"], np.ones((K, D)), np.full((K, D), 3.0), np.full((K, D), 3.0) * p["sig"][None, :] ** 2)
    st = eng.estep(starts, Lm, flags=0)
    assert type(st) is PackedDiagStats and st.buf.size == packed_len(eng) == K * K + 2 * K * D + K + 1


def test_packed_round_trip(eng):
    p = problem(3)
    push(eng, p)
    starts = np.arange(4) * 50
    st = eng.estep(starts, 40, flags=L.TRANS_WRAP)
    buf = st.buf.copy()
    wire = eng.export_packed()
    np.testing.assert_array_equal(wire, buf)                         # the statistics carry only the caller's origin
    eng.import_packed(np.zeros_like(wire))
    assert not np.any(eng.read_packed().buf)
    eng.import_packed(wire)
    np.testing.assert_array_equal(eng.read_packed().buf, buf)


def test_failures_leave_the_handle_usable(eng):
    p = problem(1)
    push(eng, p)
    K, D = p["K"], p["D"]
    starts = np.array([3, 200])
    want = eng.loglik(starts, 20)
    lib, h = eng._lib, eng._h

    def call(K_, D_, mu, hprec, cst, origin, msg):
        arr = [None if a is None else np.ascontiguousarray(a, dtype=np.float64) for a in (mu, hprec, cst, origin)]
        with pytest.raises(RuntimeError, match="^" + re.escape("svihmm_set_emission_pgauss failed: "
                                                               "svihmm_set_emission_pgauss: ") + ".*" + msg):
            L.check(lib.svihmm_set_emission_pgauss(h, K_, D_, *[L.dptr(a) for a in arr]), "svihmm_set_emission_pgauss")
        np.testing.assert_array_equal(eng.loglik(starts, 20), want)  # the family set before is still in force
    mu, hp, cs, o = p["mu"], p["hprec"], p["cst"], p["origin"]
    call(K, D, None, hp, cs, o, "NULL")
    call(K, D, mu, None, cs, o, "NULL")
    call(K, D, mu, hp, None, o, "NULL")
    call(K, D, mu, hp, cs, None, "NULL")
    call(0, D, mu, hp, cs, o, "K = 0")
    z = np.zeros((257, D))
    call(257, D, z, z, z, o, "K = 257")
    call(K, 0, mu, hp, cs, o, "D = 0")
    big = np.zeros((K, L.PGAUSS_MAX_D + 1))
    call(K, L.PGAUSS_MAX_D + 1, big, big, big, np.zeros(L.PGAUSS_MAX_D + 1), "SVIHMM_PGAUSS_MAX_D")
    for bad in (np.nan, np.inf, -np.inf):
        for j, name in enumerate(("mu", "hprec", "cst")):
            t = [mu, hp, cs]
            t[j] = t[j].copy()
            t[j][1, 2] = bad
            call(K, D, t[0], t[1], t[2], o, re.escape(name + "[1][2] is not finite"))
        t = o.copy()
        t[3] = bad
        call(K, D, mu, hp, cs, t, re.escape("origin[3] is not finite"))
    t = hp.copy()
    t[2, 0] = 1e-300
    call(K, D, mu, t, cs, o, re.escape("hprec[2][0] is positive"))
    for v in (1e150, -1e150, 1e200):
        t = mu.copy()
        t[0, 4] = v
        call(K, D, t, hp, cs, o, re.escape("|mu[0][4]| is at or above SVIHMM_PGAUSS_ABSENT"))
        t = o.copy()
        t[1] = v
        call(K, D, mu, hp, cs, t, re.escape("|origin[1]| is at or above SVIHMM_PGAUSS_ABSENT"))
    # resident observations of another width: refused at the first E-step-type call, before any device work
    eng.set_obs(np.zeros((50, 3)))
    for fn in (lambda: eng.loglik([0], 20), lambda: eng.estep([0], 20), lambda: eng.viterbi([0], 20)):
        with pytest.raises(RuntimeError, match="svihmm_set_emission_pgauss: the family has D = 5 columns, the "
                                               "resident observations have 3"):
            fn()
    eng.set_obs(p["x"], p["mask"])
    np.testing.assert_array_equal(eng.loglik(starts, 20), want)


def test_refusals(eng):
    p = problem(0)
    push(eng, p)
    with pytest.raises(RuntimeError, match="svihmm_pred_logprob: NIW emission only"):
        eng.pred_logprob([0, 40], 30)
    with pytest.raises(RuntimeError, match="svihmm_svi_iteration: the resident SVI loop does not take the family of "
                                           "svihmm_set_emission_pgauss"):
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


# ---- held-out scores ------------------------------------------------------------------------------------------------
def entry_bound(K, M):
    """|device - NumPy| per entry: the existing bound of tests/test_gpu_heldout.py, 2 (8 M + K + 8) 2^-52, M the largest
    magnitude among the entry's operands."""
    return 2.0 * (8.0 * M + K + 8.0) * ULP


@pytest.mark.parametrize("i", [0, 1, 3, 5], ids=[IDS[0], IDS[1], IDS[3], IDS[5]])
def test_heldout_entries_against_numpy_on_the_same_posterior_bits(eng, i):
    p = problem(i)
    push(eng, p)
    q = eng.forward_backward([0], T, flags=L.MASK_AS_NAN, want=("var_x",))["var_x"][0]
    rows, cols, vals = H.entry_list(p, 3000, seed=77 + i)
    mean, cnt, lp = eng.heldout_entries(rows, cols, vals, resident=False, want_lp=True)
    want, M = H.heldout_entries_numpy(p, q, rows, cols, vals)
    assert np.array_equal(np.isnan(lp), np.isnan(want))
    ok = ~np.isnan(want)
    assert cnt == ok.sum() and 0.9 <= ok.mean() < 1.0
    d = np.abs(lp[ok] - want[ok])
    bound = entry_bound(p["K"], M[ok])
    worst = int(np.argmax(d / bound))
    print("%s: max |d| / bound = %.3g (|d| = %.3g, M = %.3g)" % (IDS[i], (d / bound).max(), d[worst], M[ok][worst]))
    assert np.all(d <= bound)
    assert abs(mean - np.mean(lp[ok])) <= 1e-12 * abs(np.mean(lp[ok]))
    mean2, cnt2, lp2 = eng.heldout_entries(rows, cols, vals, resident=False, want_lp=True)
    assert mean2 == mean and cnt2 == cnt and np.array_equal(lp2, lp, equal_nan=True)
    assert np.array_equal(eng.read_rows("var_x", 0, T), q)           # the held-out call left the posterior alone


@pytest.mark.parametrize("i", [1, 3], ids=[IDS[1], IDS[3]])
def test_heldout_rows_against_the_formula(eng, i):
    p = problem(i)
    push(eng, p)
    q = eng.forward_backward([0], T, flags=L.MASK_AS_NAN, want=("var_x",))["var_x"][0]
    mean, cnt, lp = eng.heldout_rows(want_lp=True)
    ll_true = lliks_of(p, flags=0)
    v = np.log(q + 1e-9) + ll_true
    want = np.where(p["mask"], H.lse_rows(v), np.nan)
    assert np.array_equal(np.isnan(lp), np.isnan(want)) and cnt == p["mask"].sum()
    ok = p["mask"]
    M = np.maximum(np.abs(ll_true).max(1), np.abs(np.log(q + 1e-9)).max(1))[ok]
    assert np.all(np.abs(lp[ok] - want[ok]) <= entry_bound(p["K"], M))
    assert abs(mean - np.mean(want[ok])) <= 1e-12 * abs(np.mean(want[ok]))
