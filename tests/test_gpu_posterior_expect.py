"""svihmm_posterior_expect / svihmm_posterior_expect_entries on the MI355X: posterior expectations of per-state tables
against the posterior rows the last E-step-type call left in HBM (kernels_expect.h), through the C ABI, HipEngine and
the classes (``posterior_expect``, ``reconstruct``, ``impute``).

The kernel tests reach their rows as short chains on host lliks (``SVIHMM_USE_HOST_LLIKS``): the calls do not depend
on the emission family, so no family is set there, and every K from 1 to 256 costs one tiny E-step.  The posterior
rows the references are formed from are the bits ``read_rows("var_x")`` hands out."""
import ctypes as C

import numpy as np
import pytest

from pysvihmm_amd import _lib as L
from pysvihmm_amd import hmmbatchcd, hmmsgd_metaobs
from tests import heldout_helpers as H
from tests import posterior_expect_helpers as P
from tests import test_gpu_heldout as TH
from tests import test_gpu_pgauss_classes as PG

pytestmark = pytest.mark.gpu

ROWS = 257                                   # 9 wave tiles of 32 rows: three workgroups, the last tile one row long
ALL_F = (1, 15, 16, 17, 96, 1024)
DENSE = [(1, ROWS, (1, 17)), (3, ROWS, (1, 17)), (5, ROWS, ALL_F), (64, ROWS, (1, 17)), (65, ROWS, ALL_F),
         (256, ROWS, (1, 17))] + [(5, r, (17,)) for r in (1, 15, 17, 63, 65)]


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def globals_of(K, seed, uniform=False):
    rng = np.random.default_rng(seed)
    if uniform:
        return np.full(K, -np.log(K)), np.full((K, K), -np.log(K))
    a = rng.random((K, K)) + 0.2
    p = rng.random(K) + 0.2
    return np.log(p / p.sum()), np.log(a / a.sum(axis=1)[:, None])


def host_batch(e, ll, seed=1, uniform=False):
    """A batch on host lliks ``ll`` [B, Lm, K]: its var_x rows as the device hands them out."""
    B, Lm, K = ll.shape
    e.set_globals(*globals_of(K, seed, uniform))
    e.set_lliks(ll)
    e.forward_backward(None, Lm, flags=L.USE_HOST_LLIKS, want=(), B=B)
    q = e.read_rows("var_x", 0, B * Lm)
    assert q.shape == (B * Lm, K) and np.all(np.isfinite(q))
    return q


def lliks(B, Lm, K, seed):
    return 2.0 * np.random.default_rng(seed).normal(size=(B, Lm, K))


def table(K, F, seed):
    """Entries about 1e3, mixed signs."""
    rng = np.random.default_rng(seed)
    return 1e3 * rng.normal(size=(K, F)) * rng.choice([-1.0, 1.0], size=(K, F))


_chains = {}


def chain(e, K, rows):
    q = host_batch(e, lliks(1, rows, K, 100 + K + rows))
    _chains.setdefault((K, rows), q)
    assert np.array_equal(q, _chains[(K, rows)])
    return q


# ---- 1. the dense kernel against the extended-precision reference ---------------------------------------------------
@pytest.mark.parametrize("K,rows,Fs", DENSE, ids=["K%d-rows%d" % (k, r) for k, r, _ in DENSE])
def test_dense_against_the_extended_reference(eng, K, rows, Fs):
    """|out - ref| <= K 2^-52 sum_k |var_x[g][k] table[k][f]| per output: derived (any order of K fused or unfused
    multiply-adds stays within gamma_K of that sum), not measured.  Two calls give the same bits."""
    q = chain(eng, K, rows)
    for F in Fs:
        tab = table(K, F, 7 * K + F)
        out = eng.posterior_expect(tab)
        assert out.shape == (rows, F)
        u = P.dense_error_in_bounds(out, q, tab)
        print("FIG dense K=%d F=%d rows=%d: max error %.4f of bound" % (K, F, rows, u))
        assert u <= 1.0
        np.testing.assert_array_equal(eng.posterior_expect(tab), out)
    t1 = table(K, 1, 3)
    out1 = eng.posterior_expect(t1[:, 0])                       # a [K] table counts as F = 1
    assert out1.shape == (rows, 1) and np.array_equal(out1, eng.posterior_expect(t1))
    np.testing.assert_array_equal(eng.read_rows("var_x", 0, rows), q)


def test_a_result_above_the_pass_size_runs_in_several_passes(eng):
    """The device copy of the dense result holds 256 MiB; more rows run pass by pass.  K = 2, F = 1024 and 32768 + 33
    rows: two passes, the second one tile and one row long.  The rows at the start and around the seam against the
    extended reference within the dense bound; every row of both passes against the two-term product in doubles
    (its own error and the kernel's are each at most 2 x 2^-52 (|t0| + |t1|): 5 of that unit in all); and every row
    bit for bit against one-pass calls on the same batch."""
    K, F, per_pass = 2, 1024, (256 << 20) // (1024 * 8)
    rows = per_pass + 33
    ll = lliks(1, rows, K, 77)
    q = host_batch(eng, ll, uniform=True)
    tab = table(K, F, 19)
    out = eng.posterior_expect(tab)
    assert out.shape == (rows, F) and out.nbytes > 256 << 20
    for a, b in ((0, 64), (per_pass - 40, rows)):
        u = P.dense_error_in_bounds(out[a:b], q[a:b], tab)
        print("FIG passes rows %d..%d: max error %.4f of bound" % (a, b, u))
        assert u <= 1.0
    whole = q[:, :1] * tab[0] + q[:, 1:] * tab[1]
    assert np.all(np.abs(out - whole) <= 5 * 2.0 ** -52 * (np.abs(tab[0]) + np.abs(tab[1])))
    np.testing.assert_array_equal(eng.posterior_expect(tab), out)
    # the same batch against 16 and 48 of the table's columns: one pass each (4 and 12 MB).  An output's summation order
    # does not depend on the feature group's width or on the launch, so every row of both passes has these bits.
    np.testing.assert_array_equal(eng.posterior_expect(tab[:, :16]), out[:, :16])
    np.testing.assert_array_equal(eng.posterior_expect(tab[:, 976:]), out[:, 976:])


# ---- 2. bits do not depend on where a row sits in the grid ----------------------------------------------------------
def test_bits_do_not_depend_on_the_grid_position(eng):
    """The same posterior row met in two batches gives the same output bits wherever it sat (tile, wave, lane,
    workgroup).  Stated only for rows whose var_x is bit-equal in both batches, which is checked first: the same
    windows in another order and number (a window's posteriors do not depend on its neighbours in the batch), and one
    window against several windows of another length under uniform transitions, where few or no rows may qualify."""
    K, F, Lm = 5, 17, 33
    tab = table(K, F, 11)
    ll = lliks(6, Lm, K, 5)
    qa = host_batch(eng, ll)
    oa = eng.posterior_expect(tab)
    pick = [5, 0, 3, 3, 2]
    qb = host_batch(eng, ll[pick])
    ob = eng.posterior_expect(tab)
    same = 0
    for i, w in enumerate(pick):
        for t in range(Lm):
            ra, rb = w * Lm + t, i * Lm + t
            if np.array_equal(qa[ra], qb[rb]):
                same += 1
                assert np.array_equal(oa[ra], ob[rb]), (w, t)
    assert same >= Lm                      # at least one whole window kept its posterior bits
    # one window of 48 rows / three windows of 16 rows over the same lliks, uniform transitions
    one = lliks(1, 48, K, 6)
    qc = host_batch(eng, one, uniform=True)
    oc = eng.posterior_expect(tab)
    qd = host_batch(eng, one.reshape(3, 16, K), uniform=True)
    od = eng.posterior_expect(tab)
    also = 0
    for r in range(48):
        if np.array_equal(qc[r], qd[r]):
            also += 1
            assert np.array_equal(oc[r], od[r]), r
    print("FIG grid independence: %d rows bit-equal across window orders, %d of 48 across window lengths" % (same, also))


# ---- 3. the entries kernel: bit for bit the NumPy loop --------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 5, 65, 256])
def test_entries_equal_the_numpy_loop(eng, K):
    F = 17
    q = chain(eng, K, ROWS)
    tab = table(K, F, 13 + K)
    rng = np.random.default_rng(K)
    rows = rng.integers(0, ROWS, size=700)
    cols = rng.integers(0, F, size=700)
    rows[:4], cols[:4] = [0, ROWS - 1, 9, 9], [0, F - 1, 4, 4]                # both ends of [0, F), a duplicate
    out = eng.posterior_expect_entries(tab, rows, cols)
    np.testing.assert_array_equal(out, P.entry_loop(q, tab, rows, cols))
    assert out[2] == out[3]
    np.testing.assert_array_equal(eng.posterior_expect_entries(tab, rows, cols), out)
    one = eng.posterior_expect_entries(tab, [ROWS - 1], [F - 1])
    np.testing.assert_array_equal(one, P.entry_loop(q, tab, [ROWS - 1], [F - 1]))
    none = eng.posterior_expect_entries(tab, [], [])
    assert none.shape == (0,)
    np.testing.assert_array_equal(eng.read_rows("var_x", 0, ROWS), q)


# ---- 4. all four batch kinds ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", H.KINDS)
def test_every_batch_kind_and_nothing_else_changes(eng, kind):
    """Row g of the result belongs to row g of read_rows("var_x") -- a window batch with overlapping windows, the
    whole chain, all sequences, a subset with a repeated sequence -- and the packed statistics, var_x and the held-out
    scores read after the calls carry the bits read before them."""
    cs = H.e2e_case("poisson", 1, kind)
    n = TH.run_kind(eng, cs, kind)
    K = cs["p"]["K"]

    def state():
        packed = eng.read_packed().buf.copy() if kind != "chain" else None
        return (packed, eng.read_rows("var_x", 0, n), eng.heldout_rows(want_lp=True),
                eng.heldout_entries(cs["rows"], cs["cols"], cs["vals"], resident=False, want_lp=True))
    before = state()
    q = before[1]
    tab = table(K, 33, 21)
    out = eng.posterior_expect(tab)
    assert out.shape == (n, 33)
    u = P.dense_error_in_bounds(out, q, tab)
    print("FIG kind %s K=%d rows=%d: max error %.4f of bound" % (kind, K, n, u))
    assert u <= 1.0
    rng = np.random.default_rng(4)
    rows, cols = rng.integers(0, n, size=300), rng.integers(0, 33, size=300)
    rows[0], rows[1] = 0, n - 1
    np.testing.assert_array_equal(eng.posterior_expect_entries(tab, rows, cols), P.entry_loop(q, tab, rows, cols))
    after = state()
    if before[0] is not None:
        np.testing.assert_array_equal(after[0], before[0])
    np.testing.assert_array_equal(after[1], before[1])
    for a, b in ((after[2], before[2]), (after[3], before[3])):
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2], equal_nan=True)
    if kind == "windows":           # a row in two windows appears once per window, each with that window's posterior
        res = cs["res"]
        g1, g2 = np.flatnonzero(res == 30)                    # resident row 30: in the windows from 0 and from 25
        assert (g1, g2) == (30, H.WINDOW_LM + 5)
        np.testing.assert_array_equal(eng.posterior_expect_entries(tab, [g1, g2], [3, 3]),
                                      P.entry_loop(q, tab, [g1, g2], [3, 3]))


# ---- 5. host lliks, and the identity table under allowed-state sets -------------------------------------------------
def test_identity_table_returns_var_x_under_state_sets(eng):
    """Products with 1.0 and sums with 0.0 are exact, so the identity table returns var_x itself -- with allowed-state
    sets in force exactly 0.0 at every forbidden (row, state) pair.  (The batches of tests 1-3 ran on host lliks.)"""
    p = H.problem("poisson", 1)
    K, T = p["K"], H.T
    TH.push(eng, p)
    rng = np.random.default_rng(12)
    allowed = rng.random((T, K)) < 0.6
    allowed[np.arange(T), rng.integers(0, K, size=T)] = True
    eng.set_state_sets(allowed)
    q = eng.forward_backward([0], T, flags=L.MASK_AS_NAN, want=("var_x",))["var_x"][0]
    assert np.all(np.isfinite(q))
    out = eng.posterior_expect(np.eye(K))
    np.testing.assert_array_equal(out, q)
    assert np.all(out[~allowed] == 0.0) and (~allowed).sum() > T
    r, c = np.nonzero(~allowed)
    assert np.all(eng.posterior_expect_entries(np.eye(K), r, c) == 0.0)
    eng.set_state_sets(None)
    # a batch on host lliks next to a family that is set: taken, and correct
    ll = lliks(2, 40, K, 9)
    qh = host_batch(eng, ll)
    tab = table(K, 5, 2)
    assert P.dense_error_in_bounds(eng.posterior_expect(tab), qh, tab) <= 1.0


def test_a_batch_of_the_fp32_mode_is_taken_as_fp64_rows():
    """var_x of a batch that ran in the fp32 format is handed out as doubles (what read_rows returns): the calls take
    it as any other batch, within the same bound on those rows, and the precision report does not move."""
    from pysvihmm_amd.engine import HipEngine
    from tests.helpers import make_problem
    K, D, B, Lm = 5, 3, 7, 40
    pb = make_problem(K, D, 4000, seed=K * 7 + D, miss=0.05, sep=4.0)
    e = HipEngine(0, dtype="f32")
    try:
        e.set_obs(pb["obs"], pb["mask"])
        e.set_globals(pb["mod_init"], pb["ltran"])
        e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        e.estep(np.random.default_rng(B).integers(0, 4000 - Lm + 1, size=B), Lm, flags=L.TRANS_WRAP)
        assert e.precision() == ("f32", True)
        q = e.read_rows("var_x", 0, B * Lm)
        tab = table(K, 17, 5)
        out = e.posterior_expect(tab)
        assert P.dense_error_in_bounds(out, q, tab) <= 1.0
        rows, cols = np.arange(B * Lm) % 97, np.arange(B * Lm) % 17
        np.testing.assert_array_equal(e.posterior_expect_entries(tab, rows, cols), P.entry_loop(q, tab, rows, cols))
        assert e.precision() == ("f32", True)
        np.testing.assert_array_equal(e.read_rows("var_x", 0, B * Lm), q)
    finally:
        e.close()


# ---- 6. refusals ----------------------------------------------------------------------------------------------------
def test_refusals_leave_the_handle_usable(eng):
    K, F, rows = 5, 17, 65
    q = chain(eng, K, rows)
    tab = table(K, F, 31)
    want = eng.posterior_expect(tab)
    lib, h = eng._lib, eng._h
    out = np.empty((rows, F))
    r1, c1 = np.array([3], dtype=np.int64), np.array([2], dtype=np.int32)
    i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
    dense = lambda hh, f, t, o: lib.svihmm_posterior_expect(hh, f, L.dptr(t), L.dptr(o))
    ents = lambda hh, f, t, n, r, c, o: lib.svihmm_posterior_expect_entries(
        hh, f, L.dptr(t), n, None if r is None else L.i64ptr(r), None if c is None else i32(c), L.dptr(o))

    def refused(rc, text):
        assert rc != 0
        assert text in L.last_error(), L.last_error()
    refused(dense(None, F, tab, out), "svihmm_posterior_expect: NULL handle")
    refused(dense(h, F, None, out), "svihmm_posterior_expect: table is NULL")
    refused(dense(h, F, tab, None), "svihmm_posterior_expect: out is NULL")
    refused(dense(h, 0, tab, out), "F = 0 is outside [1, 1024]")
    refused(dense(h, 1025, tab, out), "F = 1025 is outside [1, 1024]")
    refused(ents(None, F, tab, 1, r1, c1, out), "svihmm_posterior_expect_entries: NULL handle")
    refused(ents(h, F, None, 1, r1, c1, out), "svihmm_posterior_expect_entries: table is NULL")
    refused(ents(h, F, tab, 1, r1, c1, None), "svihmm_posterior_expect_entries: out is NULL")
    refused(ents(h, 0, tab, 1, r1, c1, out), "F = 0 is outside [1, 1024]")
    refused(ents(h, F, tab, -1, r1, c1, out), "n = -1 must not be negative")
    refused(ents(h, F, tab, 1, None, c1, out), "row and col must be given when n > 0")
    refused(ents(h, F, tab, 1, r1, None, out), "row and col must be given when n > 0")
    for bad_row in (-1, rows):
        with pytest.raises(RuntimeError, match=r"row\[1\] = %d is outside \[0, nrows = %d\)" % (bad_row, rows)):
            eng.posterior_expect_entries(tab, [0, bad_row], [0, 0])
    for bad_col in (-1, F):
        with pytest.raises(RuntimeError, match=r"col\[2\] = %d is outside \[0, F = %d\)" % (bad_col, F)):
            eng.posterior_expect_entries(tab, [0, 1, 2], [0, 0, bad_col])
    for bad in (np.nan, np.inf):
        t2 = tab.copy()
        t2[3, 9] = bad
        with pytest.raises(RuntimeError, match=r"svihmm_posterior_expect: table\[3\]\[9\] is not finite"):
            eng.posterior_expect(t2)
        with pytest.raises(RuntimeError, match=r"svihmm_posterior_expect_entries: table\[3\]\[9\] is not finite"):
            eng.posterior_expect_entries(t2, [0], [0])
    # still the batch, still the bits
    np.testing.assert_array_equal(eng.posterior_expect(tab), want)
    # a globals' K that is not the batch's
    eng.set_globals(*globals_of(K + 1, 2))
    with pytest.raises(RuntimeError, match=r"the globals' K \(6\) is not the K of the posterior batch held \(5\)"):
        eng.posterior_expect(table(K + 1, F, 1))
    with pytest.raises(RuntimeError, match=r"the globals' K \(6\) is not the K of the posterior batch held \(5\)"):
        eng.posterior_expect_entries(table(K + 1, F, 1), [0], [0])
    # K > 256
    q257 = host_batch(eng, lliks(1, 20, 257, 3))
    assert q257.shape == (20, 257)
    with pytest.raises(RuntimeError, match="svihmm_posterior_expect: K = 257 > 256 not supported"):
        eng.posterior_expect(np.ones((257, 2)))
    with pytest.raises(RuntimeError, match="svihmm_posterior_expect_entries: K = 257 > 256 not supported"):
        eng.posterior_expect_entries(np.ones((257, 2)), [0], [0])
    # no posterior batch held: after loglik, viterbi and a new set_obs
    p = H.problem("poisson", 0)
    Kp = p["K"]
    tp = table(Kp, 4, 8)

    def held():
        TH.push(eng, p)
        eng.forward_backward([0], H.T, flags=L.MASK_AS_NAN, want=())
        return eng.posterior_expect(tp)
    base = held()
    for drop in (lambda: eng.loglik([0], 50), lambda: eng.viterbi([0], 50), lambda: TH.push(eng, p)):
        drop()
        for call in (lambda: eng.posterior_expect(tp), lambda: eng.posterior_expect_entries(tp, [0], [0])):
            with pytest.raises(RuntimeError, match="no posterior batch held: call svihmm_forward_backward, "
                                                   r"svihmm_estep_minibatch\(_ex\), svihmm_estep_sequences or "
                                                   "svihmm_estep_sequence_subset first"):
                call()
        np.testing.assert_array_equal(held(), base)           # the handle computes correctly afterwards
    assert P.dense_error_in_bounds(base, eng.read_rows("var_x", 0, H.T), tp) <= 1.0


def test_a_fresh_handle_holds_no_batch():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    try:
        e.set_globals(*globals_of(3, 1))
        with pytest.raises(RuntimeError, match="svihmm_posterior_expect: no posterior batch held"):
            e.posterior_expect(np.ones((3, 2)))
    finally:
        e.close()


# ---- 7. the classes on the HIP engine -------------------------------------------------------------------------------
class hidden(object):
    """The engine without its two calls: the classes then take the NumPy route on var_x."""

    def __init__(self, e):
        self.e = e

    def __enter__(self):
        self.e.posterior_expect = self.e.posterior_expect_entries = None

    def __exit__(self, *a):
        del self.e.posterior_expect, self.e.posterior_expect_entries


class counted(object):
    """Counts the engine's device calls."""

    def __init__(self, e):
        self.e, self.n = e, [0, 0]

    def __enter__(self):
        dense, ents = self.e.posterior_expect, self.e.posterior_expect_entries

        def d(*a):
            self.n[0] += 1
            return dense(*a)

        def s(*a):
            self.n[1] += 1
            return ents(*a)
        self.e.posterior_expect, self.e.posterior_expect_entries = d, s
        return self.n

    def __exit__(self, *a):
        del self.e.posterior_expect, self.e.posterior_expect_entries


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_model(eng, m, name, absent, var_x=None, prepare=False):
    """impute() on the device == impute() on the NumPy route, bit for bit; reconstruct() within the dense bound."""
    x = np.asarray(m.obs)
    tab = P.family_table(m, name)
    with counted(eng) as n:
        dev = m.impute()
        rec = m.reconstruct()
    assert n == [1, 1]                                         # both went to the device
    with hidden(eng):
        host = m.impute()
        rec_host = m.reconstruct()
    cat = (lambda a: np.concatenate(a)) if isinstance(dev, list) else (lambda a: a)
    if isinstance(dev, list):
        lens = [len(a) for a in dev]
        assert lens == [int(v) for v in np.diff(m.seq_off)] and [len(a) for a in rec] == lens
    dev, host, rec, rec_host = cat(dev), cat(host), cat(rec), cat(rec_host)
    np.testing.assert_array_equal(bits(dev), bits(host))
    np.testing.assert_array_equal(bits(dev[~absent]), bits(x[~absent]))
    assert absent.sum() > 50 and np.all(np.isfinite(dev))
    q = m.var_x if var_x is None else var_x
    r, c = np.nonzero(absent)
    np.testing.assert_array_equal(dev[r, c], P.entry_loop(q, tab, r, c))
    u = P.dense_error_in_bounds(rec, q, tab)
    print("FIG classes %s: reconstruct max error %.4f of bound" % (name, u))
    assert u <= 1.0 and P.dense_error_in_bounds(rec_host, q, tab) <= 1.0


def test_product_gaussian_model_imputes_on_the_device(eng):
    x, mask = PG.data(PG.T, 1)
    np.random.seed(3)
    m = hmmbatchcd.VBHMM(x.copy(), np.ones(PG.K), np.ones((PG.K, PG.K)), PG.emitters(), mask=mask, maxit=3, engine=eng)
    m.infer()
    assert m._pgauss_fastpath() and m._expect_engine() is eng
    np.testing.assert_array_equal(eng.read_rows("var_x", 0, PG.T), m.var_x)
    check_model(eng, m, "pgauss", ~m.var_emit[0]._present(x)[1])
    eng.viterbi([0], 20)                                        # the batch is gone: the NumPy route, the same bits
    with hidden(eng):
        host = m.impute()
    with counted(eng) as n:
        again = m.impute()
    assert n == [0, 1]
    np.testing.assert_array_equal(bits(again), bits(host))


def test_poisson_model_imputes_on_the_device(eng):
    rng = np.random.default_rng(6)
    T, D, K = 300, 3, 3
    x = rng.poisson(np.array([2.0, 9.0, 4.0])[rng.integers(0, 3, size=(T, 1))] * np.ones(D)).astype(float)
    x[rng.random(x.shape) < 0.15] = np.nan
    x[4, 1] = -1.0
    m = P.small_model("poisson", x, K=K, engine=eng, maxit=3)
    m.infer()
    assert m._poisson_fastpath() and m._expect_engine() is eng
    check_model(eng, m, "poisson", ~m.var_emit[0]._present(x)[1])


def test_list_obs_imputes_on_the_device(eng):
    x, mask = PG.data(sum(PG.LENGTHS), 2)
    xs, ms, off = PG.split(x, mask)
    np.random.seed(4)
    m = hmmbatchcd.VBHMM(xs, np.ones(PG.K), np.ones((PG.K, PG.K)), PG.emitters(), mask=ms, maxit=2, engine=eng)
    m.infer()
    # infer() ends on the last sequence's messages; the all-sequences E-step puts every row's posterior back in HBM
    assert m._expect_engine() is None
    m._full_estep_device()
    m.var_x = m._read_var_x()
    assert m._expect_engine() is eng
    check_model(eng, m, "pgauss", ~m.var_emit[0]._present(x)[1])


def test_metaobs_model_takes_the_full_local_update_route(eng):
    rng = np.random.default_rng(7)
    T, D, K = 300, 3, 3
    x = rng.poisson(np.array([2.0, 9.0, 4.0])[np.repeat(rng.integers(0, 3, size=T // 10), 10)][:, None]
                    * np.ones(D)).astype(float)
    x[rng.random(x.shape) < 0.15] = np.nan
    m = P.small_model("poisson", x, K=K, engine=eng, cls=hmmsgd_metaobs.VBHMM, tau=1.0, kappa=0.7, metaobs_half=8,
                      mb_sz=6, maxit=4, seed=3)
    m.infer()
    assert m._expect_engine() is None                           # the batch held is a minibatch of windows
    tab = P.family_table(m, "poisson")
    absent = ~m.var_emit[0]._present(x)[1]
    with counted(eng) as n:
        dev = m.impute()
    assert n == [0, 1] and m._expect_engine() is eng            # full_local_update() ran first, then the device call
    full = eng.read_rows("var_x", 0, T)
    with hidden(eng):                                           # (full_local_update() again: the same E-step)
        host = m.impute()
    np.testing.assert_array_equal(bits(dev), bits(host))
    np.testing.assert_array_equal(bits(dev[~absent]), bits(x[~absent]))
    r, c = np.nonzero(absent)
    np.testing.assert_array_equal(dev[r, c], P.entry_loop(full, tab, r, c))
    assert P.dense_error_in_bounds(m.reconstruct(), full, tab) <= 1.0
    # a decoder drops the library's batch while the engine still notes the whole chain: reconstruct() / impute() then
    # run full_local_update() again and answer for all T rows, never for the last window's var_x
    for drop in (lambda: m.viterbi(), lambda: eng.loglik([0], 50)):
        rec = m.reconstruct()
        drop()
        with counted(eng) as n:
            rec2 = m.reconstruct()
        assert n == [2, 0]                                      # refused once, then the device call on the new batch
        assert rec2.shape == (T, D)
        np.testing.assert_array_equal(rec2, rec)
        drop()
        np.testing.assert_array_equal(bits(m.impute()), bits(dev))
        drop()
        with hidden(eng):
            np.testing.assert_array_equal(bits(m.impute()), bits(dev))
            assert m.reconstruct().shape == (T, D)
