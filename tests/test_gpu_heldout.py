"""svihmm_heldout_rows / svihmm_heldout_entries on the MI355X: held-out log-probability against the posterior rows the
last E-step left in HBM (kernels_heldout.h), through the C ABI, HipEngine and the classes.

Shapes: the Poisson problems of tests/poisson_helpers.py (T = 700; K = 3, 16, 64, 65, 256; D up to 128; tables beyond
64 KB) and multi-column Categorical models of the same K set whose columns mix 1, 2 and 7 symbols, one of them at
D = 128, sum V = 1024 (tests/heldout_helpers.py).  The NumPy statements of both formulas live there too."""
import ctypes as C

import numpy as np
import pytest

from oracle import ref_numpy as R
from pysvihmm_amd import _lib as L
from tests import heldout_helpers as H
from tests import mcat_helpers as MH
from tests import poisson_helpers as PH
from tests.helpers import make_problem

pytestmark = pytest.mark.gpu

CASES = ([("poisson", i) for i in range(len(PH.SHAPES))] + [("mcat", i) for i in range(len(H.MCAT_K))])
CASE_IDS = ["pois-" + s for s in PH.IDS] + ["mcat-" + s for s in H.MCAT_IDS]
ULP = 2.0 ** -52


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def push(e, p, x=None, mask=True):
    e.set_obs(p["x"] if x is None else x, p["mask"] if mask is True else mask)
    e.set_globals(p["mod_init"], p["ltran"])
    if p["fam"] == "poisson":
        e.set_emission_poisson(p["elog"], p["erate"], p["C"])
    else:
        e.set_emission_mcat(MH.split_tables(p["logp"], p["V"]))


def entry_bound(p, M):
    """|device - NumPy| per entry: about 3 ulp-of-M per v_k = log(q_k + 1e-9) + term_k, carried through exp, a K-term
    sum and log, and the same again on the NumPy side.  M: the largest magnitude among the entry's operands."""
    return 2.0 * (8.0 * M + p["K"] + 8.0) * ULP


# ---- 1. the entry kernel in isolation ---------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,i", CASES, ids=CASE_IDS)
def test_entry_kernel_against_numpy_on_the_same_posterior_bits(eng, fam, i):
    """out_lp entry by entry against the NumPy formula on the var_x bits the device itself hands out.  The term is
    bit-identical by the fixed operation order; log, exp and the sum order differ: |d| <= 2 (8 M + K + 8) 2^-52.
    NaN positions and the count are exact; the mean is the sum of the finite out_lp in workgroup order, to 4 ulp."""
    p = H.problem(fam, i)
    push(eng, p)
    q = eng.forward_backward([0], H.T, flags=L.MASK_AS_NAN, want=("var_x",))["var_x"][0]
    rows, cols, vals, _ = H.entry_list(p, p["x"], 3000, seed=77 + i)
    mean, cnt, lp = eng.heldout_entries(rows, cols, vals, resident=False, want_lp=True)
    want, M = H.heldout_entries_numpy(p, q, rows, cols, vals)
    assert np.array_equal(np.isnan(lp), np.isnan(want))
    ok = ~np.isnan(want)
    assert cnt == ok.sum() and ok.mean() >= 0.9
    d = np.abs(lp[ok] - want[ok])
    bound = entry_bound(p, M[ok])
    worst = int(np.argmax(d / bound))
    print("%s: max |d| / bound = %.3g (|d| = %.3g, M = %.3g)" % (CASE_IDS[CASES.index((fam, i))], (d / bound).max(),
                                                              d[worst], M[ok][worst]))
    assert np.all(d <= bound)
    km, kc = H.kernel_order_mean(lp)
    assert kc == cnt
    assert abs(mean - km) <= 4 * ULP * abs(km)
    # the same posterior rows read back again: the held-out call left them alone
    assert np.array_equal(eng.read_rows("var_x", 0, H.T), q)


# ---- 2. entry counts at the kernel's seams ------------------------------------------------------------------------------
@pytest.mark.parametrize("fam,i", [("poisson", 0), ("poisson", 3), ("mcat", 0), ("mcat", 3)],
                         ids=["pois-K3", "pois-K65", "mcat-K3", "mcat-K65"])
def test_entry_counts_at_the_seams(eng, fam, i):
    p = H.problem(fam, i)
    assert p["K"] in (3, 65)
    push(eng, p)
    q = eng.forward_backward([0], H.T, flags=L.MASK_AS_NAN, want=("var_x",))["var_x"][0]
    rng = np.random.default_rng(5 + i)
    E = H.PER_BLOCK
    for n in (1, 15, 16, 17, E - 1, E, E + 1, 3 * E + 5):
        rows = rng.integers(0, H.T, size=n)
        cols = rng.integers(0, p["D"], size=n).astype(np.int32)
        vals = p["x"][rows, cols]
        rows[-1], cols[-1], vals[-1] = H.T - 1, p["D"] - 1, 0.0          # the last entry counts: the tail is scored
        a = eng.heldout_entries(rows, cols, vals, resident=False, want_lp=True)
        b = eng.heldout_entries(rows, cols, vals, resident=False, want_lp=True)
        assert a[0] == b[0] and a[1] == b[1] and np.array_equal(a[2], b[2], equal_nan=True)     # bit-identical
        want, M = H.heldout_entries_numpy(p, q, rows, cols, vals)
        ok = ~np.isnan(want)
        assert len(a[2]) == n and np.array_equal(np.isnan(a[2]), ~ok) and a[1] == ok.sum() and ok[-1]
        assert np.all(np.abs(a[2][ok] - want[ok]) <= entry_bound(p, M[ok]))
        km, _ = H.kernel_order_mean(a[2])
        assert abs(a[0] - km) <= 4 * ULP * abs(km)
        assert eng.heldout_entries(rows, cols, vals, resident=False) == (a[0], a[1])          # without out_lp
    assert eng.heldout_entries([], [], [], resident=False) == (None, 0)
    assert eng.heldout_entries([], [], []) == (None, 0)
    nan = eng.heldout_entries([3, 4], [0, 0], [np.nan, -1.0], resident=False, want_lp=True)
    assert nan[:2] == (None, 0) and np.isnan(nan[2]).all()


# ---- 3. end to end against the referee ---------------------------------------------------------------------------------
def run_kind(e, cs, kind):
    """The E-step of a batch kind on the case's blanked data, masked rows missing; returns the number of batch rows."""
    p = cs["p"]
    push(e, p, x=cs["xb"])
    if kind == "windows":
        e.estep(H.WINDOW_STARTS, H.WINDOW_LM, flags=L.MASK_AS_NAN | L.TRANS_WRAP)
    elif kind == "chain":
        e.forward_backward([0], H.T, flags=L.MASK_AS_NAN, want=())
    else:
        e.set_sequences(np.diff(cs["off"]))
        if kind == "sequences":
            e.estep_sequences(flags=L.MASK_AS_NAN)
        else:
            e.estep_sequence_subset(H.SUBSET_IDX, flags=L.MASK_AS_NAN)
    return len(cs["res"])


@pytest.mark.parametrize("kind", H.KINDS)
@pytest.mark.parametrize("fam,i", CASES, ids=CASE_IDS)
def test_end_to_end_against_the_referee(eng, fam, i, kind):
    """Both modes after every kind of E-step-type call -- a window batch (5, 40) with overlapping windows
    (svihmm_estep_minibatch), the whole chain (1, 700) (svihmm_forward_backward), svihmm_estep_sequences and
    svihmm_estep_sequence_subset with a repeated sequence -- against the NumPy formulas on the NumPy referee's
    posteriors (oracle.ref_numpy on the helper lliks): the mean to rtol 1e-9, the project's figure for this quantity
    (tests/test_gpu_parity.py), counts and NaN positions exactly."""
    cs = H.e2e_case(fam, i, kind)
    p = cs["p"]
    n = run_kind(eng, cs, kind)
    mean, cnt, lp = eng.heldout_rows(want_lp=True)
    want = H.heldout_rows_numpy(cs["q"], cs["ll_true"], cs["masked"])
    wm, wc = H.mean_count(want)
    assert len(lp) == n and cnt == wc and wc >= 3 and np.array_equal(np.isnan(lp), np.isnan(want))
    print("rows    %s %s: rel diff of the mean %.3g" % (fam, kind, abs(mean - wm) / abs(wm)))
    np.testing.assert_allclose(mean, wm, rtol=1e-9)
    rows, cols, vals = cs["rows"], cs["cols"], cs["vals"]
    emean, ecnt, elp = eng.heldout_entries(rows, cols, vals, resident=False, want_lp=True)
    ewant, _ = H.heldout_entries_numpy(p, cs["q"], rows, cols, vals)
    em, ec = H.mean_count(ewant)
    assert ecnt == ec and np.array_equal(np.isnan(elp), np.isnan(ewant))
    print("entries %s %s: rel diff of the mean %.3g" % (fam, kind, abs(emean - em) / abs(em)))
    np.testing.assert_allclose(emean, em, rtol=1e-9)
    # row mode again after the entries: one E-step scored several ways, bit for bit
    again = eng.heldout_rows(want_lp=True)
    assert again[0] == mean and again[1] == cnt and np.array_equal(again[2], lp, equal_nan=True)


@pytest.mark.parametrize("fam", ["poisson", "mcat"])
def test_resident_rows_map_to_batch_rows(eng, fam):
    """resident=True: after a window batch a resident row scores once per occurrence in the windows, after
    estep_sequences unchanged, after a subset at its positions in the gathered order; a row outside raises."""
    for kind in H.KINDS:
        cs = H.e2e_case(fam, 1, kind)
        run_kind(eng, cs, kind)
        res, rows, cols, vals = cs["res"], cs["rows"], cs["cols"], cs["vals"]
        # every speckled entry by its resident row: all occurrences of that row in the batch
        rr = res[rows]
        mean, cnt, lp, src = eng.heldout_entries(rr, cols, vals, resident=True, want_lp=True)
        occ = [np.flatnonzero(res == r) for r in rr]
        g = np.concatenate(occ)
        e = np.concatenate([np.full(len(o), j) for j, o in enumerate(occ)])
        assert np.array_equal(src, e)
        bmean, bcnt, blp = eng.heldout_entries(g, cols[e], vals[e], resident=False, want_lp=True)
        assert (mean, cnt) == (bmean, bcnt) and np.array_equal(lp, blp, equal_nan=True)
        if kind in ("windows", "subset"):
            assert len(g) > len(rr)                     # overlapping windows / the repeated sequence
            outside = np.setdiff1d(np.arange(len(cs["p"]["x"])), res)[:1]
            with pytest.raises(ValueError, match="lies in no"):
                eng.heldout_entries(outside, [0], [0.0])
        else:
            assert np.array_equal(g, rr)


def _small_family(name):
    """K = 9, D = 3 (as test_pred_logprob_vs_numpy) on the sequence lengths of the product families' tests:
    (push(engine), lliks(rows, masked-as-missing))."""
    K, D = 9, 3
    Ts = sum(PH.LENGTHS)
    pb = make_problem(K, D, Ts, seed=66, miss=0.15)
    obs, mask = pb["obs"], pb["mask"]
    if name == "niw":
        par = (pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        setter, ll = "set_emission_niw", lambda x: R.lliks_niw(x, *par)
    elif name == "diag":
        rng = np.random.default_rng(1)
        par = (pb["mu"], 0.5 + 4 * rng.random((K, D)), 2.0 + 5 * rng.random((K, D)), 1.0 + 6 * rng.random((K, D)))
        setter, ll = "set_emission_diag", lambda x: R.lliks_diag(x, *par)
    else:
        rng = np.random.default_rng(2)
        V = 6
        obs = ((pb["sts"] + rng.integers(0, 3, size=Ts)) % V).astype(np.float64)[:, None]
        a = rng.random((K, V)) * 4 + 0.3
        from scipy.special import digamma
        logp = digamma(a) - digamma(a.sum(1))[:, None]
        par = (logp,)
        setter = "set_emission_cat"

        def ll(x):
            out = np.zeros((len(x), K))
            ok = ~np.isnan(x[:, 0])
            out[ok] = logp[:, x[ok, 0].astype(int)].T
            return out
    return pb, obs, mask, setter, par, ll


@pytest.mark.parametrize("name", ["niw", "diag", "cat"])
def test_row_mode_on_a_list_for_the_other_families(eng, name):
    pb, obs, mask, setter, par, ll = _small_family(name)
    eng.set_obs(obs, mask)
    eng.set_globals(pb["mod_init"], pb["ltran"])
    getattr(eng, setter)(*par)
    eng.set_sequences(PH.LENGTHS)
    off = np.concatenate(([0], np.cumsum(PH.LENGTHS)))
    xm = obs.copy()
    xm[mask] = np.nan
    llm = np.nan_to_num(ll(xm))
    q = np.concatenate([H.referee_posterior(llm[a:b], pb["mod_init"], pb["ltran"]) for a, b in zip(off[:-1], off[1:])])
    want = H.heldout_rows_numpy(q, ll(obs), mask)
    eng.estep_sequences(flags=L.MASK_AS_NAN)
    mean, cnt, lp = eng.heldout_rows(want_lp=True)
    assert cnt == mask.sum() and np.array_equal(np.isnan(lp), ~mask)
    np.testing.assert_allclose(mean, H.mean_count(want)[0], rtol=1e-9)
    idx = np.array([5, 2, 5], dtype=np.int32)
    eng.estep_sequence_subset(idx, flags=L.MASK_AS_NAN)
    res = np.concatenate([np.arange(off[s], off[s + 1]) for s in idx])
    mean, cnt = eng.heldout_rows()
    assert cnt == mask[res].sum()
    np.testing.assert_allclose(mean, H.mean_count(want[res])[0], rtol=1e-9)
    if name != "cat":
        with pytest.raises(RuntimeError, match="multi-column Categorical and the Poisson family only"):
            eng.heldout_entries([0], [0], [1.0], resident=False)


# ---- 4. row mode agrees with what exists --------------------------------------------------------------------------------
@pytest.mark.parametrize("B,Lm", [(5, 40), (230, 12)])
def test_row_mode_agrees_with_pred_logprob(eng, B, Lm):
    K, D, T = 9, 3, 4000
    pb = make_problem(K, D, T, seed=66, miss=0.15)
    starts = (np.arange(B) * 17) % (T - Lm + 1)
    eng.set_obs(pb["obs"], pb["mask"])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    tot, cnt = 0.0, 0
    for s0 in starts:
        m = pb["mask"][s0:s0 + Lm]
        x = pb["obs"][s0:s0 + Lm].copy()
        xm = x.copy()
        xm[m] = np.nan
        ll = R.lliks_niw(xm, pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        q = H.referee_posterior(ll, pb["mod_init"], pb["ltran"])
        if m.any():
            lt = R.lliks_niw(x[m], pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
            tot += np.sum(np.logaddexp.reduce(np.log(q[m] + 1e-9) + lt, axis=1))
            cnt += int(m.sum())
    eng.forward_backward(starts, Lm, flags=L.MASK_AS_NAN, want=())
    hv, hn = eng.heldout_rows()
    pv, pn = eng.pred_logprob(starts, Lm, flags=L.MASK_AS_NAN)
    assert hn == pn == cnt
    np.testing.assert_allclose(hv, tot / cnt, rtol=1e-9)
    np.testing.assert_allclose(pv, tot / cnt, rtol=1e-9)
    eng.set_obs(pb["obs"], None)                        # no mask on the handle: nothing to score, nothing launched
    eng.forward_backward(starts, Lm, flags=L.MASK_AS_NAN, want=())
    assert eng.heldout_rows() == (None, 0)
    r = eng.heldout_rows(want_lp=True)
    assert r[:2] == (None, 0) and len(r[2]) == B * Lm and np.isnan(r[2]).all()


@pytest.mark.parametrize("fam", ["poisson", "mcat"])
def test_pred_logprob_still_refuses_the_table_families(eng, fam):
    push(eng, H.problem(fam, 0))
    with pytest.raises(RuntimeError, match="NIW emission only"):
        eng.pred_logprob([0], 50)


# ---- 5. state is left alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fam", ["poisson", "mcat"])
def test_heldout_calls_leave_the_state_alone(eng, fam):
    cs = H.e2e_case(fam, 1, "windows")
    run_kind(eng, cs, "windows")
    n = len(H.WINDOW_STARTS) * H.WINDOW_LM
    packed = eng.read_packed().buf.copy()
    q = eng.read_rows("var_x", 0, n)
    prec = eng.precision()
    wrows = cs["rows"]
    first = (eng.heldout_rows(want_lp=True), eng.heldout_entries(wrows, cs["cols"], cs["vals"], resident=False))
    assert np.array_equal(eng.read_packed().buf, packed)
    assert np.array_equal(eng.read_rows("var_x", 0, n), q)
    assert eng.precision() == prec
    # a suffstats call in between computes on the caller's posteriors: the batch held is still the E-step's
    eng.suffstats(H.WINDOW_STARTS, H.WINDOW_LM, q.reshape(len(H.WINDOW_STARTS), H.WINDOW_LM, -1), flags=L.TRANS_WRAP)
    second = (eng.heldout_rows(want_lp=True), eng.heldout_entries(wrows, cs["cols"], cs["vals"], resident=False))
    assert first[0][:2] == second[0][:2] and np.array_equal(first[0][2], second[0][2], equal_nan=True)
    assert first[1] == second[1]
    cs = H.e2e_case(fam, 1, "sequences")
    push(eng, cs["p"], x=cs["xb"])
    eng.set_sequences(np.diff(cs["off"]))
    a, lb_a, q0_a = eng.estep_sequences(flags=L.MASK_AS_NAN)
    eng.heldout_rows()
    eng.heldout_entries(cs["rows"], cs["cols"], cs["vals"])
    assert np.array_equal(eng.read_packed().buf, a.buf)
    b, lb_b, q0_b = eng.estep_sequences(flags=L.MASK_AS_NAN)
    assert np.array_equal(a.buf, b.buf) and np.array_equal(lb_a, lb_b) and np.array_equal(q0_a, q0_b)


# ---- 6. failures ---------------------------------------------------------------------------------------------------------
def test_failures_have_messages_and_leave_the_handle_usable():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    try:
        lib, h = e._lib, e._h
        out2 = np.empty(2)
        i32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        rows, cols, vals = np.array([0, 1], dtype=np.int64), np.array([0, 0], dtype=np.int32), np.array([1.0, 2.0])

        def entries(n=2, r=rows, c=cols, v=vals, o=out2, handle=None):
            return lib.svihmm_heldout_entries(h if handle is None else handle, n, L.i64ptr(r), None if c is None else i32(c),
                                              L.dptr(v), L.dptr(o), None)

        def fails(rc, pattern):
            assert rc != 0
            with pytest.raises(RuntimeError, match=pattern):
                L.check(rc, "call")

        fails(lib.svihmm_heldout_rows(None, L.dptr(out2), None), "svihmm_heldout_rows: NULL handle")
        fails(lib.svihmm_heldout_rows(h, None, None), "svihmm_heldout_rows: out2 is NULL")
        fails(lib.svihmm_heldout_entries(None, 2, L.i64ptr(rows), i32(cols), L.dptr(vals), L.dptr(out2), None),
              "svihmm_heldout_entries: NULL handle")
        fails(entries(o=None), "svihmm_heldout_entries: out2 is NULL")
        fails(entries(n=-1), "n = -1 must not be negative")
        fails(entries(r=None), "row, col and val must be given")
        fails(entries(c=None), "row, col and val must be given")
        fails(entries(v=None), "row, col and val must be given")
        # no posterior batch yet: the message names the calls that leave one
        p = H.problem("poisson", 0)
        push(e, p)
        for rc in (entries(), lib.svihmm_heldout_rows(h, L.dptr(out2), None)):
            fails(rc, "no posterior batch held: call svihmm_forward_backward, svihmm_estep_minibatch")
        e.forward_backward([0, 100], 50, flags=L.MASK_AS_NAN, want=())
        assert e.heldout_entries(rows, cols, vals, resident=False)[1] == 2           # usable
        fails(entries(r=np.array([0, 100], dtype=np.int64)), r"row\[1\] = 100 is outside \[0, nrows = 100\)")
        fails(entries(r=np.array([-1, 0], dtype=np.int64)), r"row\[0\] = -1 is outside")
        fails(entries(c=np.array([0, 2], dtype=np.int32)), r"col\[1\] = 2 is outside \[0, D = 2\)")
        fails(entries(c=np.array([-3, 0], dtype=np.int32)), r"col\[0\] = -3 is outside")
        assert e.heldout_entries(rows, cols, vals, resident=False)[1] == 2 and e.heldout_rows()[1] > 0
        # a decoder since: its batch is gone, and the message says which call is needed
        e.viterbi([0], 60)
        for rc in (entries(), lib.svihmm_heldout_rows(h, L.dptr(out2), None)):
            fails(rc, "no posterior batch held: call svihmm_forward_backward.*a decoder")
        e.estep([0, 100], 50, flags=L.MASK_AS_NAN)
        assert e.heldout_rows()[1] > 0
        e.loglik([0], 10)
        fails(entries(), "no posterior batch held")
        e.set_sequences([300, 400])
        e.estep_sequences(flags=L.MASK_AS_NAN)
        assert e.heldout_rows()[1] == p["mask"].sum()
        e.viterbi_sequences()
        fails(lib.svihmm_heldout_rows(h, L.dptr(out2), None), "no posterior batch held")
        # another family than the batch's; entries take the two product families only
        e.estep_sequences(flags=L.MASK_AS_NAN)
        pm = H.problem("mcat", 0)
        e.set_emission_mcat(MH.split_tables(pm["logp"], pm["V"]))
        fails(lib.svihmm_heldout_rows(h, L.dptr(out2), None), "emission family is not the one the posterior batch held")
        push(e, p)
        pb = make_problem(3, 2, H.T, seed=1, miss=0.1)
        e.set_obs(pb["obs"], pb["mask"])
        e.set_globals(pb["mod_init"], pb["ltran"])
        e.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        e.forward_backward([0], 200, flags=L.MASK_AS_NAN, want=())
        fails(entries(), "multi-column Categorical and the Poisson family only")
        assert e.heldout_rows()[1] == pb["mask"][:200].sum()
        # a batch of host lliks has no true observation
        e.set_lliks(np.zeros((1, 40, 3)))
        e.forward_backward(None, 40, flags=L.USE_HOST_LLIKS, want=(), B=1)
        fails(lib.svihmm_heldout_rows(h, L.dptr(out2), None), "host lliks.*no true observation")
        # the globals' K changed since
        e.forward_backward([0], 200, flags=L.MASK_AS_NAN, want=())
        pb4 = make_problem(4, 2, 50, seed=2)
        e.set_globals(pb4["mod_init"], pb4["ltran"])
        fails(lib.svihmm_heldout_rows(h, L.dptr(out2), None), r"globals' K \(4\) is not the K of the posterior batch held \(3\)")
        # K > 256
        pw = make_problem(257, 2, 120, seed=3, miss=0.2)
        e.set_obs(pw["obs"], pw["mask"])
        e.set_globals(pw["mod_init"], pw["ltran"])
        e.set_emission_niw(pw["mu"], pw["sigma"], pw["kappa"], pw["nu"])
        e.forward_backward([0], 120, flags=L.MASK_AS_NAN, want=())
        fails(lib.svihmm_heldout_rows(h, L.dptr(out2), None), "K = 257 > 256 not supported")
        fails(entries(), "K = 257 > 256 not supported")
        # ... and the handle still works
        push(e, p)
        e.forward_backward([0], H.T, flags=L.MASK_AS_NAN, want=())
        assert e.heldout_rows()[1] == p["mask"].sum()
    finally:
        e.close()


# ---- 7. the classes ------------------------------------------------------------------------------------------------------
def test_batchcd_entries_on_a_list_of_sequences():
    from pysvihmm_amd import hmmbatchcd, util
    from pysvihmm_amd.distributions import ProductPoisson
    K, D, CMAX = 4, 3, 255
    lam = np.array([[1.0, 9.0, 30.0], [6.0, 1.5, 12.0], [15.0, 20.0, 2.0], [3.0, 40.0, 60.0]])
    lengths = (40, 1, 65, 30, 64, 57, 43)
    rng = np.random.default_rng(2)
    Tt = sum(lengths)
    sts = np.repeat(rng.integers(0, K, size=Tt // 12 + 1), 12)[:Tt]
    x = rng.poisson(lam[sts]).astype(float)
    x[rng.random(x.shape) < 0.05] = np.nan
    off = np.concatenate(([0], np.cumsum(lengths)))
    xs = [x[a:b] for a, b in zip(off[:-1], off[1:])]
    xb, r, c, v = util.speckle_holdout(xs, 0.1, seed=4)
    erng = np.random.default_rng(9)
    emit = np.array([ProductPoisson(np.ones(D), np.full(D, 0.2), alpha_mf=erng.uniform(1.0, 40.0, size=D) * 2.0,
                                    beta_mf=np.full(D, 2.0), max_count=CMAX) for _ in range(K)])
    np.random.seed(4)
    m = hmmbatchcd.VBHMM(xb, np.ones(K), np.ones((K, K)), emit, maxit=3)
    m.infer()
    assert len(m.elbo_vec) == 3
    m.local_update()                                   # the class's own var_x under the factors infer() left
    before = (m.var_tran.copy(), m.var_init.copy(), [(e.alpha_mf.copy(), e.beta_mf.copy()) for e in m.var_emit],
              np.array(m.var_x))
    tabs = [e.expected_tables() for e in m.var_emit]
    p = dict(fam="poisson", K=K, D=D, C=CMAX, elog=np.stack([t[0] for t in tabs]), erate=np.stack([t[1] for t in tabs]),
             logfact=PH.logfact_table(CMAX))
    want, _ = H.heldout_entries_numpy(p, before[3], r, c, v)
    val, lp = m.heldout_entries_logprob(r, c, v, per_entry=True)
    assert len(lp) == len(r) > 50 and not np.isnan(lp).any()
    np.testing.assert_allclose(val, np.mean(want), rtol=1e-9)
    np.testing.assert_allclose(lp, want, rtol=1e-9)
    assert m.heldout_entries_logprob(r, c, v) == val
    assert m.heldout_logprob() is None                 # no masked rows
    after = (m.var_tran, m.var_init, [(e.alpha_mf, e.beta_mf) for e in m.var_emit], np.array(m.var_x))
    assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(before[2], after[2]))
    assert np.array_equal(before[3], after[3])
    with pytest.raises(ValueError, match="not blanked"):
        m.heldout_entries_logprob([0], [int(np.flatnonzero(~np.isnan(m.obs[0]))[0])], [1.0])


def test_heldout_logprob_is_the_literal_host_formula():
    from pysvihmm_amd import hmmbatchcd
    from pysvihmm_amd.distributions import ProductCategorical
    K, V, Tt = 3, (2, 5, 1, 7), 300
    rng = np.random.default_rng(6)
    sts = np.repeat(rng.integers(0, K, size=Tt // 8 + 1), 8)[:Tt]
    th = [rng.dirichlet(np.ones(v) * 0.5, size=K) for v in V]
    obs = np.stack([[rng.choice(len(t[s]), p=t[s]) for s in sts] for t in th], axis=1).astype(float)
    obs[rng.random(obs.shape) < 0.05] = np.nan
    mask = rng.random(Tt) < 0.15
    emit = np.array([ProductCategorical(alphav_0=[np.ones(v) * 1.5 for v in V],
                                        alpha_mf=[rng.random(v) * 6 + 0.5 for v in V]) for _ in range(K)])
    np.random.seed(1)
    m = hmmbatchcd.VBHMM(obs.copy(), np.ones(K), np.ones((K, K)), emit, mask=mask, maxit=2)
    m.infer()
    q = m.full_local_update()
    logprob = np.zeros((int(mask.sum()), K))
    for k, odist in enumerate(m.var_emit):
        logprob[:, k] = np.log(q[mask, k] + 1e-9) + odist.expected_log_likelihood(obs[mask, :])
    want = np.mean(np.logaddexp.reduce(logprob, axis=1))
    vt = m.var_tran.copy()
    np.testing.assert_allclose(m.heldout_logprob(), want, rtol=1e-9)
    np.testing.assert_allclose(m.pred_logprob(), want, rtol=1e-12)
    assert np.array_equal(m.var_tran, vt) and np.array_equal(m.var_x, q)
