"""GPU: the resident SVI loop on the multi-column Categorical (family 3, svihmm_svi_begin_mcat) and Poisson (family 4,
svihmm_svi_begin_poisson) families: global step and ELBO against the extended-precision referee
(tests/svi_family_helpers.py), the table builders k_mcat_table / k_pois_table, three iterations against the
host-stepped route on the same device, hmmsgd_metaobs.VBHMM on both families, and the refusals.

Bounds as in tests/test_gpu_svi_globals.py (tests/svi_cases.py): step outputs 8 eps scale, ELBO 16 eps sum|terms|,
tables 32 eps max(1, |terms|).  tests/test_svi_families_ref.py shows a float64 NumPy restatement of each device
formula inside them.  Referee tests run with automatic centring off, as there.  Every loop that ran must have stayed
on its device-side counters (svi_recoveries() == 0)."""
import mpmath as mp
import numpy as np
import pytest

from tests import svi_cases as C
from tests import svi_family_helpers as H
from tests import svi_referee as R

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not R.have_extended_precision(), reason="np.longdouble is not wider than double on this host")


def _engine(events=0, centring_off=True):
    from pysvihmm_amd.engine import HipEngine
    eng = HipEngine(0)
    if centring_off:
        eng.set_variant("centring", 1)
    if events:
        eng.set_variant("svi_loop", 1)       # stream events instead of device-side counters
    return eng


# ---------------------------------------------------------------------------------------------------
#  5. step and ELBO against the referee
# ---------------------------------------------------------------------------------------------------
def _run(c, events=0):
    from pysvihmm_amd import _lib as L
    eng = _engine(events)
    try:
        recs = H.case_run(eng, c, L.TRANS_WRAP)
        return recs, eng.svi_recoveries()
    finally:
        eng.close()


@needs_ld
@pytest.mark.parametrize("case", [pytest.param(c, id=H.family_case_id(c)) for c in H.FAMILY_CASES])
def test_global_step_and_elbo(case):
    """One svi_iteration (two with AdaGrad) per case, as tests/test_gpu_svi_globals.py::test_global_step_and_elbo:
    the state after it against the referee's step fed the state before and the packed statistics the step consumed;
    svi_read_elbo against lb + the referee's global lower bound of the state read back.  mcat: a one-symbol column
    and one wider than a wave, 128 binary columns at K = 65 (k_mcat_table: 32 columns per wave), F = 1024; Poisson:
    a over 1e-2 .. 1e6, b over 1e-2 .. 1e4, counts up to 300, D = 65 and 128 (two trips of the 64-lane table and ELBO
    loops).  The stream-event loop must give the same state and ELBO bit for bit.
    Largest on the device, in units of the bound: alpha 0.182 and var_tran 0.179 (mcat K = 65, 128 binary columns,
    blocks), a 0.156 and b 0.153 (Poisson K = 64, D = 65), ada_G 0.093 (Poisson K = 3, D = 5, second AdaGrad
    iteration); ELBO 0.0152 (Poisson K = 3, D = 1, rho = 1)."""
    c = H.family_case(*case)
    recs, nrec = _run(c)
    assert nrec == 0 and len(recs) == c["nit"]
    worst = {}
    for it, rec in enumerate(recs):
        ref, glb = H.case_reference(c, rec)
        errs = R.step_errors(H.got_dict(c, rec["post"], rec["ada_post"]), ref, C.STEP_MULT)
        e_elbo = H.elbo_error(rec["elbo"], rec["packed"].lb[0], glb)
        print("FIG step %s it %d: %s ELBO %.4f of bound (elbo %.10g, sum|terms| %.3g)"
              % (H.family_case_id(case), it, {n: round(v, 3) for n, v in errs.items()}, e_elbo, rec["elbo"], float(glb[1])))
        worst[it] = (errs, e_elbo)
        assert np.isfinite(rec["elbo"])
        assert set(errs) == set(ref)
    for it, (errs, e_elbo) in worst.items():
        assert max(errs.values()) <= 1.0, (it, errs)
        assert e_elbo <= 1.0, (it, e_elbo)
    ev, nrec_ev = _run(c, events=1)
    assert nrec_ev == 0
    for ra, rb in zip(recs, ev):
        for x, y in zip(ra["post"], rb["post"]):
            np.testing.assert_array_equal(x, y, err_msg="stream-event loop")
        if ra["ada_post"] is not None:
            np.testing.assert_array_equal(ra["ada_post"], rb["ada_post"])
        assert ra["elbo"] == rb["elbo"]


# ---------------------------------------------------------------------------------------------------
#  6. tables
# ---------------------------------------------------------------------------------------------------
def test_one_column_table_has_the_categorical_familys_bits():
    """Right after svi_begin_mcat with D = 1, loglik of a window is bit-identical to loglik after svi_begin_cat on
    the same column and alpha (V = 70: two trips of the lane-strided sums)."""
    K, V, T = 5, 70, 64
    rng = np.random.default_rng(1)
    obs = rng.integers(0, V, size=(T, 1)).astype(np.float64)
    alpha, alpha0 = 0.05 + rng.gamma(0.5, 20.0, size=(K, V)), 1.0 + rng.random((K, V))
    vt, pt = R.tran_family("counts", K), C.prior_tran_for(K)
    out = []
    for fam in ("cat", "mcat"):
        eng = _engine()
        try:
            eng.set_obs(obs, None)
            if fam == "cat":
                eng.svi_begin_cat(pt, vt, alpha0, alpha, 2)
            else:
                eng.svi_begin_mcat(pt, vt, [alpha0], [alpha], 2)
            out.append(eng.loglik([3], 40))
            assert eng.svi_recoveries() == 0
        finally:
            eng.close()
    assert np.all(out[0] < 0)
    np.testing.assert_array_equal(out[0], out[1])


@needs_ld
def test_mcat_table_against_mpmath():
    """k_mcat_table for D = 4 columns (V = 2, 3, 1, 70): a probe array with one present entry per row reads every
    table entry back through loglik; against psi(alpha) - psi(column sum) within 32 eps max(1, |psi|, |psi sum|).
    Largest on the device: 0.078 of the bound."""
    K, V = 5, (2, 3, 1, 70)
    F, D = sum(V), len(V)
    rng = np.random.default_rng(2)
    obs = np.full((F, D), np.nan)
    f = 0
    for d, v in enumerate(V):
        for s in range(v):
            obs[f, d] = s
            f += 1
    alpha = [0.05 + rng.gamma(0.5, 20.0, size=(K, v)) for v in V]
    alpha0 = [1.0 + rng.random((K, v)) for v in V]
    eng = _engine()
    try:
        eng.set_obs(obs, None)
        eng.svi_begin_mcat(C.prior_tran_for(K), R.tran_family("counts", K), alpha0, alpha, 2)
        ll = eng.loglik([0], F)[0]                     # [F, K]
        assert eng.svi_recoveries() == 0
    finally:
        eng.close()
    want, scale = np.empty((F, K)), np.empty((F, K))
    with mp.workdps(30):
        f = 0
        for d, v in enumerate(V):
            for k in range(K):
                ps = mp.digamma(mp.fsum(mp.mpf(float(x)) for x in alpha[d][k]))
                for s in range(v):
                    px = mp.digamma(mp.mpf(float(alpha[d][k, s])))
                    want[f + s, k] = float(px - ps)
                    scale[f + s, k] = float(max(mp.mpf(1), abs(px), abs(ps)))
            f += v
    e = R.err_in_bound(ll, want, scale, C.PSI_MULT)
    print("FIG table mcat: %.3f of bound" % e)
    assert e <= 1.0
    np.testing.assert_array_equal(ll[5], np.zeros(K))          # the one-symbol column (feature 5): psi(a) - psi(a)


@needs_ld
def test_poisson_table_against_mpmath():
    """k_pois_table: a probe array of 2 D rows (one present column each, count 0, then count 1) reads erate exactly
    (ll = -erate) and elog - erate; against a / b and psi(a) - log b within 32 eps max(1, |psi(a)|, |log b|, a / b).
    A row with no present entry gives +0.0 for every state.  D = 65: two trips of the 64-lane loop.
    On the device: erate equal to the correctly rounded a / b in every entry, elog - erate 0.059 of the bound."""
    from pysvihmm_amd.distributions import _logfact_table
    K, D = 5, 65
    c = H.family_case("poisson", K, D, 0.3, "counts")
    a, b = c["factors"]
    obs = np.full((2 * D + 1, D), np.nan)
    for d in range(D):
        obs[d, d] = 0.0
        obs[D + d, d] = 1.0
    eng = _engine()
    try:
        eng.set_obs(obs, None)
        eng.svi_begin_poisson(c["prior_tran"], c["var_tran"], c["prior"], (a, b), H.POIS_C, 2)
        ll = eng.loglik([0], 2 * D + 1)[0]             # [2 D + 1, K]
        assert eng.svi_recoveries() == 0
    finally:
        eng.close()
    erate = -ll[:D].T                                    # [K, D]
    diff = ll[D:2 * D].T + _logfact_table(H.POIS_C)[1]   # elog - erate
    w_er, w_df, scale = np.empty((K, D)), np.empty((K, D)), np.empty((K, D))
    with mp.workdps(30):
        for k in range(K):
            for d in range(D):
                x, y = mp.mpf(float(a[k, d])), mp.mpf(float(b[k, d]))
                w_er[k, d] = float(x / y)
                w_df[k, d] = float(mp.digamma(x) - mp.log(y) - x / y)
                scale[k, d] = float(max(mp.mpf(1), abs(mp.digamma(x)), abs(mp.log(y)), x / y))
    e1, e2 = R.err_in_bound(erate, w_er, scale, C.PSI_MULT), R.err_in_bound(diff, w_df, scale, C.PSI_MULT)
    print("FIG table poisson: erate %.3f, elog - erate %.3f of bound" % (e1, e2))
    assert e1 <= 1.0 and e2 <= 1.0
    assert np.all(ll[2 * D] == 0.0) and not np.signbit(ll[2 * D]).any()


# ---------------------------------------------------------------------------------------------------
#  7. three iterations at engine level against the host-stepped route on the same device
# ---------------------------------------------------------------------------------------------------
MAXC = 60


def _engine_problem(fam, holes):
    K, D, T = 5, 3, 2000
    rng = np.random.default_rng(7 if fam == "mcat" else 8)
    sts = np.repeat(rng.integers(0, K, size=T // 10 + 1), 10)[:T]
    if fam == "mcat":
        V = (2, 3, 4)
        th = [rng.dirichlet(np.ones(v) * 0.5, size=K) for v in V]
        obs = np.stack([[rng.choice(len(t[s]), p=t[s]) for s in sts] for t in th], axis=1).astype(np.float64)
        prior = [np.full((K, v), 1.5) for v in V]
        fac = [1.0 + 5.0 * rng.random((K, v)) for v in V]
    else:
        obs = rng.poisson(np.linspace(1.0, 20.0, K)[sts][:, None] * np.linspace(1.0, 2.0, D)[None, :]).astype(np.float64)
        prior = [np.full((K, D), 2.0), np.full((K, D), 0.5)]
        rate = np.sort(rng.uniform(0.5, 25.0, size=(K, D)), axis=0)
        fac = [4.0 * rate, np.full((K, D), 4.0)]
    mask = None
    if holes:
        mask = rng.random(T) < 0.1
        obs[rng.permutation(T)[:T // 3], 1] = np.nan
        bad = rng.permutation(T)[:T // 10]
        obs[bad[::2], 0] = -1.0
        obs[bad[1::2], 0] = 1e6
    return dict(K=K, D=D, T=T, obs=obs, mask=mask, prior=prior, fac=fac, prior_tran=1.0 + rng.random((K, K)),
                var_tran=1.0 + 10.0 * rng.random((K, K)))


def _begin(eng, fam, p, maxit):
    eng.set_obs(p["obs"], p["mask"])
    if fam == "mcat":
        eng.svi_begin_mcat(p["prior_tran"], p["var_tran"], p["prior"], p["fac"], maxit)
    else:
        eng.svi_begin_poisson(p["prior_tran"], p["var_tran"], p["prior"], p["fac"], MAXC, maxit)


@pytest.mark.parametrize("variant", ["wrap", "inner", "holes", "keep"])
@pytest.mark.parametrize("fam", ["mcat", "poisson"])
def test_three_iterations_equal_the_host_stepped_route(fam, variant):
    """K = 5, D = 3, T = 2000, 8 windows of 33 rows.  The host-stepped route (SciPy tables -> set_emission_* ->
    estep -> the NumPy rules) runs on the same device; tolerances of
    test_gpu_svi_globals.py::test_lds_workgroup_globals_end_to_end (state rtol 1e-6 / atol 1e-9, ELBO rtol 1e-9).
    `inner`: statistics over the segment (8, 17); `holes`: masked rows, a column NaN in a third of the rows,
    out-of-range entries; `keep`: SVIHMM_SVI_KEEP_WINDOW, the kept rows equal a forward_backward on the last window
    under the pre-step parameters."""
    from pysvihmm_amd import _lib as L
    p = _engine_problem(fam, variant == "holes")
    B, Lm, half, T = 8, 33, 16, p["T"]
    bA, bE = (T - 2 * half - 1) / (2.0 * half * B), (T - 2 * half - 1) / ((2.0 * half + 1) * B)
    inner = (8, 17) if variant == "inner" else None
    r2 = np.random.default_rng(5)
    iters = [(r2.integers(0, T - Lm, size=B), Lm, L.TRANS_WRAP, (it + 1.0) ** -0.7, bA, bE, inner) for it in range(3)]
    eng = _engine(centring_off=False)
    try:
        _begin(eng, fam, p, 3)
        for it, (starts, _, flags, rho, _, _, _) in enumerate(iters):
            if variant == "keep" and it == 2:
                flags |= L.SVI_KEEP_WINDOW
            eng.svi_iteration(it, starts, B, Lm, flags, rho, bA, bE, inner=inner)
        elbo = eng.svi_read_elbo(3)[0]
        vt, vi, fac = eng.svi_read_factors()
        kept = eng.read_rows("var_x", (B - 1) * Lm, Lm) if variant == "keep" else None
        assert eng.svi_recoveries() == 0
        with pytest.raises(RuntimeError, match="svihmm_svi_read_state: NIW layout"):
            eng.svi_read_state()
    finally:
        eng.close()
    ref = _engine(centring_off=False)
    try:
        ref.set_obs(p["obs"], p["mask"])
        rvt, rvi, rfac, relbo = H.host_stepped(ref, fam, p["prior_tran"], p["var_tran"], p["prior"], p["fac"], MAXC, iters)
        if kept is not None:
            s2 = H.host_stepped(ref, fam, p["prior_tran"], p["var_tran"], p["prior"], p["fac"], MAXC, iters[:2])
            H.push_state(ref, fam, s2[0], s2[2], MAXC)
            want = ref.forward_backward([iters[2][0][-1]], Lm, flags=0, want=("var_x",))["var_x"][0]
            np.testing.assert_allclose(kept, want, rtol=1e-6, atol=1e-9)
    finally:
        ref.close()
    np.testing.assert_allclose(vt, rvt, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(vi, rvi, rtol=1e-6, atol=1e-9)
    for x, y in zip(fac, rfac):
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(elbo, relbo, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------
#  8. class level
# ---------------------------------------------------------------------------------------------------
def _class_data(fam, T=4000, K=5, D=3):
    rng = np.random.default_rng(21 if fam == "mcat" else 22)
    sts = np.repeat(rng.integers(0, K, size=T // 12 + 1), 12)[:T]
    if fam == "mcat":
        th = [rng.dirichlet(np.ones(v) * 0.5, size=K) for v in (2, 3, 4)]
        obs = np.stack([[rng.choice(len(t[s]), p=t[s]) for s in sts] for t in th], axis=1).astype(np.float64)
    else:
        obs = rng.poisson(np.linspace(1.0, 20.0, K)[sts][:, None] * np.linspace(1.0, 2.0, D)[None, :]).astype(np.float64)
    return obs, rng.random(T) < 0.1


def _model(fam, obs, mask, engine, K=5, **kw):
    from pysvihmm_amd import hmmsgd_metaobs
    from pysvihmm_amd.distributions import ProductCategorical, ProductPoisson
    np.random.seed(4)
    if fam == "mcat":
        emit = np.array([ProductCategorical(alphav_0=[np.ones(v) * 1.5 for v in (2, 3, 4)]) for _ in range(K)])
    else:
        emit = np.array([ProductPoisson(np.full(3, 2.0), np.full(3, 0.5), max_count=MAXC) for _ in range(K)])
    return hmmsgd_metaobs.VBHMM(obs.copy(), np.ones(K), np.ones((K, K)), emit, tau=1.0, kappa=0.7, metaobs_half=6,
                                mb_sz=5, mask=mask, maxit=3, seed=4, engine=engine, **kw)


def _factors(fam, G):
    return list(G.alpha_mf) if fam == "mcat" else [G.alpha_mf, G.beta_mf]


def _close(fam, a, b, rtol):
    """tests/test_categorical._close_cat for these families"""
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=max(rtol, 1e-8))
    for G, H_ in zip(a.var_emit, b.var_emit):
        for x, y in zip(_factors(fam, G), _factors(fam, H_)):
            np.testing.assert_allclose(x, y, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(a.var_x, b.var_x, rtol=rtol * 10, atol=1e-11)


@pytest.mark.parametrize("adagrad", [False, True])
@pytest.mark.parametrize("fam", ["mcat", "poisson"])
def test_class_device_loop_equals_host_loops(fam, adagrad):
    """hmmsgd_metaobs.VBHMM, K = 5, D = 3, T = 4000, Dirichlet priors 1.5: HIP device loop == HIP host loop ==
    oracle-engine host loop at the 1e-7 / 1e-6 of test_categorical.py::test_categorical_device_loop_on_gpu."""
    from oracle.engine import OracleEngine
    obs, mask = _class_data(fam)
    a = _model(fam, obs, mask, None, adagrad=adagrad)
    assert a._svi_family() == fam and a._svi_device_ok()
    a.infer()
    assert a.engine.name == "hip" and a.engine.svi_recoveries() == 0
    b = _model(fam, obs, mask, None, adagrad=adagrad); b.infer(device_loop=False)
    c = _model(fam, obs, mask, OracleEngine(), adagrad=adagrad); c.infer()
    assert min(x.min() for G in a.var_emit for x in _factors(fam, G)) > 0
    _close(fam, a, b, 1e-7)
    _close(fam, a, c, 1e-6)
    assert np.all(np.isfinite(a.iter_time)) and np.all(a.iter_time > 0)
    assert np.all(np.isfinite(a.elbo_vec))


@pytest.mark.parametrize("mode", ["growBuffer", "adaptive"])
@pytest.mark.parametrize("fam", ["mcat", "poisson"])
def test_class_device_loop_with_growing_windows(fam, mode):
    """One run each with growBuffer=True and with adaptive=True: the device loop pulls its state for
    select_buffer / select_L (svihmm_grow_windows takes both families) and equals the host loop."""
    obs, mask = _class_data(fam)
    kw = dict(growBuffer=True) if mode == "growBuffer" else {}
    ikw = dict(perIter=2, epsilon=1e-3, Lcutoff=12)
    if mode == "adaptive":
        ikw["adaptive"] = True
    a = _model(fam, obs, mask, None, **kw)
    assert a._svi_device_ok()
    a.infer(**ikw)
    assert a.engine.svi_recoveries() == 0
    b = _model(fam, obs, mask, None, **kw); b.infer(device_loop=False, **ikw)
    _close(fam, a, b, 1e-7)


# ---------------------------------------------------------------------------------------------------
#  9. refusals
# ---------------------------------------------------------------------------------------------------
def _loop_is_intact(eng, fam, it, starts):
    """the loop begun earlier still steps, and its state is readable"""
    from pysvihmm_amd import _lib as L
    eng.svi_iteration(it, starts, len(starts), 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)
    vt, vi, fac = eng.svi_read_factors()
    assert np.all(np.isfinite(vt)) and all(np.all(np.isfinite(x)) and np.all(x > 0) for x in fac)
    assert np.isfinite(eng.svi_read_elbo(it + 1)[0][it])
    assert eng.svi_recoveries() == 0


def test_refusals_leave_the_handle_and_the_loop_intact():
    from pysvihmm_amd import _lib as L
    import ctypes
    K = 3
    starts = np.array([0, 20, 40])
    cm = H.family_case("mcat", K, (2, 5), 0.3, "counts")
    cp = H.family_case("poisson", K, 2, 0.3, "counts")
    pt, vt = cm["prior_tran"], cm["var_tran"]
    eng = _engine()
    try:
        # ---- multi-column Categorical
        eng.set_obs(cm["obs"], None)
        eng.svi_begin_mcat(pt, vt, cm["prior"], cm["factors"], 8)
        it = 0
        bad = [
            ("resident observations have 2", [np.ones((K, 2))] * 3, [np.ones((K, 2))] * 3),          # D != resident D
            ("exceeds SVIHMM_MCAT_MAX_F", [np.ones((K, 1000)), np.ones((K, 25))], [np.ones((K, 1000)), np.ones((K, 25))]),
            ("Dirichlet parameters must be positive", cm["prior"], [cm["factors"][0], 0.0 * cm["factors"][1]]),
            ("Dirichlet parameters must be positive", [cm["prior"][0], -cm["prior"][1]], cm["factors"]),
        ]
        for msg, a0, a in bad:
            with pytest.raises(RuntimeError, match="svihmm_svi_begin_mcat: .*" + msg):
                eng.svi_begin_mcat(pt, vt, a0, a, 8)
            _loop_is_intact(eng, "mcat", it, starts); it += 1
        # V[d] < 1 (the Python wrapper derives V from the arrays' shapes: straight through the C ABI)
        V = np.array([2, 0], dtype=np.int32)
        flat = np.ascontiguousarray(np.ones((K, 2)))
        rc = eng._lib.svihmm_svi_begin_mcat(eng._h, K, 2, V.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), L.dptr(pt),
                                            L.dptr(vt), L.dptr(flat), L.dptr(flat), 8)
        assert rc != 0 and "V[1] = 0" in L.last_error()
        _loop_is_intact(eng, "mcat", it, starts); it += 1
        with pytest.raises(RuntimeError, match="svihmm_svi_read_state: NIW layout"):
            eng.svi_read_state()
        # an upload of the same family and shape keeps the loop alive, a NIW upload ends it
        eng.set_emission_mcat([np.log(np.full((K, 2), 0.5)), np.log(np.full((K, 5), 0.2))])
        _loop_is_intact(eng, "mcat", it, starts); it += 1
        eng.set_emission_niw(np.zeros((K, 2)), np.tile(np.eye(2), (K, 1, 1)), np.ones(K), np.full(K, 5.0))
        with pytest.raises(RuntimeError, match="call svihmm_svi_begin first"):
            eng.svi_iteration(it, starts, 3, 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)
        # ---- Poisson
        eng.set_obs(cp["obs"], None)
        eng.svi_begin_poisson(pt, vt, cp["prior"], cp["factors"], H.POIS_C, 8)
        it = 0
        a, b = cp["factors"]
        bad = [
            ("resident observations have 2", (np.ones((K, 3)), np.ones((K, 3))), (np.ones((K, 3)), np.ones((K, 3))), 10),
            ("Gamma parameters must be positive", cp["prior"], (a, 0.0 * b), 10),
            ("Gamma parameters must be positive", (-cp["prior"][0], cp["prior"][1]), (a, b), 10),
        ]
        for msg, p0, f, cmax in bad:
            with pytest.raises(RuntimeError, match="svihmm_svi_begin_poisson: .*" + msg):
                eng.svi_begin_poisson(pt, vt, p0, f, cmax, 8)
            _loop_is_intact(eng, "poisson", it, starts); it += 1
        # C out of range and a non-finite logfact[c]: through the C ABI (the wrapper builds the table itself)
        pb = np.ascontiguousarray(np.stack(cp["prior"])); fb = np.ascontiguousarray(np.stack([a, b]))
        lf = np.zeros(4); lf[2] = np.inf
        for cmax, tab, msg in ((L.POISSON_MAX_COUNT + 1, np.zeros(4), "outside [0, SVIHMM_POISSON_MAX_COUNT"),
                               (-1, np.zeros(4), "outside [0, SVIHMM_POISSON_MAX_COUNT"),
                               (3, lf, "logfact[2] is not finite")):
            rc = eng._lib.svihmm_svi_begin_poisson(eng._h, K, 2, L.dptr(pt), L.dptr(vt), L.dptr(pb), L.dptr(fb),
                                                   L.dptr(tab), cmax, 8)
            assert rc != 0 and msg in L.last_error(), L.last_error()
            _loop_is_intact(eng, "poisson", it, starts); it += 1
        with pytest.raises(RuntimeError, match="svihmm_svi_read_state: NIW layout"):
            eng.svi_read_state()
        eng.set_emission_poisson(np.zeros((K, 2)), np.ones((K, 2)), H.POIS_C)
        _loop_is_intact(eng, "poisson", it, starts); it += 1
        eng.set_emission_niw(np.zeros((K, 2)), np.tile(np.eye(2), (K, 1, 1)), np.ones(K), np.full(K, 5.0))
        with pytest.raises(RuntimeError, match="call svihmm_svi_begin first"):
            eng.svi_iteration(it, starts, 3, 17, L.TRANS_WRAP, 0.5, 3.0, 3.0)
    finally:
        eng.close()
