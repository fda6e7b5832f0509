"""GPU: the global kernels of the resident SVI loop against the extended-precision referee (tests/svi_referee.py).

k_svi_globals (GTH stationary vector, psi-expectations with digamma_d), svi_tran_step, k_svi_global_step /
k_svi_global_step_simple / the merged step of k_svi_step_theta32s, and k_svi_vlb* / svi_rowterm / the two ELBO
assemblies are otherwise checked end to end against the eig-based oracle engine at 1e-6 / 1e-9 on benign inputs.
Here every kernel is held to a float64 error bound on the inputs where it can go wrong: all three GTH
implementations (K <= 64 one wavefront in registers, K = 65 .. 94 the workgroup elimination in LDS, K >= 95 the same
on global scratch), nearly decoupled / near-permutation / absorbing transition factors, kappa and nu spread over
eight and six decades, every D at which the step takes another kernel.

Bounds (tests/test_svi_referee.py shows a float64 NumPy restatement of each device formula inside them on the same
inputs; largest device figures of the run that introduced the tests, in units of the bound, in each docstring):
  var_init          max(16, K) eps relative, component-wise          (GTH: O(K eps))
  ltran, mod_init   32 eps max(1, |psi(x)|, |psi(sum)|) absolute     (digamma_d: 5 eps per evaluation)
  step outputs      8 eps scale, scale = sum of |terms| of the element (tests/svi_referee.py)
  ELBO              16 eps sum|terms| of the global lower bound
The factors are uploaded with automatic centring off (debug variant 9 = 1): the loop's state then lives in the
caller's coordinates and what comes back is what the kernels computed, with no host-side shift on top."""
import numpy as np
import pytest

from tests import svi_cases as C
from tests import svi_referee as R

pytestmark = [pytest.mark.gpu,
              pytest.mark.skipif(not R.have_extended_precision(), reason="np.longdouble is not wider than double on this host")]
EPS = R.F64_EPS


def _engine(events=0, theta=None):
    from pysvihmm_amd.engine import HipEngine
    eng = HipEngine(0)
    eng.set_variant("centring", 1)                    # no automatic centring of the resident observations
    if events:
        eng.set_variant("svi_loop", 1)       # stream events instead of device-side counters (k_svi_elbo forms the total)
    if theta is not None:
        eng.set_variant("wide_sweeps", theta)
    return eng


def _begin_globals(family, K, fam="niw", events=0):
    """svi_begin* on a [64, 1] resident array -> (var_tran, var_init, var_init via read_factors, mod_init, ltran):
    svi_begin launches the globals of iteration 0"""
    W = 1 if fam != "cat" else 3
    c = C.step_case(fam, K, W, 0.3, family)
    eng = _engine(events)
    try:
        C.case_begin(eng, c)
        vi2 = eng.svi_read_factors()[1]
        vi = eng.svi_read_state()[1] if fam == "niw" else vi2
        mi, lt = eng.read_globals()
        return c["var_tran"], vi, vi2, mi, lt
    finally:
        eng.close()


def _check_globals(K, family, fam="niw"):
    A, vi, vi2, mi, lt = _begin_globals(family, K, fam)
    np.testing.assert_array_equal(vi, vi2)
    pi = R.stationary(A)
    e_vi = float(np.max(np.abs(R.ld(vi) - pi) / pi)) / EPS
    ltr, lts, mir, mis = R.psi_expectations(A, vi)        # mod_init at the var_init the device returned
    e_lt = R.err_in_bound(lt, ltr, lts, C.PSI_MULT)
    e_mi = R.err_in_bound(mi, mir, mis, C.PSI_MULT)
    print("FIG globals %s K=%d %s [%s]: var_init %.2f eps = %.3f of bound, ltran %.3f, mod_init %.3f of bound"
          % (fam, K, family, C.globals_path(K), e_vi, e_vi / C.gth_bound(K), e_lt, e_mi))
    assert np.all(np.isfinite(vi)) and np.all(vi > 0)
    assert e_vi <= C.gth_bound(K), "var_init: %.3g eps" % e_vi
    assert e_lt <= 1.0, "ltran: %.3g of the bound" % e_lt
    assert e_mi <= 1.0, "mod_init: %.3g of the bound" % e_mi


@pytest.mark.parametrize("K,family", C.globals_cases(), ids=["K%d-%s" % kf for kf in C.globals_cases()])
def test_globals_after_begin(K, family):
    """var_init / ltran / mod_init right after svi_begin.  K <= 64 the wavefront kernel, 65 and 94 the LDS workgroup
    elimination (K - 1 = 64 and 93: lane ownership of the first pivot row on both sides of a wavefront; the K|1 stride,
    the clamped column and the psum double buffer at odd and even K), 95 / 128 / 256 global scratch.  `sink` puts
    psi(~1e-9) ~ -1e9 into mod_init (quirk Q5).
    Largest on the device: var_init 21.2 eps (K = 256, sink: 0.08 of its bound; 0.13 of the bound at K = 17, ring),
    ltran 0.066 of the bound (K = 128, counts), mod_init 0.11 (K = 95, sink).  Before this test existed a read right
    after svi_begin returned the second, never-written var_init slot."""
    _check_globals(K, family)


@pytest.mark.parametrize("fam", ["diag", "cat"])
def test_globals_after_begin_other_families(fam):
    _check_globals(65, "blocks", fam)


@pytest.mark.parametrize("K,family", [(64, "blocks"), (80, "ring"), (100, "counts")])
def test_globals_are_bit_identical_on_stream_events(K, family):
    a = _begin_globals(family, K, events=0)
    b = _begin_globals(family, K, events=1)
    for n, x, y in zip(("var_tran", "var_init", "var_init'", "mod_init", "ltran"), a, b):
        np.testing.assert_array_equal(x, y, err_msg=n)


_CASES = [pytest.param(c, id=C.step_case_id(c)) for c in C.STEP_CASES]


def _run(c, events=0, theta=None):
    from pysvihmm_amd import _lib as L
    eng = _engine(events, theta)
    try:
        recs = C.case_run(eng, c, L.TRANS_WRAP)
        return recs, eng.svi_recoveries()
    finally:
        eng.close()


def _same(c, a, b, what):
    for ra, rb in zip(a, b):
        for x, y in zip(ra["post"], rb["post"]):
            np.testing.assert_array_equal(x, y, err_msg=what)
        if ra["ada_post"] is not None:
            np.testing.assert_array_equal(ra["ada_post"], rb["ada_post"], err_msg=what)
        assert ra["elbo"] == rb["elbo"], (what, ra["elbo"], rb["elbo"])


@pytest.mark.parametrize("case", _CASES)
def test_global_step_and_elbo(case):
    """One svi_iteration (two with AdaGrad) per case: the state after it against the referee's step fed the state
    before, the packed statistics the step consumed (read_packed, before anything overwrites them) and the same
    scalars; svi_read_elbo against lb (the last packed entry) + the referee's global lower bound of the state read
    back.  NIW D = 17 .. 32 takes the merged k_svi_step_theta32s, the other D k_svi_global_step; K = 1 / 64 / 65 / 130
    walk the 64-lane groups of the ELBO tail; `blocks` puts 2.5e-3 next to 1e6 in var_tran, `sink` (empty shard: no
    sweeps from its globals) 1e8.  The stream-event loop (k_svi_elbo instead of the tail of k_svi_vlb) must give the
    same state and ELBO bit for bit, the separate step + theta kernels (variant 13 = 3) at D = 32 as well (they
    did not at K = 64, D = 32, rho = 1 -- 12 % of mu' one ulp apart -- until both kernels took the blend from
    svi_niw_* with contraction off).
    Largest on the device, in units of the bound: sigma 0.29 and mu 0.27 (NIW K = 80, D = 96, rho = 0.3), var_tran
    0.22, nu 0.15, kappa 0.13, ada_G 0.11 (NIW K = 65, D = 17, AdaGrad), betas 0.20 (diagonal K = 65, D = 128, blocks),
    nus 0.12, alphas 0.11, Categorical alpha 0.16 (K = 130, sink); ELBO 0.099 (NIW K = 3, D = 64, rho = 1)."""
    c = C.step_case(*case)
    recs, nrec = _run(c)
    assert nrec == 0 and len(recs) == c["nit"]
    worst = {}
    for it, rec in enumerate(recs):
        ref, glb = C.case_reference(c, rec)
        errs = R.step_errors(C.case_got(c, rec), ref, C.STEP_MULT)
        e_elbo = C.elbo_error(rec["elbo"], rec["packed"].lb[0], glb)
        print("FIG step %s it %d: %s ELBO %.4f of bound (elbo %.10g, sum|terms| %.3g)"
              % (C.step_case_id(case), it, {n: round(v, 3) for n, v in errs.items()}, e_elbo, rec["elbo"], float(glb[1])))
        worst[it] = (errs, e_elbo)
        assert np.isfinite(rec["elbo"])
    for it, (errs, e_elbo) in worst.items():
        assert max(errs.values()) <= 1.0, (it, errs)
        assert e_elbo <= 1.0, (it, e_elbo)
    ev, _ = _run(c, events=1)
    _same(c, recs, ev, "stream-event loop")
    if c["fam"] == "niw" and c["D"] == 32:
        sep, _ = _run(c, theta=3)
        _same(c, recs, sep, "separate step and theta kernels")


@pytest.mark.parametrize("K", [80, 94])
def test_lds_workgroup_globals_end_to_end(K):
    """Three iterations against the oracle engine in the style (and at the tolerances) of
    test_gpu_classes.py::test_svi_iteration_engine_level, at two K of the LDS workgroup elimination: the sweeps of
    every iteration are gated on its globals."""
    from oracle.engine import OracleEngine
    from pysvihmm_amd.engine import HipEngine
    from pysvihmm_amd.distributions import niw_prior_logpart
    from pysvihmm_amd import _lib as L
    from tests.helpers import make_problem
    D, B, Lm, T = 3, 6, 17, 4000
    pb = make_problem(K, D, T, seed=K + D, miss=0.05)
    rng = np.random.default_rng(K)
    prior_tran = 1.0 + rng.random((K, K))
    mu0 = np.tile(pb["obs"].mean(0), (K, 1)) + 0.1 * rng.normal(size=(K, D))
    sg0 = np.tile(0.75 * np.cov(pb["obs"].T).reshape(D, D), (K, 1, 1))
    ka0, nu0 = np.full(K, 0.01), np.full(K, D + 2.0)
    bA, bE = (T - 2 * 8 - 1) / (2. * 8 * B), (T - 2 * 8 - 1) / ((2. * 8 + 1) * B)
    res = []
    for eng in (HipEngine(0), OracleEngine()):
        try:
            eng.set_obs(pb["obs"], pb["mask"])
            eng.svi_begin(prior_tran, pb["var_tran"], (mu0, sg0, ka0, nu0),
                          (pb["mu"], pb["sigma"], pb["kappa"], pb["nu"]), niw_prior_logpart(sg0, nu0), 3, 1.0)
            r2 = np.random.default_rng(5)
            for it in range(3):
                eng.svi_iteration(it, r2.integers(0, T - Lm, size=B), B, Lm, L.TRANS_WRAP, (it + 1.0) ** -0.7, bA, bE)
            elbo = eng.svi_read_elbo(3)[0]
            res.append((eng.svi_read_state(), elbo))
        finally:
            eng.close()
    (sa, ea), (sb, eb) = res
    for n, a, b in zip(("var_tran", "var_init", "mu", "sigma", "kappa", "nu"), sa, sb):
        np.testing.assert_allclose(a, b, rtol=1e-6, atol=1e-9, err_msg=n)
    np.testing.assert_allclose(ea, eb, rtol=1e-9)
