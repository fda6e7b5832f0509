"""The extended-precision referee of the resident SVI loop's global kernels (tests/svi_referee.py) is right, and the
bounds tests/test_gpu_svi_globals.py holds the device to are attainable in float64: a NumPy restatement of every device
formula passes the same bounds on the same inputs.  CPU only."""
import mpmath as mp
import numpy as np
import pytest

from tests import svi_cases as C
from tests import svi_referee as R

pytestmark = pytest.mark.skipif(not R.have_extended_precision(),
                                reason="np.longdouble is not wider than double on this host")
EPS = R.F64_EPS


def _rel_ld_mp(ld, mpv, dps=60):
    with mp.workdps(dps):
        return max(float(abs(R.mpf_ld(a) - b) / b) for a, b in zip(ld, mpv))


@pytest.mark.parametrize("K", [2, 3, 17, 64, 65])
def test_stationary_longdouble_against_60_digit_gth(K):
    """<= 1e-18 relative, component-wise, on all five matrix families (measured: 5.7e-19 at K = 64, sink)."""
    for fam in R.FAMILIES:
        A = R.tran_family(fam, K)
        err = _rel_ld_mp(R.stationary(A), R.stationary_mp(A))
        print("K=%d %s: %.2e" % (K, fam, err))
        assert err <= 1e-18, (fam, err)


@pytest.mark.parametrize("K", [2, 3, 17, 64, 65, 100])
def test_stationary_against_the_eig_oracle_on_well_coupled_chains(K):
    from oracle import ref_numpy as O
    A = R.tran_family("counts", K)
    pi = R.stationary(A)
    assert abs(float(np.sum(pi * pi)) - 1.0) < 1e-15
    err = float(np.max(np.abs(R.ld(O.stationary_init(A)) - pi) / pi))
    assert err <= 1e-12, err


def test_eig_oracle_cannot_referee_nearly_decoupled_chains():
    """Why this referee exists: on the `blocks` family np.linalg.eig's Perron vector is 1e-9 .. 1e-7 off
    component-wise while float64 GTH stays within a few eps -- the eig route is a valid referee for the stationary
    vector on well-coupled chains only."""
    from oracle import ref_numpy as O
    for K in (3, 17, 64):
        A = R.tran_family("blocks", K)
        pi = R.stationary(A)
        eig = float(np.max(np.abs(R.ld(O.stationary_init(A)) - pi) / pi))
        gth = float(np.max(np.abs(R.ld(R.stationary_f64(A)) - pi) / pi))
        print("K=%d: eig %.2e, float64 GTH %.1f eps" % (K, eig, gth / EPS))
        assert eig > 1e-10 and gth <= C.gth_bound(K) * EPS


def test_digamma_restatement_against_mpmath():
    """digamma_d (device_helpers.h: recurrence to x >= 10, asymptotic series) as restated in float64: the per-evaluation
    error the ltran / mod_init bound is built on.  Measured 5.0 eps max(1, |psi|) on this grid (1e-9 .. 1e10, dense on
    [0.9, 11], the root at 1.4616.., both sides of the x = 10 switch); the bound of the globals test is
    32 eps = two evaluations + a subtraction with 3x headroom."""
    xs = np.concatenate([10.0 ** np.linspace(-9, 10, 2000), np.linspace(0.9, 11, 3000),
                         1.4616321449683623 + np.linspace(-1e-3, 1e-3, 101), 10 + np.linspace(-1e-6, 1e-6, 101),
                         [np.nextafter(10.0, 0.0), 10.0, np.nextafter(10.0, 20.0)]])
    d = R.digamma_f64(xs)
    with mp.workdps(30):
        err = max(float(abs(mp.mpf(float(a)) - mp.digamma(mp.mpf(float(x)))) / max(1, abs(mp.digamma(mp.mpf(float(x))))))
                  for a, x in zip(d, xs))
    print("digamma_f64: %.2f eps" % (err / EPS))
    assert err <= 8 * EPS


@pytest.mark.parametrize("K", C.GTH_KS)
def test_float64_globals_restatement_passes_the_gpu_bounds(K):
    """GTH with reciprocal-then-multiply and the digamma_d recurrence, float64 NumPy, on the inputs of check (a):
    var_init within max(16, K) eps, ltran and mod_init within 32 eps max(1, |psi(x)|, |psi(sum)|)."""
    for k, fam in C.globals_cases():
        if k != K:
            continue
        A = R.tran_family(fam, K)
        pi = R.stationary(A)
        vi = R.stationary_f64(A)
        e_vi = float(np.max(np.abs(R.ld(vi) - pi) / pi)) / EPS
        lt, ls, mi, ms = R.psi_expectations(A, vi)
        g = R.digamma_f64((A + R.SVI_EPS).ravel()).reshape(K, K) - R.digamma_f64(A.sum(axis=1) + R.SVI_EPS)[:, None]
        gm = R.digamma_f64(vi + R.SVI_EPS) - R.digamma_f64(np.array([vi.sum() + R.SVI_EPS]))
        e_lt = R.err_in_bound(g, lt, ls, C.PSI_MULT)
        e_mi = R.err_in_bound(gm, mi, ms, C.PSI_MULT)
        print("K=%d %s: var_init %.1f eps (bound %g), ltran %.3f, mod_init %.3f of bound" % (K, fam, e_vi, C.gth_bound(K), e_lt, e_mi))
        assert e_vi <= C.gth_bound(K) and e_lt <= 1.0 and e_mi <= 1.0


def test_mpmath_and_longdouble_factorisations_agree():
    """niw_vlb factors sigma in mpmath up to D = 8 and in longdouble beyond: at D = 8 both routes give the same
    term to 1e-17 of its scale."""
    c = C.step_case("niw", 3, 8, 0.3, "counts")
    mu, sg, ka, nu = c["factors"]
    mu0, sg0, ka0, nu0 = c["prior"]
    for k in range(3):
        a = R.niw_vlb(mu[k], sg[k], ka[k], nu[k], mu0[k], sg0[k], ka0[k], nu0[k], use_mp=True)
        b = R.niw_vlb(mu[k], sg[k], ka[k], nu[k], mu0[k], sg0[k], ka0[k], nu0[k], use_mp=False)
        assert abs(a[0] - b[0]) <= 1e-17 * a[1] and abs(a[1] - b[1]) <= 1e-15 * a[1]


def test_vlb_referee_against_the_host_classes_on_mild_inputs():
    """global_lower_bound_* pieces against distributions.*.get_vlb / ref_numpy.dirichlet_lower_bound (float64 host
    code) on mild parameters, at that code's accuracy."""
    from oracle import ref_numpy as O
    from pysvihmm_amd.distributions import Categorical, DiagonalGaussian, Gaussian
    rng = np.random.default_rng(3)
    K, D = 4, 3
    p, q = 1.0 + rng.random((K, K)), 1.0 + 20.0 * rng.random((K, K))
    v, a = R.dirichlet_rows(p, q)
    assert abs(float(v) - O.dirichlet_lower_bound(p, q)) <= 64 * EPS * float(a)
    A = rng.normal(size=(D, D)); sg = A @ A.T + D * np.eye(D)
    B = rng.normal(size=(D, D)); sg0 = B @ B.T + D * np.eye(D)
    mu, mu0 = rng.normal(size=D), rng.normal(size=D)
    for conv, zs in (("pybasicbayes", 1.0), ("bishop", -1.0)):
        g = Gaussian(mu=mu, sigma=np.eye(D), mu_0=mu0, sigma_0=sg0, kappa_0=0.3, nu_0=D + 2.5)
        g.mu_mf, g.sigma_mf, g.kappa_mf, g.nu_mf = mu, sg, 4.2, D + 9.0
        v, a = R.niw_vlb(mu, sg, 4.2, D + 9.0, mu0, sg0, 0.3, D + 2.5, zsign=zs)
        assert abs(float(v) - g.get_vlb(conv)) <= 64 * EPS * float(a)
    # -KL(q || prior) vanishes at the prior (Bishop's sign)
    v, a = R.niw_vlb(mu0, sg0, 0.3, D + 2.5, mu0, sg0, 0.3, D + 2.5, zsign=-1.0)
    assert abs(float(v)) <= 1e-25 * float(a)
    m, nu, al, be = rng.normal(size=D), 0.5 + rng.random(D), 1.0 + 3 * rng.random(D), 0.5 + rng.random(D)
    m0, nu0, al0, be0 = rng.normal(size=D), 0.5 + rng.random(D), 1.0 + rng.random(D), 0.5 + rng.random(D)
    g = DiagonalGaussian(mu=m, sigmas=np.ones(D), mu_0=m0, nus_0=nu0, alphas_0=al0, betas_0=be0)
    g._set_mf(m, nu, al, be)
    v, a = R.diag_vlb(m, nu, al, be, m0, nu0, al0, be0)
    assert abs(float(v) - g.get_vlb()) <= 64 * EPS * float(a)
    al, al0 = 0.2 + 5 * rng.random(6), 0.5 + rng.random(6)
    v, a = R.cat_vlb(al, al0)
    assert abs(float(v) - Categorical(weights=np.full(6, 1 / 6.), alphav_0=al0, alpha_mf=al).get_vlb()) <= 64 * EPS * float(a)


_CASES = [pytest.param(c, id=C.step_case_id(c)) for c in C.STEP_CASES]


@pytest.mark.parametrize("case", _CASES)
def test_float64_step_and_elbo_restatements_pass_the_gpu_bounds(case):
    """Every case of checks (b) and (c), on the host: the statistics come from the oracle engine's E-step; its
    global step and ELBO (oracle.engine.OracleEngine.svi_iteration: NumPy float64, scipy's digamma / gammaln,
    LAPACK solves) and the float64 restatements of the device's expressions (k_svi_global_step_body / _simple_body,
    svi_tran_step, k_svi_vlb_body / k_svi_vlb_simple_body, svi_rowterm, k_svi_elbo_body) are both held to the bounds
    the device is held to: 8 eps scale per output element of the step, 16 eps sum|terms| for the ELBO."""
    from oracle.engine import OracleEngine
    from pysvihmm_amd import _lib as L
    c = C.step_case(*case)
    recs = C.case_run(OracleEngine(), c, L.TRANS_WRAP)
    assert len(recs) == c["nit"]
    for it, rec in enumerate(recs):
        ref, glb = C.case_reference(c, rec)
        for who, got, elbo in (("oracle engine", C.case_got(c, rec), rec["elbo"]),
                               ("float64 restatement", C.case_step_f64(c, rec), C.elbo_f64_of(c, rec))):
            errs = R.step_errors(got, ref, C.STEP_MULT)
            e_elbo = C.elbo_error(elbo, rec["packed"].lb[0], glb)
            print("it %d, %s: step %s, ELBO %.4f of bound (sum|terms| %.3g)"
                  % (it, who, {n: round(v, 3) for n, v in errs.items()}, e_elbo, float(glb[1])))
            assert set(errs) == set(ref) and max(errs.values()) <= 1.0, (who, errs)
            assert e_elbo <= 1.0, (who, e_elbo)


def test_referee_scales_see_the_cancellation_in_sigma():
    """sigma' = e3 - kappa' mu' mu'': with a mean far from the origin the terms are ~kappa |mu|^2 while sigma' stays
    O(1) -- the scale must follow the terms, not the result (a flat rtol on sigma' would either fail a correct
    float64 step or hide a wrong one)."""
    c = C.step_case("niw", 3, 2, 0.3, "counts")
    mu, sg, ka, nu = c["factors"]
    from oracle.engine import OracleEngine
    from pysvihmm_amd import _lib as L
    rec = C.case_run(OracleEngine(), c, L.TRANS_WRAP)[0]
    far = (rec["pre"][0], mu + 1e4) + tuple(rec["pre"][2:])
    ref = R.global_step_niw(far, C.prior_tuple(c), rec["packed"], 0.3, c["bA"], c["bE"], c["B"])
    val, scale = ref["sigma"]
    assert float(np.min(scale / np.maximum(np.abs(val), 1e-300))) > 1.0
    assert float(np.max(scale)) > 1e6 * float(np.max(np.abs(R.global_step_niw(*((rec["pre"], C.prior_tuple(c), rec["packed"], 0.3, c["bA"], c["bE"], c["B"])))["sigma"][0])))
    got = R.global_step_niw_f64(far, C.prior_tuple(c), rec["packed"], 0.3, c["bA"], c["bE"], c["B"])
    assert max(R.step_errors(got, ref, C.STEP_MULT).values()) <= 1.0
