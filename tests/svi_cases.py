"""The cases of tests/test_gpu_svi_globals.py and the driver that runs them on an engine with the HipEngine protocol
(HipEngine, OracleEngine), shared with the float64 restatements of tests/test_svi_referee.py.  The referee itself is
tests/svi_referee.py.  Only tests import this module."""
import mpmath as mp
import numpy as np

from tests.svi_referee import (FAMILIES, F64_EPS, tran_family, step_errors, global_step_niw, global_step_diag,
                               global_step_cat, global_step_niw_f64, global_step_diag_f64, global_step_cat_f64,
                               global_lower_bound_niw, global_lower_bound_diag, global_lower_bound_cat, rowterms_f64,
                               niw_vlb_f64, diag_vlb_f64, cat_vlb_f64, elbo_f64)


# ---------------------------------------------------------------------------------------------------
#  the cases of tests/test_gpu_svi_globals.py, shared with the float64 restatements of tests/test_svi_referee.py
# ---------------------------------------------------------------------------------------------------
GTH_KS = (1, 2, 3, 17, 63, 64, 65, 94, 95, 128, 256)
PSI_MULT, STEP_MULT, ELBO_MULT = 32.0, 8.0, 16.0
T_OBS, B_WIN, L_WIN = 64, 6, 17


def gth_bound(K):
    """component-wise relative bound on var_init in units of eps: GTH's error is O(K eps)"""
    return float(max(16, K))


def globals_path(K):
    """which of the three GTH implementations svi_globals() (svihmm_hip.hip) picks"""
    if K <= 64:
        return "wave/registers"
    return "workgroup/LDS" if 2 * K * (K | 1) * 8 + 9 * 1024 <= 150 * 1024 else "workgroup/global scratch"


def globals_cases():
    """(K, family) of check (a); the degenerate families are skipped at K = 1"""
    return [(K, f) for K in GTH_KS for f in FAMILIES if K > 1 or f in ("counts", "minimal")]


def prior_tran_for(K, seed=0):
    return 1.0 + np.random.default_rng(77 + 13 * K + seed).random((K, K))


def _spd(rng, D, lo, hi):
    """random SPD matrix with eigenvalues log-spaced in [lo, hi] (condition number hi / lo <= 100)"""
    Q, _ = np.linalg.qr(rng.normal(size=(D, D)))
    A = (Q * np.exp(np.linspace(np.log(lo), np.log(hi), D))) @ Q.T
    return 0.5 * (A + A.T)


# (family, K, W, rho, var_tran family, options)   W = D (niw, diag) or V (cat)
STEP_CASES = [
    ("niw", 3, 1, 1.0, "counts", ""), ("niw", 3, 16, 0.3, "counts", ""), ("niw", 3, 17, 1.0, "counts", ""),
    ("niw", 3, 32, 1e-8, "counts", ""), ("niw", 3, 33, 0.3, "counts", ""), ("niw", 3, 64, 1.0, "counts", ""),
    ("niw", 3, 96, 1e-8, "counts", ""),
    ("niw", 64, 1, 0.3, "counts", ""), ("niw", 64, 17, 0.3, "counts", ""), ("niw", 64, 32, 1.0, "counts", ""),
    ("niw", 80, 16, 1e-8, "counts", ""), ("niw", 80, 33, 1.0, "counts", ""), ("niw", 80, 96, 0.3, "counts", ""),
    ("niw", 80, 32, 0.3, "counts", ""), ("niw", 64, 64, 1e-8, "counts", ""),
    ("niw", 1, 2, 0.3, "counts", ""), ("niw", 65, 3, 0.3, "counts", ""), ("niw", 130, 2, 0.3, "counts", ""),
    ("niw", 64, 2, 0.3, "blocks", ""), ("niw", 65, 17, 0.3, "blocks", ""),
    ("niw", 3, 2, 0.3, "counts", "empty"), ("niw", 65, 2, 1e-8, "sink", "empty"),
    ("niw", 3, 2, 0.3, "counts", "adagrad"), ("niw", 65, 17, 0.3, "counts", "adagrad"),
    ("diag", 3, 1, 1.0, "counts", ""), ("diag", 64, 65, 0.3, "counts", ""), ("diag", 65, 128, 1e-8, "blocks", ""),
    ("diag", 3, 5, 0.3, "counts", "adagrad"),
    ("cat", 3, 2, 1.0, "counts", ""), ("cat", 64, 65, 0.3, "blocks", ""), ("cat", 3, 300, 1e-8, "counts", ""),
    ("cat", 130, 7, 0.3, "sink", "empty"),
]


def step_case_id(c):
    return "%s-K%d-W%d-rho%g-%s%s" % (c[0], c[1], c[2], c[3], c[4], ("-" + c[5]) if c[5] else "")


def step_case(fam, K, W, rho, tran, opts=""):
    """Everything one global-step / ELBO case needs: a benign problem on T_OBS resident rows, B_WIN windows of L_WIN
    rows, factors whose kappa spans 1e-2 .. 1e6 and nu D + 2 .. 1e6 across the states (sigma scaled with nu so that
    the expected precision stays benign), priors with condition number <= 30."""
    from tests.helpers import make_problem
    rng = np.random.default_rng(1000 * K + W + (7 if fam == "diag" else 19 if fam == "cat" else 0))
    D = 1 if fam == "cat" else W
    pb = make_problem(K, D, T_OBS, seed=K + W)
    c = dict(fam=fam, K=K, W=W, D=D, rho=float(rho), opts=opts, tran=tran, obs=pb["obs"], mask=None,
             var_tran=tran_family(tran, K), prior_tran=prior_tran_for(K), nit=2 if "adagrad" in opts else 1,
             B=B_WIN, Lm=L_WIN, bA=(4000 - 17.0) / (16.0 * B_WIN), bE=(4000 - 17.0) / (17.0 * B_WIN))
    r2 = np.random.default_rng(5 + K)
    c["starts"] = [r2.integers(0, T_OBS - L_WIN, size=B_WIN) for _ in range(c["nit"])]
    if "empty" in opts:
        c["starts"] = [s[:0] for s in c["starts"]]
    lin = lambda lo, hi: rng.permutation(np.linspace(lo, hi, K)) if K > 1 else np.array([0.5 * (lo + hi)])
    if fam == "niw":
        kappa = 10.0 ** lin(-2.0, 6.0)
        nu = D + 2.0 + (10.0 ** lin(0.0, 6.0) - 1.0)
        base = np.stack([_spd(rng, D, 1.0, 30.0) for _ in range(K)])
        sigma = base * (nu - D - 1.0)[:, None, None]
        mu0 = 0.3 * rng.normal(size=(K, D))
        sg0 = np.stack([_spd(rng, D, 0.5, 15.0) for _ in range(K)])
        c["factors"] = (pb["mu"], sigma, kappa, nu)
        c["prior"] = (mu0, sg0, 0.01 + rng.random(K), D + 2.0 + 3.0 * rng.random(K))
    elif fam == "diag":
        c["factors"] = (pb["mu"], 10.0 ** rng.uniform(-2, 4, size=(K, D)), 1.0 + 10.0 ** rng.uniform(0, 4, size=(K, D)),
                        None)
        al = c["factors"][2]
        c["factors"] = c["factors"][:3] + (al * rng.uniform(0.5, 2.0, size=(K, D)),)     # E sigma^2 ~ 1
        c["prior"] = (0.3 * rng.normal(size=(K, D)), 0.01 + rng.random((K, D)), 1.0 + rng.random((K, D)),
                      0.5 + rng.random((K, D)))
    else:
        V = W
        c["obs"] = rng.integers(0, V, size=(T_OBS, 1)).astype(np.float64)
        c["factors"] = 0.05 + rng.gamma(0.5, 20.0, size=(K, V))
        # (>= 1: every window contributes alpha_0 - 1, hmmsgd_metaobs.py:1071-1084 -- a sparser prior drives the
        #  factors of rarely visited states below zero, where no Dirichlet lives)
        c["prior"] = 1.0 + rng.random((K, V))
    return c


def case_begin(eng, c):
    """set_obs + svi_begin* of a case on an engine with the HipEngine protocol (HipEngine, OracleEngine)"""
    from pysvihmm_amd.distributions import niw_prior_logpart
    eng.set_obs(c["obs"], c["mask"])
    if c["fam"] == "niw":
        eng.svi_begin(c["prior_tran"], c["var_tran"], c["prior"], c["factors"],
                      niw_prior_logpart(c["prior"][1], c["prior"][3]), 2, 1.0)
    elif c["fam"] == "diag":
        eng.svi_begin_diag(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], 2)
    else:
        eng.svi_begin_cat(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], 2)
    if "adagrad" in c["opts"]:
        eng.svi_set_adagrad(np.ones((c["K"], c["K"])))


def state_tuple(c, var_tran, fac):
    return (var_tran,) + (tuple(fac) if c["fam"] != "cat" else (fac,))


def prior_tuple(c):
    return (c["prior_tran"],) + (tuple(c["prior"]) if c["fam"] != "cat" else (c["prior"],))


STEP_REF = {"niw": global_step_niw, "diag": global_step_diag, "cat": global_step_cat}
STEP_F64 = {"niw": global_step_niw_f64, "diag": global_step_diag_f64, "cat": global_step_cat_f64}
GLB_REF = {"niw": global_lower_bound_niw, "diag": global_lower_bound_diag, "cat": global_lower_bound_cat}
FACTOR_NAMES = {"niw": ("mu", "sigma", "kappa", "nu"), "diag": ("mu", "nus", "alphas", "betas"), "cat": ("alpha",)}


def got_dict(c, var_tran, fac, ada_G=None):
    d = {"var_tran": var_tran}
    d.update(zip(FACTOR_NAMES[c["fam"]], fac if c["fam"] != "cat" else (fac,)))
    if ada_G is not None:
        d["ada_G"] = ada_G
    return d


def elbo_error(got, lb, glb):
    """|got - (lb + glb)| in units of ELBO_MULT * eps * sum|terms| (sum|terms| of the global lower bound alone)"""
    v, a = glb
    with mp.workdps(40):
        want = mp.mpf(float(lb)) + v
        return float(abs(mp.mpf(float(got)) - want) / (ELBO_MULT * F64_EPS * a))


def case_run(eng, c, flags):
    """svi_begin + the case's iterations on ``eng``; per iteration the state before (what the step consumed), the
    packed statistics it consumed (read before anything overwrites them), the state after, the AdaGrad accumulator
    before / after and the ELBO entry.  The state before iteration 0 is what was uploaded (float64, unchanged)."""
    case_begin(eng, c)
    fam = c["fam"]
    pre = state_tuple(c, c["var_tran"], c["factors"])
    ada = np.ones((c["K"], c["K"])) if "adagrad" in c["opts"] else None
    recs = []
    for it in range(c["nit"]):
        eng.svi_iteration(it, c["starts"][it], c["B"], c["Lm"], flags, c["rho"], c["bA"], c["bE"])
        packed = eng.read_packed()
        if fam == "niw":
            s = eng.svi_read_state()
            vt, vi, fac = s[0], s[1], s[2:]
        else:
            vt, vi, fac = eng.svi_read_factors()
        post = state_tuple(c, vt, fac)
        ada_post = eng.svi_read_adagrad() if ada is not None else None
        elbo = eng.svi_read_elbo(it + 1)[0][it]
        recs.append(dict(pre=pre, packed=packed, post=post, ada_pre=ada, ada_post=ada_post, elbo=float(elbo),
                         var_init=vi))
        pre, ada = post, ada_post
    return recs


def case_reference(c, rec):
    """(referee step outputs {name: (value, scale)}, (global lower bound, sum|terms|) of the record's post-state)"""
    fam = c["fam"]
    ref = STEP_REF[fam](rec["pre"], prior_tuple(c), rec["packed"], c["rho"], c["bA"], c["bE"], c["B"],
                        ada_G=rec["ada_pre"])
    return ref, GLB_REF[fam](rec["post"], prior_tuple(c))


def case_got(c, rec):
    """the record's own post-state as the dict ``step_errors`` takes"""
    return got_dict(c, rec["post"][0], rec["post"][1:] if c["fam"] != "cat" else rec["post"][1], rec["ada_post"])


def case_step_f64(c, rec):
    """the float64 restatement of the device's step, fed the record's pre-state and statistics"""
    return STEP_F64[c["fam"]](rec["pre"], prior_tuple(c), rec["packed"], c["rho"], c["bA"], c["bE"], c["B"],
                              ada_G=rec["ada_pre"])


def elbo_f64_of(c, rec):
    """the device's ELBO assembly in float64 from the record's post-state and lb"""
    from pysvihmm_amd.distributions import niw_prior_logpart
    fam, post = c["fam"], rec["post"]
    rowterm, pc = rowterms_f64(c["prior_tran"], post[0])
    if fam == "niw":
        pr = c["prior"]
        vlb = niw_vlb_f64(*(tuple(post[1:]) + tuple(pr) + (niw_prior_logpart(pr[1], pr[3]), 1.0)))
    elif fam == "diag":
        vlb = diag_vlb_f64(post[1:], c["prior"])
    else:
        vlb = cat_vlb_f64(post[1], c["prior"])
    return elbo_f64(rec["packed"].lb[0], vlb, rowterm, pc)
