"""GPU: the eleven entry points that put an emission family in force -- six svihmm_set_emission_* and five
svihmm_svi_begin* -- as one table of argument refusals and one matrix of loop endings.

Part 1, refusals.  Every argument refusal that can be reached through the C ABI, with its full text written out here
(copied from the source of the commit before these entry points began to share their checks, and run against that
commit's library once: the texts are part of the ABI).  Each refusal is raised on a handle that has a family in
force; a loglik of the tiny batch taken after it is bit-identical to the one taken before.  The order of the cases of
one entry point follows the order of its checks, and a case whose arguments would fail a later check as well says
which refusal wins.

Part 2, loop endings.  For each of the five loop families L and each of the six setters S: begin L, run two
iterations on the device-side counters (the second iteration's ELBO kernels are deferred), call S.
  S re-pushes L's own family and shape: the loop lives -- the next iteration runs and svi_read_elbo(3) is finite.
  anything else: svi_iteration refuses, sync() lets the side streams drain, and a loglik under S agrees with a fresh
  handle that only did set_obs + S.  Not bitwise: a Gaussian family that arrives after a table family takes its
  centre from column means formed on the device.  rtol 1e-6 / atol 1e-8, the whole-buffer tolerance of
  tests/test_gpu_family_switch.py::test_family_b_after_family_a.

Shapes: K = 3, D = 2, T = 200 rows of small non-negative integers (column 0 in {0, 1}, column 1 in {0..4}), which
every family reads: reals, symbols of the columns V = (2, 5) and counts below C = 10 alike.  The Categorical family
reads column 0 alone.  Windows B = 3, Lm = 17; maxit = 4."""
import ctypes
import re

import numpy as np
import pytest

from pysvihmm_amd import _lib as L

pytestmark = pytest.mark.gpu

K, D, T, B, LM, MAXIT, C = 3, 2, 200, 3, 17, 4, 10
VS = (2, 5)
F = sum(VS)
STARTS = np.array([0, 60, 150], dtype=np.int64)
FAMILIES = ("niw", "diag", "cat", "mcat", "poisson", "pgauss")
LOOPS = FAMILIES[:5]


def _problem():
    rng = np.random.default_rng(77)
    p = {}
    p["x"] = np.stack([rng.integers(0, VS[0], size=T), rng.integers(0, VS[1], size=T)], axis=1).astype(np.float64)
    p["mod_init"] = np.log(rng.dirichlet(np.ones(K)))
    p["ltran"] = np.log(rng.dirichlet(np.ones(K) * 3.0, size=K))
    p["prior_tran"] = 1.0 + rng.random((K, K))
    p["var_tran"] = 1.0 + 10.0 * rng.random((K, K))
    A = rng.normal(size=(K, D, D))
    p["niw"] = (1.0 + rng.normal(size=(K, D)), np.einsum("kij,klj->kil", A, A) + 2.0 * np.eye(D), 0.5 + rng.random(K),
                D + 2.0 + 3.0 * rng.random(K))
    p["niw0"] = (np.ones((K, D)), np.tile(np.eye(D), (K, 1, 1)), np.full(K, 0.1), np.full(K, D + 2.0))
    p["diag"] = tuple(np.ascontiguousarray(a) for a in
                      (1.0 + rng.normal(size=(K, D)), 0.5 + rng.random((K, D)), 2.0 + rng.random((K, D)), 1.0 + rng.random((K, D))))
    p["diag0"] = (np.ones((K, D)), np.full((K, D), 0.1), np.full((K, D), 2.0), np.full((K, D), 1.0))
    p["cat"] = np.log(rng.dirichlet(np.ones(VS[0]), size=K))                      # logp [K, V]
    p["cat_a"], p["cat_a0"] = 1.0 + 5.0 * rng.random((K, VS[0])), np.full((K, VS[0]), 1.5)
    p["mcat"] = [np.log(rng.dirichlet(np.ones(v), size=K)) for v in VS]
    p["mcat_a"], p["mcat_a0"] = [1.0 + 5.0 * rng.random((K, v)) for v in VS], [np.full((K, v), 1.5) for v in VS]
    p["pois_ab"] = (1.0 + 4.0 * rng.random((K, D)), 1.0 + rng.random((K, D)))
    p["pois_ab0"] = (np.full((K, D), 2.0), np.full((K, D), 0.5))
    p["pois"] = (np.log(p["pois_ab"][0] / p["pois_ab"][1]), p["pois_ab"][0] / p["pois_ab"][1])      # elog, erate
    p["pg"] = (1.0 + rng.normal(size=(K, D)), -0.5 - rng.random((K, D)), -1.0 - rng.random((K, D)))   # mu, hprec, cst
    p["origin"] = np.array([0.5, 2.0])
    return p


P = _problem()


def _obs(name):
    return np.ascontiguousarray(P["x"][:, :1]) if name.startswith("cat") else P["x"]


def _set(e, name):
    """The setter of family ``name`` with the module's shapes (``cat3`` / ``mcat35``: the family in another shape)."""
    if name == "niw":
        e.set_emission_niw(*P["niw"])
    elif name == "diag":
        e.set_emission_diag(*P["diag"])
    elif name == "cat":
        e.set_emission_cat(P["cat"])
    elif name == "cat3":
        e.set_emission_cat(np.log(np.full((K, 3), 1.0 / 3.0)))
    elif name == "mcat":
        e.set_emission_mcat(P["mcat"])
    elif name == "mcat35":
        e.set_emission_mcat([np.log(np.full((K, 3), 1.0 / 3.0)), P["mcat"][1]])
    elif name == "poisson":
        e.set_emission_poisson(P["pois"][0], P["pois"][1], C)
    else:
        e.set_emission_pgauss(*P["pg"], origin=P["origin"])


def _begin(e, name):
    pt, vt = P["prior_tran"], P["var_tran"]
    if name == "niw":
        e.svi_begin(pt, vt, P["niw0"], P["niw"], np.zeros(K), MAXIT)
    elif name == "diag":
        e.svi_begin_diag(pt, vt, P["diag0"], P["diag"], MAXIT)
    elif name == "cat":
        e.svi_begin_cat(pt, vt, P["cat_a0"], P["cat_a"], MAXIT)
    elif name == "mcat":
        e.svi_begin_mcat(pt, vt, P["mcat_a0"], P["mcat_a"], MAXIT)
    else:
        e.svi_begin_poisson(pt, vt, P["pois_ab0"], P["pois_ab"], C, MAXIT)


def _engine():
    from pysvihmm_amd.engine import HipEngine
    return HipEngine(0)


# ---------------------------------------------------------------------------------------------------
#  1. the refusal table
# ---------------------------------------------------------------------------------------------------
_keep = []                       # (the arrays behind the pointers of the cases below)


def dp(a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    _keep.append(a)
    return L.dptr(a)


def ip(a):
    a = np.ascontiguousarray(a, dtype=np.int32)
    _keep.append(a)
    return a.ctypes.data_as(ctypes.POINTER(ctypes.c_int32))


def _with(a, idx, v):
    a = np.array(a, dtype=np.float64)
    a[idx] = v
    return a


PT, VT = P["prior_tran"], P["var_tran"]
HOST = "evaluate the expected log-likelihoods on the host and pass them with svihmm_set_lliks / SVIHMM_USE_HOST_LLIKS"
PSEUDO = ("svihmm_svi_begin: prior_tran below 1 or var_tran below SVIHMM_SVI_MIN_PSEUDOCOUNT may need the log-domain "
          "recursion mid-loop: run the loop through svihmm_set_globals + svihmm_estep_minibatch")
LOW_VT = _with(VT, (1, 2), 1e-3)
LOW_PT = _with(PT, (0, 1), 0.5)


def _niw(h, k=K, d=D, a=None):
    mu, sg, ka, nu = a or [dp(x) for x in P["niw"]]
    return lambda lib: lib.svihmm_set_emission_niw(h, k, d, mu, sg, ka, nu)


def _diag(h, k=K, d=D, a=None):
    mu, nus, al, be = a or [dp(x) for x in P["diag"]]
    return lambda lib: lib.svihmm_set_emission_diag(h, k, d, mu, nus, al, be)


def _cat(h, k=K, v=VS[0], null=False):
    lp = None if null else dp(P["cat"])
    return lambda lib: lib.svihmm_set_emission_cat(h, k, v, lp)


def _mcat(h, k=K, d=D, v=VS, logp=None, null=()):
    V = None if "V" in null else ip(v)
    lp = None if "logp" in null else dp(np.zeros((max(k, 1), max(int(np.sum(np.maximum(v, 0))), 1))) if logp is None else logp)
    return lambda lib: lib.svihmm_set_emission_mcat(h, k, d, V, lp)


def _pois(h, k=K, d=D, c=C, elog=None, erate=None, lf=None, null=()):
    shape = (max(k, 1), max(d, 1))
    el = None if "elog" in null else dp(np.zeros(shape) if elog is None else elog)
    er = None if "erate" in null else dp(np.ones(shape) if erate is None else erate)
    tab = None if "logfact" in null else dp(np.zeros(max(C, 0) + 1) if lf is None else lf)
    return lambda lib: lib.svihmm_set_emission_poisson(h, k, d, el, er, tab, c)


def _pg(h, k=K, d=D, mu=None, hprec=None, cst=None, origin=None, null=()):
    shape = (max(k, 1), max(d, 1))
    arrs = {"mu": np.zeros(shape) if mu is None else mu, "hprec": -np.ones(shape) if hprec is None else hprec,
            "cst": np.zeros(shape) if cst is None else cst, "origin": np.zeros(shape[1]) if origin is None else origin}
    ptr = {n: None if n in null else dp(a) for n, a in arrs.items()}
    return lambda lib: lib.svihmm_set_emission_pgauss(h, k, d, ptr["mu"], ptr["hprec"], ptr["cst"], ptr["origin"])


def _b_niw(h, k=K, d=D, pt=PT, vt=VT, maxit=MAXIT, null=None):
    n = max(k, 1)
    arrs = [pt, vt, np.ones((n, d)), np.tile(np.eye(d), (n, 1, 1)), np.ones(n), np.full(n, d + 2.0), np.zeros(n),
            np.ones((n, d)), np.tile(np.eye(d), (n, 1, 1)), np.ones(n), np.full(n, d + 2.0)]
    ptrs = [None if null == i else dp(a) for i, a in enumerate(arrs)]
    return lambda lib: lib.svihmm_svi_begin(h, k, d, *(ptrs + [maxit, 1.0]))


def _b_diag(h, k=K, d=D, pt=PT, vt=VT, prior=None, fac=None, maxit=MAXIT, null=()):
    n = max(k, 1)
    pb = None if "prior" in null else dp(np.ones((4, n, max(d, 1))) if prior is None else prior)
    fb = dp(np.ones((4, n, max(d, 1))) if fac is None else fac)
    return lambda lib: lib.svihmm_svi_begin_diag(h, k, d, dp(pt), dp(vt), pb, fb, maxit)


def _b_cat(h, k=K, v=VS[0], pt=PT, vt=VT, a0=None, a=None, maxit=MAXIT, null=()):
    shape = (max(k, 1), max(v, 1))
    p0 = None if "alpha0" in null else dp(np.ones(shape) if a0 is None else a0)
    p1 = dp(np.ones(shape) if a is None else a)
    return lambda lib: lib.svihmm_svi_begin_cat(h, k, v, dp(pt), dp(vt), p0, p1, maxit)


def _b_mcat(h, k=K, d=D, v=VS, pt=PT, vt=VT, a0=None, a=None, maxit=MAXIT, null=()):
    shape = (max(k, 1), max(int(np.sum(np.maximum(v, 0))), 1))
    V = None if "V" in null else ip(v)
    p0, p1 = dp(np.ones(shape) if a0 is None else a0), dp(np.ones(shape) if a is None else a)
    return lambda lib: lib.svihmm_svi_begin_mcat(h, k, d, V, dp(pt), dp(vt), p0, p1, maxit)


def _b_pois(h, k=K, d=D, c=C, pt=PT, vt=VT, prior=None, fac=None, lf=None, maxit=MAXIT, null=()):
    shape = (2, max(k, 1), max(d, 1))
    pb, fb = dp(np.ones(shape) if prior is None else prior), dp(np.ones(shape) if fac is None else fac)
    tab = None if "logfact" in null else dp(np.zeros(max(C, 0) + 1) if lf is None else lf)
    return lambda lib: lib.svihmm_svi_begin_poisson(h, k, d, dp(pt), dp(vt), pb, fb, tab, c, maxit)


def refusal_cases():
    """(id, family in force on the handle, handle -> call, full text); a case builds its arrays when it is made for a handle."""
    N, I = np.nan, np.inf
    big = np.ones((1025, 1025))
    sn, sd, sc = "svihmm_set_emission_niw: ", "svihmm_set_emission_diag: ", "svihmm_set_emission_cat: "
    sm, sp, sg = "svihmm_set_emission_mcat: ", "svihmm_set_emission_poisson: ", "svihmm_set_emission_pgauss: "
    bn, bd, bc = "svihmm_svi_begin: ", "svihmm_svi_begin_diag: ", "svihmm_svi_begin_cat: "
    bm, bp = "svihmm_svi_begin_mcat: ", "svihmm_svi_begin_poisson: "
    none4 = [None] * 4
    cases = [
        # ---- svihmm_set_emission_niw
        ("set_niw-K0", "niw", lambda h: _niw(h, k=0), sn + "bad arguments"),
        ("set_niw-D0", "niw", lambda h: _niw(h, d=0), sn + "bad arguments"),
        ("set_niw-null", "niw", lambda h: _niw(h, a=none4), sn + "bad arguments"),
        ("set_niw-D97", "niw", lambda h: _niw(h, d=97), sn + "D > SVIHMM_NIW_MAX_D: " + HOST),
        # ---- svihmm_set_emission_diag
        ("set_diag-K0", "diag", lambda h: _diag(h, k=0), sd + "bad arguments"),
        ("set_diag-D0", "diag", lambda h: _diag(h, d=-1), sd + "bad arguments"),
        ("set_diag-null", "diag", lambda h: _diag(h, a=none4), sd + "bad arguments"),
        ("set_diag-D129", "diag", lambda h: _diag(h, d=129), sd + "D > SVIHMM_DIAG_MAX_D: " + HOST),
        # ---- svihmm_set_emission_cat
        ("set_cat-K0", "cat", lambda h: _cat(h, k=0), sc + "bad arguments"),
        ("set_cat-V0", "cat", lambda h: _cat(h, v=0), sc + "bad arguments"),
        ("set_cat-null", "cat", lambda h: _cat(h, null=True), sc + "bad arguments"),
        # ---- svihmm_set_emission_mcat (K, D, V[d], F, logp)
        ("set_mcat-nullV", "mcat", lambda h: _mcat(h, null=("V",)), sm + "V and logp must not be NULL"),
        ("set_mcat-nulllogp", "mcat", lambda h: _mcat(h, k=0, null=("logp",)), sm + "V and logp must not be NULL"),
        ("set_mcat-K0", "mcat", lambda h: _mcat(h, k=0, d=0), sm + "K = 0 outside [1, 256]"),
        ("set_mcat-K257", "mcat", lambda h: _mcat(h, k=257), sm + "K = 257 outside [1, 256]"),
        ("set_mcat-D0", "mcat", lambda h: _mcat(h, d=0, v=(0,)), sm + "D = 0 outside [1, SVIHMM_MCAT_MAX_D = 128]"),
        ("set_mcat-D129", "mcat", lambda h: _mcat(h, d=129, v=(1,) * 129), sm + "D = 129 outside [1, SVIHMM_MCAT_MAX_D = 128]"),
        ("set_mcat-V1", "mcat", lambda h: _mcat(h, v=(2000, 0)), sm + "V[1] = 0 (every column needs at least one symbol)"),
        ("set_mcat-Vneg", "mcat", lambda h: _mcat(h, v=(-3, 5)), sm + "V[0] = -3 (every column needs at least one symbol)"),
        ("set_mcat-F", "mcat", lambda h: _mcat(h, v=(1000, 25), logp=np.full((K, 1025), N)),
         sm + "F = sum of V = 1025 exceeds SVIHMM_MCAT_MAX_F = 1024"),
        ("set_mcat-nan", "mcat", lambda h: _mcat(h, logp=_with(np.zeros((K, F)), (2, 3), N)), sm + "logp[2][3] is not finite"),
        ("set_mcat-inf", "mcat", lambda h: _mcat(h, logp=_with(_with(np.zeros((K, F)), (1, 6), -I), (2, 0), N)), sm + "logp[1][6] is not finite"),
        # ---- svihmm_set_emission_poisson (K, D, C, elog / erate entry by entry, logfact)
        ("set_pois-null", "poisson", lambda h: _pois(h, k=0, null=("erate",)), sp + "elog, erate and logfact must not be NULL"),
        ("set_pois-nulllf", "poisson", lambda h: _pois(h, null=("logfact",)), sp + "elog, erate and logfact must not be NULL"),
        ("set_pois-K0", "poisson", lambda h: _pois(h, k=0, d=0), sp + "K = 0 outside [1, 256]"),
        ("set_pois-K257", "poisson", lambda h: _pois(h, k=257), sp + "K = 257 outside [1, 256]"),
        ("set_pois-D0", "poisson", lambda h: _pois(h, d=0, c=-1), sp + "D = 0 outside [1, SVIHMM_POISSON_MAX_D = 128]"),
        ("set_pois-D129", "poisson", lambda h: _pois(h, d=129), sp + "D = 129 outside [1, SVIHMM_POISSON_MAX_D = 128]"),
        ("set_pois-Cneg", "poisson", lambda h: _pois(h, c=-1, elog=np.full((K, D), N)), sp + "C = -1 outside [0, SVIHMM_POISSON_MAX_COUNT = 1048575]"),
        ("set_pois-Cbig", "poisson", lambda h: _pois(h, c=1048576), sp + "C = 1048576 outside [0, SVIHMM_POISSON_MAX_COUNT = 1048575]"),
        ("set_pois-elog", "poisson", lambda h: _pois(h, elog=_with(np.zeros((K, D)), (1, 1), I), lf=_with(np.zeros(C + 1), 0, N)),
         sp + "elog[1][1] is not finite"),
        ("set_pois-erate", "poisson", lambda h: _pois(h, elog=_with(np.zeros((K, D)), (2, 0), N), erate=_with(np.ones((K, D)), (1, 1), N)),
         sp + "erate[1][1] is not finite"),
        ("set_pois-elog-first", "poisson", lambda h: _pois(h, elog=_with(np.zeros((K, D)), (1, 0), N), erate=_with(np.ones((K, D)), (1, 0), N)),
         sp + "elog[1][0] is not finite"),
        ("set_pois-logfact", "poisson", lambda h: _pois(h, lf=_with(np.zeros(C + 1), 7, I)), sp + "logfact[7] is not finite"),
        # ---- svihmm_set_emission_pgauss (K, D, then entry by entry: mu, hprec, cst finite, hprec <= 0, |mu|; origin)
        ("set_pg-null", "pgauss", lambda h: _pg(h, k=0, null=("cst",)), sg + "mu, hprec, cst and origin must not be NULL"),
        ("set_pg-nullorigin", "pgauss", lambda h: _pg(h, null=("origin",)), sg + "mu, hprec, cst and origin must not be NULL"),
        ("set_pg-K0", "pgauss", lambda h: _pg(h, k=0, d=0), sg + "K = 0 outside [1, 256]"),
        ("set_pg-K257", "pgauss", lambda h: _pg(h, k=257), sg + "K = 257 outside [1, 256]"),
        ("set_pg-D0", "pgauss", lambda h: _pg(h, d=0), sg + "D = 0 outside [1, SVIHMM_PGAUSS_MAX_D = 128]"),
        ("set_pg-D129", "pgauss", lambda h: _pg(h, d=129), sg + "D = 129 outside [1, SVIHMM_PGAUSS_MAX_D = 128]"),
        ("set_pg-mu", "pgauss", lambda h: _pg(h, mu=_with(np.zeros((K, D)), (2, 1), N), origin=[N, 0.0]), sg + "mu[2][1] is not finite"),
        ("set_pg-hprec", "pgauss", lambda h: _pg(h, hprec=_with(-np.ones((K, D)), (0, 1), -I), cst=_with(np.zeros((K, D)), (0, 1), N)),
         sg + "hprec[0][1] is not finite"),
        ("set_pg-cst", "pgauss", lambda h: _pg(h, cst=_with(np.zeros((K, D)), (1, 0), I), hprec=_with(-np.ones((K, D)), (1, 0), 2.0)),
         sg + "cst[1][0] is not finite"),
        ("set_pg-hpos", "pgauss", lambda h: _pg(h, hprec=_with(-np.ones((K, D)), (1, 1), 0.25), mu=_with(np.zeros((K, D)), (1, 1), 1e150)),
         sg + "hprec[1][1] is positive (hprec = -0.5 alphas / betas)"),
        ("set_pg-muabs", "pgauss", lambda h: _pg(h, mu=_with(np.zeros((K, D)), (0, 0), -1e150)), sg + "|mu[0][0]| is at or above SVIHMM_PGAUSS_ABSENT"),
        ("set_pg-origin", "pgauss", lambda h: _pg(h, origin=[0.0, I]), sg + "origin[1] is not finite"),
        ("set_pg-originabs", "pgauss", lambda h: _pg(h, origin=[2e150, N]), sg + "|origin[0]| is at or above SVIHMM_PGAUSS_ABSENT"),
        # ---- svihmm_svi_begin
        ("begin_niw-K0", "niw", lambda h: _b_niw(h, k=0), bn + "bad arguments"),
        ("begin_niw-maxit0", "niw", lambda h: _b_niw(h, maxit=0), bn + "bad arguments"),
        ("begin_niw-nullpt", "niw", lambda h: _b_niw(h, null=0), bn + "bad arguments"),
        ("begin_niw-nullnu", "niw", lambda h: _b_niw(h, null=10), bn + "bad arguments"),
        ("begin_niw-K1025", "niw", lambda h: _b_niw(h, k=1025, pt=big, vt=big), bn + "K > 1024 unsupported"),
        ("begin_niw-D3", "niw", lambda h: _b_niw(h, d=3), bn + "D does not match the resident observations"),
        ("begin_niw-vt", "niw", lambda h: _b_niw(h, vt=LOW_VT), PSEUDO),
        ("begin_niw-pt", "niw", lambda h: _b_niw(h, pt=LOW_PT), PSEUDO),
        # ---- svihmm_svi_begin_diag
        ("begin_diag-D0", "diag", lambda h: _b_diag(h, d=0), bd + "bad arguments"),
        ("begin_diag-null", "diag", lambda h: _b_diag(h, null=("prior",)), bd + "bad arguments"),
        ("begin_diag-D129", "diag", lambda h: _b_diag(h, d=129), bd + "D > SVIHMM_DIAG_MAX_D"),
        ("begin_diag-nus", "diag", lambda h: _b_diag(h, fac=_with(np.ones((4, K, D)), (1, 2, 0), 0.0), vt=LOW_VT),
         bd + "nus, alphas, betas must be positive"),
        ("begin_diag-betas0", "diag", lambda h: _b_diag(h, prior=_with(np.ones((4, K, D)), (3, 0, 1), N)), bd + "nus, alphas, betas must be positive"),
        ("begin_diag-K1025", "diag", lambda h: _b_diag(h, k=1025, pt=big, vt=big), bn + "K > 1024 unsupported"),
        ("begin_diag-D3", "diag", lambda h: _b_diag(h, d=3), bn + "D does not match the resident observations"),
        ("begin_diag-vt", "diag", lambda h: _b_diag(h, vt=LOW_VT), PSEUDO),
        # ---- svihmm_svi_begin_cat
        ("begin_cat-V0", "cat", lambda h: _b_cat(h, v=0), bc + "bad arguments"),
        ("begin_cat-null", "cat", lambda h: _b_cat(h, null=("alpha0",)), bc + "bad arguments"),
        ("begin_cat-D2", "mcat", lambda h: _b_cat(h, a=np.zeros((K, VS[0]))), bc + "the resident observations must be one symbol column (D = 1)"),
        ("begin_cat-alpha", "cat", lambda h: _b_cat(h, a=_with(np.ones((K, VS[0])), (2, 1), 0.0), pt=LOW_PT), bc + "Dirichlet parameters must be positive"),
        ("begin_cat-alpha0", "cat", lambda h: _b_cat(h, a0=_with(np.ones((K, VS[0])), (0, 0), -1.0)), bc + "Dirichlet parameters must be positive"),
        ("begin_cat-K1025", "cat", lambda h: _b_cat(h, k=1025, pt=big, vt=big), bn + "K > 1024 unsupported"),
        ("begin_cat-pt", "cat", lambda h: _b_cat(h, pt=LOW_PT), PSEUDO),
        # ---- svihmm_svi_begin_mcat (K, D, V[d], F, the resident D, alpha)
        ("begin_mcat-null", "mcat", lambda h: _b_mcat(h, k=0, null=("V",)), bm + "bad arguments"),
        ("begin_mcat-maxit", "mcat", lambda h: _b_mcat(h, k=0, maxit=-1), bm + "bad arguments"),
        ("begin_mcat-K0", "mcat", lambda h: _b_mcat(h, k=0, d=0), bm + "K = 0 outside [1, 256]"),
        ("begin_mcat-K257", "mcat", lambda h: _b_mcat(h, k=257, pt=np.ones((257, 257)), vt=np.ones((257, 257))), bm + "K = 257 outside [1, 256]"),
        ("begin_mcat-D0", "mcat", lambda h: _b_mcat(h, d=0, v=(0,)), bm + "D = 0 outside [1, SVIHMM_MCAT_MAX_D = 128]"),
        ("begin_mcat-D129", "mcat", lambda h: _b_mcat(h, d=129, v=(1,) * 129), bm + "D = 129 outside [1, SVIHMM_MCAT_MAX_D = 128]"),
        ("begin_mcat-V0", "mcat", lambda h: _b_mcat(h, d=3, v=(2, 5, 0)), bm + "V[2] = 0 (every column needs at least one symbol)"),
        ("begin_mcat-F", "mcat", lambda h: _b_mcat(h, d=3, v=(1000, 20, 5)), bm + "F = sum of V = 1025 exceeds SVIHMM_MCAT_MAX_F = 1024"),
        ("begin_mcat-D3", "mcat", lambda h: _b_mcat(h, d=3, v=(2, 5, 2), a=np.zeros((K, 9))),
         bm + "the family has D = 3 symbol columns, the resident observations have 2"),
        ("begin_mcat-alpha", "mcat", lambda h: _b_mcat(h, a=_with(np.ones((K, F)), (1, 4), 0.0), vt=LOW_VT), bm + "Dirichlet parameters must be positive"),
        ("begin_mcat-alpha0", "mcat", lambda h: _b_mcat(h, a0=_with(np.ones((K, F)), (2, 6), N)), bm + "Dirichlet parameters must be positive"),
        ("begin_mcat-vt", "mcat", lambda h: _b_mcat(h, vt=LOW_VT), PSEUDO),
        # ---- svihmm_svi_begin_poisson (K, D, C, logfact, the resident D, a / b)
        ("begin_pois-null", "poisson", lambda h: _b_pois(h, k=0, null=("logfact",)), bp + "bad arguments"),
        ("begin_pois-maxit", "poisson", lambda h: _b_pois(h, k=0, maxit=0), bp + "bad arguments"),
        ("begin_pois-K0", "poisson", lambda h: _b_pois(h, k=0, d=0), bp + "K = 0 outside [1, 256]"),
        ("begin_pois-K257", "poisson", lambda h: _b_pois(h, k=257, pt=np.ones((257, 257)), vt=np.ones((257, 257))), bp + "K = 257 outside [1, 256]"),
        ("begin_pois-D0", "poisson", lambda h: _b_pois(h, d=0, c=-1), bp + "D = 0 outside [1, SVIHMM_POISSON_MAX_D = 128]"),
        ("begin_pois-D129", "poisson", lambda h: _b_pois(h, d=129), bp + "D = 129 outside [1, SVIHMM_POISSON_MAX_D = 128]"),
        ("begin_pois-Cneg", "poisson", lambda h: _b_pois(h, c=-1, d=3), bp + "C = -1 outside [0, SVIHMM_POISSON_MAX_COUNT = 1048575]"),
        ("begin_pois-Cbig", "poisson", lambda h: _b_pois(h, c=1048576), bp + "C = 1048576 outside [0, SVIHMM_POISSON_MAX_COUNT = 1048575]"),
        ("begin_pois-logfact", "poisson", lambda h: _b_pois(h, d=3, lf=_with(np.zeros(C + 1), 2, I)), bp + "logfact[2] is not finite"),
        ("begin_pois-D3", "poisson", lambda h: _b_pois(h, d=3, fac=np.zeros((2, K, 3))),
         bp + "the family has D = 3 count columns, the resident observations have 2"),
        ("begin_pois-b", "poisson", lambda h: _b_pois(h, fac=_with(np.ones((2, K, D)), (1, 2, 1), 0.0), pt=LOW_PT), bp + "Gamma parameters must be positive"),
        ("begin_pois-a0", "poisson", lambda h: _b_pois(h, prior=_with(np.ones((2, K, D)), (0, 0, 0), -2.0)), bp + "Gamma parameters must be positive"),
        ("begin_pois-pt", "poisson", lambda h: _b_pois(h, pt=LOW_PT), PSEUDO),
    ]
    return cases


CASES = refusal_cases()


NULL_HANDLE = [
    (_niw, "svihmm_set_emission_niw: bad arguments"), (_diag, "svihmm_set_emission_diag: bad arguments"),
    (_cat, "svihmm_set_emission_cat: bad arguments"),
    (_mcat, "svihmm_set_emission_mcat: handle is NULL"), (_pois, "svihmm_set_emission_poisson: handle is NULL"),
    (_pg, "svihmm_set_emission_pgauss: handle is NULL"), (_b_niw, "svihmm_svi_begin: bad arguments"),
    (_b_diag, "svihmm_svi_begin_diag: bad arguments"), (_b_cat, "svihmm_svi_begin_cat: bad arguments"),
    (_b_mcat, "svihmm_svi_begin_mcat: bad arguments"), (_b_pois, "svihmm_svi_begin_poisson: bad arguments"),
]


@pytest.fixture(scope="module")
def handles():
    """One handle per family in force, each with the loglik of the tiny batch taken before any refusal."""
    made = {}

    def get(name):
        if name not in made:
            e = _engine()
            e.set_obs(_obs(name), None)
            e.set_globals(P["mod_init"], P["ltran"])
            _set(e, name)
            made[name] = (e, e.loglik(STARTS, LM))
        return made[name]
    yield get
    for e, _ in made.values():
        e.close()


def test_null_handle_refusals():
    lib = L.load()
    for make, text in NULL_HANDLE:
        assert make(None)(lib) != 0
        assert L.last_error() == text
    del _keep[:]


@pytest.mark.parametrize("fam,make,text", [pytest.param(*c[1:], id=c[0]) for c in CASES])
def test_refusal_text_and_untouched_handle(handles, fam, make, text):
    e, ll0 = handles(fam)
    assert np.all(np.isfinite(ll0)) and np.any(ll0 != 0.0)
    rc = make(e._h)(e._lib)
    del _keep[:]
    assert rc != 0
    assert L.last_error() == text
    np.testing.assert_array_equal(e.loglik(STARTS, LM), ll0)


# ---------------------------------------------------------------------------------------------------
#  2. the loop-ending matrix
# ---------------------------------------------------------------------------------------------------
_fresh = {}


def fresh_loglik(name):
    """loglik under the setter ``name`` on a handle that only did set_obs (+ the globals loglik asks for) + the setter;
    computed once per setter and left unchanged."""
    if name not in _fresh:
        e = _engine()
        try:
            e.set_obs(_obs(name), None)
            e.set_globals(P["mod_init"], P["ltran"])
            _set(e, name)
            _fresh[name] = e.loglik(STARTS, LM)
        finally:
            e.close()
    return _fresh[name]


def _iterate(e, it):
    e.svi_iteration(it, STARTS, B, LM, L.TRANS_WRAP, 0.5, 3.0, 3.0)


# what svihmm_svi_iteration says once the setter has ended the loop, by the family the setter left in force
_TAKE = "svihmm_svi_iteration: the resident SVI loop does not take "
DEAD_LOOP = {
    "niw": "svihmm_svi_iteration: call svihmm_svi_begin first",
    "diag": "svihmm_svi_iteration: call svihmm_svi_begin first",
    "cat": "svihmm_svi_iteration: call svihmm_svi_begin first",
    "mcat": _TAKE + "the multi-column Categorical family from svihmm_set_emission_mcat alone: the family enters the loop "
                    "through svihmm_svi_begin_mcat",
    "poisson": _TAKE + "the Poisson family from svihmm_set_emission_poisson alone: the family enters the loop through "
                    "svihmm_svi_begin_poisson",
    "pgauss": _TAKE + "the family of svihmm_set_emission_pgauss; step the globals on the host from svihmm_estep_minibatch's "
                    "statistics",
}
MATRIX = [(l, s) for l in LOOPS for s in FAMILIES] + [("cat", "cat3"), ("mcat", "mcat35")]


@pytest.mark.parametrize("loop,setter", MATRIX, ids=lambda n: n)
def test_setter_after_two_iterations_of_a_loop(loop, setter):
    e = _engine()
    try:
        e.set_obs(_obs(loop), None)
        _begin(e, loop)
        _iterate(e, 0)
        _iterate(e, 1)
        _set(e, setter)
        if setter == loop:
            _iterate(e, 2)
            elbo = e.svi_read_elbo(3)[0]
            assert elbo.shape == (3,) and np.all(np.isfinite(elbo))
            assert e.svi_recoveries() == 0
            return
        with pytest.raises(RuntimeError, match=re.escape("svihmm_svi_iteration failed: " + DEAD_LOOP[setter.rstrip("35")]) + "$"):
            _iterate(e, 2)
        e.sync()
        if _obs(setter).shape[1] != _obs(loop).shape[1]:      # (the rows the family reads: uploaded under it)
            e.set_obs(_obs(setter), None)
        got = e.loglik(STARTS, LM)
    finally:
        e.close()
    want = fresh_loglik(setter)
    assert np.all(np.isfinite(want)) and np.any(want != 0.0)
    np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-8)
