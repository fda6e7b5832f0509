"""Referees, cases and drivers for the table-driven families of the resident SVI loop: multi-column Categorical
(``svihmm_svi_begin_mcat``, family 3) and Poisson (``svihmm_svi_begin_poisson``, family 4).  Shared by
tests/test_svi_families_ref.py (CPU) and tests/test_gpu_svi_families.py; built on tests/svi_referee.py and the
bounds of tests/svi_cases.py.  Only tests import this module.

Rules (pysvihmm_amd/csrc/kernels_svi.h, hmmsgd_metaobs.VBHMM.global_update):
  mcat     alpha' = ((1 - rho)(alpha - 1) + (rho bE)(nwin (alpha0 - 1) + counts)) + 1     per element of [K][F]
  Poisson  a' = (1 - rho) a + rho (a0 + bE sx),   b' = (1 - rho) b + rho (b0 + bE n)      per (k, d)
"""
import mpmath as mp
import numpy as np

from tests import svi_referee as R
from tests.svi_cases import T_OBS, B_WIN, L_WIN, ELBO_MULT, prior_tran_for
from tests.svi_referee import LD, ld, tran_step, tran_step_f64, cat_vlb, dirichlet_rows, digamma_f64, _Acc

POIS_C = 300          # largest count of the Poisson cases


# ---------------------------------------------------------------------------------------------------
#  global step: longdouble referees ({name: (value, scale)}) and float64 restatements of the device formulas
# ---------------------------------------------------------------------------------------------------
def global_step_mcat(state, prior, packed, rho, bA, bE, nwin, ada_G=None):
    """``state`` = (var_tran, alpha_0 [K,V_0], .., alpha_{D-1}), ``prior`` = (prior_tran, alpha0_0, ..), ``packed`` a
    PackedMCatStats view: the Categorical rule per column (hmmsgd_metaobs.py:907-926, 1071-1084, every window
    contributes alpha0 + counts - 1).  The output "alpha" is the [K, F] block, columns side by side."""
    out = tran_step(state[0], prior[0], packed.A_raw, nwin, rho, bA, ada_G)
    al, al0, c = (ld(np.concatenate(list(x), axis=1)) for x in (state[1:], prior[1:], packed.col_counts))
    rho, bE, nwin = LD(rho), LD(bE), LD(nwin)
    inter = nwin * (al0 - 1) + c
    inter_abs = nwin * np.abs(al0 - 1) + np.abs(c)
    new = ((1 - rho) * (al - 1) + (rho * bE) * inter) + 1
    out["alpha"] = (new, np.abs(1 - rho) * np.abs(al - 1) + np.abs(rho * bE) * inter_abs + 1)
    return out


def global_step_poisson(state, prior, packed, rho, bA, bE, nwin, ada_G=None):
    """``state`` = (var_tran, a [K,D], b [K,D]), ``prior`` = (prior_tran, a0, b0), ``packed`` a PackedPoissonStats
    view.  Scales |1 - rho||a| + |rho|(|a0| + |bE sx|), likewise for b."""
    out = tran_step(state[0], prior[0], packed.A_raw, nwin, rho, bA, ada_G)
    a, b, a0, b0, sx, n = (ld(x) for x in (state[1], state[2], prior[1], prior[2], packed.sx, packed.n))
    rho, bE = LD(rho), LD(bE)
    w, aw, ar = 1 - rho, np.abs(1 - rho), np.abs(rho)
    out["a"] = (w * a + rho * (a0 + bE * sx), aw * np.abs(a) + ar * (np.abs(a0) + np.abs(bE * sx)))
    out["b"] = (w * b + rho * (b0 + bE * n), aw * np.abs(b) + ar * (np.abs(b0) + np.abs(bE * n)))
    return out


def _tran_f64(state, prior, packed, nwin, rho, bA, ada_G):
    out = {}
    out["var_tran"], g = tran_step_f64(np.asarray(state[0], dtype=np.float64), np.asarray(prior[0], dtype=np.float64),
                                       packed.A_raw, nwin, rho, bA, ada_G)
    if g is not None:
        out["ada_G"] = g
    return out


def global_step_mcat_f64(state, prior, packed, rho, bA, bE, nwin, ada_G=None):
    """k_svi_global_step_simple_body, fam 3 (fam 2's expression on the [K][F] block)."""
    out = _tran_f64(state, prior, packed, nwin, rho, bA, ada_G)
    al, al0 = (np.concatenate([np.asarray(x, dtype=np.float64) for x in s], axis=1) for s in (state[1:], prior[1:]))
    inter = float(nwin) * (al0 - 1.0) + packed.flat
    out["alpha"] = ((1.0 - rho) * (al - 1.0) + (rho * bE) * inter) + 1.0
    return out


def global_step_poisson_f64(state, prior, packed, rho, bA, bE, nwin, ada_G=None):
    """svi_pois_step: every product and sum rounded on its own."""
    out = _tran_f64(state, prior, packed, nwin, rho, bA, ada_G)
    a, b, a0, b0 = (np.asarray(x, dtype=np.float64) for x in (state[1], state[2], prior[1], prior[2]))
    out["a"] = (1.0 - rho) * a + rho * (a0 + bE * packed.sx)
    out["b"] = (1.0 - rho) * b + rho * (b0 + bE * packed.n)
    return out


# ---------------------------------------------------------------------------------------------------
#  the factors' ELBO terms: mpmath referees ((value, sum|terms|)) and float64 restatements (vlb[K])
# ---------------------------------------------------------------------------------------------------
def mcat_vlb(alpha_cols, alpha0_cols, dps=30):
    """``ProductCategorical.get_vlb`` of ONE state: the sum over the columns of the Dirichlet term."""
    with mp.workdps(dps):
        v, a = mp.mpf(0), mp.mpf(0)
        for al, al0 in zip(alpha_cols, alpha0_cols):
            tv, ta = cat_vlb(al, al0, dps)
            v, a = v + tv, a + ta
        return v, a


def poisson_vlb(a, b, a0, b0, dps=30):
    """``ProductPoisson.get_vlb`` of ONE state: - sum_d KL(Gamma(a, b) || Gamma(a0, b0)) with its terms
    (a - a0) psi(a) - lgamma(a) + lgamma(a0) + a0 (log b - log b0) + a (b0 - b) / b.  a - a0 and b0 - b are single
    rounded operations on given numbers: the differences are the terms."""
    with mp.workdps(dps):
        c = lambda x: [mp.mpf(float(v)) for v in np.asarray(x, dtype=np.float64).ravel()]
        acc = _Acc()
        for x, y, x0, y0 in zip(c(a), c(b), c(a0), c(b0)):
            acc.add(-(x - x0) * mp.digamma(x))
            acc.add(mp.loggamma(x)); acc.add(-mp.loggamma(x0))
            acc.add(-x0 * mp.log(y)); acc.add(x0 * mp.log(y0))
            acc.add(-x * (y0 - y) / y)
        return acc.v, acc.a


def global_lower_bound_mcat(state, prior, dps=30):
    K = np.asarray(state[1]).shape[0]
    return R._glb(dirichlet_rows(prior[0], state[0], dps),
                  [mcat_vlb([np.asarray(c)[k] for c in state[1:]], [np.asarray(c)[k] for c in prior[1:]], dps)
                   for k in range(K)])


def global_lower_bound_poisson(state, prior, dps=30):
    K = np.asarray(state[1]).shape[0]
    return R._glb(dirichlet_rows(prior[0], state[0], dps),
                  [poisson_vlb(state[1][k], state[2][k], prior[1][k], prior[2][k], dps) for k in range(K)])


def mcat_vlb_f64(alpha_cols, alpha0_cols):
    """k_svi_vlb_simple_body, fam 3 (svi_mcat_vlb): per state the sum over the columns of the Dirichlet term (the
    device adds the columns' and the features' terms lane-strided and reduces once; NumPy's order here)."""
    tot = np.zeros(np.asarray(alpha_cols[0]).shape[0])
    for al, al0 in zip(alpha_cols, alpha0_cols):
        tot = tot + R.cat_vlb_f64(al, al0)
    return tot


def poisson_vlb_f64(a, b, a0, b0):
    """k_svi_vlb_simple_body, fam 4."""
    from scipy.special import gammaln
    a, b, a0, b0 = (np.asarray(x, dtype=np.float64) for x in (a, b, a0, b0))
    dg = digamma_f64(a.ravel()).reshape(a.shape)
    kl = (a - a0) * dg - gammaln(a) + gammaln(a0) + a0 * (np.log(b) - np.log(b0)) + a * (b0 - b) / b
    return -kl.sum(axis=1)


# ---------------------------------------------------------------------------------------------------
#  cases of test 5 (on the resident rows / windows of tests/svi_cases.step_case)
# ---------------------------------------------------------------------------------------------------
# (family, K, shape, rho, var_tran family, options)   shape = V (mcat, a tuple) or D (poisson)
FAMILY_CASES = [
    ("mcat", 3, (2,), 1.0, "counts", ""),
    ("mcat", 3, (2, 3, 1, 70), 0.3, "counts", ""),          # a one-symbol column and one wider than a wave
    ("mcat", 65, (2,) * 128, 0.3, "blocks", ""),
    ("mcat", 3, (256,) * 4, 1e-8, "counts", ""),            # F = 1024
    ("mcat", 130, (3, 4), 0.3, "sink", "empty"),
    ("mcat", 3, (2, 5), 0.3, "counts", "adagrad"),
    ("poisson", 3, 1, 1.0, "counts", ""),
    ("poisson", 64, 65, 0.3, "counts", ""),
    ("poisson", 65, 128, 1e-8, "blocks", ""),
    ("poisson", 130, 2, 0.3, "sink", "empty"),
    ("poisson", 3, 5, 0.3, "counts", "adagrad"),
]


def family_case_id(c):
    shp = c[2]
    s = "D%d" % shp if isinstance(shp, int) else ("%dx%d" % (len(shp), shp[0]) if len(set(shp)) == 1 and len(shp) > 1
                                                  else "V" + "_".join(str(v) for v in shp))
    return "%s-K%d-%s-rho%g-%s%s" % (c[0], c[1], s, c[3], c[4], ("-" + c[5]) if c[5] else "")


def family_case(fam, K, shape, rho, tran, opts=""):
    """A benign problem on T_OBS resident rows, B_WIN windows of L_WIN rows.  mcat: Dirichlet factors
    0.05 + Gamma(0.5, 20), priors 1 + U(0, 1) (>= 1, as the Categorical cases: every window contributes alpha0 - 1).
    Poisson: a over 1e-2 .. 1e6 and b over 1e-2 .. 1e4 across the states (rates 1 .. 100), counts up to POIS_C."""
    D = shape if fam == "poisson" else len(shape)
    rng = np.random.default_rng(1000 * K + 31 * D + (3 if fam == "poisson" else 11))
    c = dict(fam=fam, K=K, shape=shape, D=D, rho=float(rho), opts=opts, tran=tran, mask=None,
             var_tran=R.tran_family(tran, K), prior_tran=prior_tran_for(K), nit=2 if "adagrad" in opts else 1,
             B=B_WIN, Lm=L_WIN, bA=(4000 - 17.0) / (16.0 * B_WIN), bE=(4000 - 17.0) / (17.0 * B_WIN))
    r2 = np.random.default_rng(5 + K)
    c["starts"] = [r2.integers(0, T_OBS - L_WIN, size=B_WIN) for _ in range(c["nit"])]
    if "empty" in opts:
        c["starts"] = [s[:0] for s in c["starts"]]
    if fam == "mcat":
        c["obs"] = np.stack([rng.integers(0, v, size=T_OBS) for v in shape], axis=1).astype(np.float64)
        c["factors"] = [0.05 + rng.gamma(0.5, 20.0, size=(K, v)) for v in shape]
        c["prior"] = [1.0 + rng.random((K, v)) for v in shape]
    else:
        obs = rng.poisson(5.0, size=(T_OBS, D))
        wild = rng.random((T_OBS, D)) < 0.1
        obs[wild] = rng.integers(0, POIS_C + 1, size=int(wild.sum()))
        c["obs"] = obs.astype(np.float64)
        ak = 10.0 ** (rng.permutation(np.linspace(-2.0, 6.0, K)) if K > 1 else np.array([2.0]))
        a = ak[:, None] * rng.uniform(0.5, 2.0, size=(K, D))
        b = np.clip(a / rng.uniform(1.0, 20.0, size=(K, D)), 1e-2, 1e4)
        c["factors"] = (a, b)
        c["prior"] = (0.5 + rng.random((K, D)), 0.5 + rng.random((K, D)))
    return c


def case_begin(eng, c):
    eng.set_obs(c["obs"], c["mask"])
    if c["fam"] == "mcat":
        eng.svi_begin_mcat(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], 2)
    else:
        eng.svi_begin_poisson(c["prior_tran"], c["var_tran"], c["prior"], c["factors"], POIS_C, 2)
    if "adagrad" in c["opts"]:
        eng.svi_set_adagrad(np.ones((c["K"], c["K"])))


def case_run(eng, c, flags):
    """tests/svi_cases.case_run for these families: per iteration the state before, the packed statistics the step
    consumed, the state after, the AdaGrad accumulator before / after and the ELBO entry."""
    case_begin(eng, c)
    pre = (c["var_tran"],) + tuple(c["factors"])
    ada = np.ones((c["K"], c["K"])) if "adagrad" in c["opts"] else None
    recs = []
    for it in range(c["nit"]):
        eng.svi_iteration(it, c["starts"][it], c["B"], c["Lm"], flags, c["rho"], c["bA"], c["bE"])
        packed = eng.read_packed()
        vt, vi, fac = eng.svi_read_factors()
        post = (vt,) + tuple(fac)
        ada_post = eng.svi_read_adagrad() if ada is not None else None
        elbo = eng.svi_read_elbo(it + 1)[0][it]
        recs.append(dict(pre=pre, packed=packed, post=post, ada_pre=ada, ada_post=ada_post, elbo=float(elbo), var_init=vi))
        pre, ada = post, ada_post
    return recs


STEP_REF = {"mcat": global_step_mcat, "poisson": global_step_poisson}
STEP_F64 = {"mcat": global_step_mcat_f64, "poisson": global_step_poisson_f64}
GLB_REF = {"mcat": global_lower_bound_mcat, "poisson": global_lower_bound_poisson}


def prior_tuple(c):
    return (c["prior_tran"],) + tuple(c["prior"])


def case_reference(c, rec):
    ref = STEP_REF[c["fam"]](rec["pre"], prior_tuple(c), rec["packed"], c["rho"], c["bA"], c["bE"], c["B"],
                             ada_G=rec["ada_pre"])
    return ref, GLB_REF[c["fam"]](rec["post"], prior_tuple(c))


def got_dict(c, post, ada_post=None):
    d = {"var_tran": post[0]}
    if c["fam"] == "mcat":
        d["alpha"] = np.concatenate(list(post[1:]), axis=1)
    else:
        d["a"], d["b"] = post[1], post[2]
    if ada_post is not None:
        d["ada_G"] = ada_post
    return d


def case_step_f64(c, rec):
    return STEP_F64[c["fam"]](rec["pre"], prior_tuple(c), rec["packed"], c["rho"], c["bA"], c["bE"], c["B"],
                              ada_G=rec["ada_pre"])


def elbo_f64_of(c, post, lb):
    """the device's ELBO assembly in float64 from a post-state and lb"""
    rowterm, pc = R.rowterms_f64(c["prior_tran"], post[0])
    if c["fam"] == "mcat":
        vlb = mcat_vlb_f64(post[1:], c["prior"])
    else:
        vlb = poisson_vlb_f64(post[1], post[2], *c["prior"])
    return R.elbo_f64(lb, vlb, rowterm, pc)


def elbo_error(got, lb, glb):
    v, a = glb
    with mp.workdps(40):
        return float(abs(mp.mpf(float(got)) - (mp.mpf(float(lb)) + v)) / (ELBO_MULT * R.F64_EPS * a))


def synthetic_packed(c, seed=0):
    """Packed statistics of the case's windows under random posteriors (NumPy; no E-step): what the CPU restatement
    tests feed the step.  An empty shard gives all zeros."""
    from pysvihmm_amd.engine import PackedMCatStats, PackedPoissonStats
    K, D, fam = c["K"], c["D"], c["fam"]
    rng = np.random.default_rng(seed + K)
    cls, arg = (PackedMCatStats, c["shape"]) if fam == "mcat" else (PackedPoissonStats, D)
    st = cls(np.zeros(cls.size(K, arg)), K, arg)
    for s in c["starts"][0]:
        x = c["obs"][s:s + c["Lm"]].astype(int)
        q = rng.dirichlet(np.full(K, 0.3), size=c["Lm"])
        st.A_raw[:] += q[np.arange(-1, c["Lm"] - 1)].T @ q
        for d in range(D):
            if fam == "mcat":
                np.add.at(st.col_counts[d].T, x[:, d], q)
            else:
                st.sx[:, d] += q.T @ x[:, d]
                st.n[:, d] += q.sum(0)
        st.lb[0] -= 40.0 * rng.random()
    return st


# ---------------------------------------------------------------------------------------------------
#  the host-stepped route at engine level (test 7, tools/bench_svi_families.py's baseline): SciPy tables ->
#  set_emission_* -> estep -> the NumPy rules -> next iteration
# ---------------------------------------------------------------------------------------------------
def push_state(eng, fam, var_tran, factors, max_count):
    """Globals and tables of a state on the host (SciPy) -> set_globals + set_emission_*; returns var_init."""
    from scipy.special import digamma
    K = var_tran.shape[0]
    A_mean = var_tran / var_tran.sum(1)[:, None]
    pi = np.linalg.solve(A_mean.T - np.eye(K) + 1.0, np.ones(K))
    vi = pi / np.sqrt(pi @ pi)
    eng.set_globals(digamma(vi + 1e-9) - digamma(vi.sum() + 1e-9),
                    digamma(var_tran + 1e-9) - digamma(var_tran.sum(1)[:, None] + 1e-9))
    if fam == "mcat":
        eng.set_emission_mcat([digamma(a) - digamma(a.sum(1))[:, None] for a in factors])
    else:
        eng.set_emission_poisson(digamma(factors[0]) - np.log(factors[1]), factors[0] / factors[1], max_count)
    return vi


def host_stepped(eng, fam, prior_tran, var_tran, prior, factors, max_count, iters):
    """``iters`` = [(starts, Lm, flags, rho, bA, bE, inner)], obs already resident.  -> (var_tran, var_init, factors,
    elbo[len(iters)]) with the arithmetic of hmmsgd_metaobs.VBHMM's host loop (float64)."""
    from pysvihmm_amd.hmmbase import dirichlet_elbo
    from pysvihmm_amd.distributions import ProductCategorical, ProductPoisson
    K = var_tran.shape[0]
    vt = np.array(var_tran, dtype=np.float64)
    fac = [np.array(f, dtype=np.float64) for f in factors]
    elbo, vi = [], None
    for starts, Lm, flags, rho, bA, bE, inner in iters:
        vi = push_state(eng, fam, vt, fac, max_count)
        st = eng.estep(starts, Lm, flags=flags, inner=inner)
        nwin = len(starts)
        vt = ((1.0 - rho) * (vt - 1.0) + rho * (bA * (st.A_raw + nwin * (prior_tran - 1.0)))) + 1.0
        if fam == "mcat":
            fac = [((1.0 - rho) * (a - 1.0) + (rho * bE) * (nwin * (a0 - 1.0) + cnt)) + 1.0
                   for a, a0, cnt in zip(fac, prior, st.col_counts)]
            vlb = sum(ProductCategorical(weights=[x[k] / x[k].sum() for x in fac], alphav_0=[x[k] for x in prior],
                                         alpha_mf=[x[k] for x in fac]).get_vlb() for k in range(K))
        else:
            fac = [(1.0 - rho) * fac[0] + rho * (prior[0] + bE * st.sx), (1.0 - rho) * fac[1] + rho * (prior[1] + bE * st.n)]
            vlb = sum(ProductPoisson(prior[0][k], prior[1][k], fac[0][k], fac[1][k], max_count).get_vlb() for k in range(K))
        elbo.append(float(st.lb[0]) + dirichlet_elbo(prior_tran, vt) + vlb)
    return vt, vi, fac, np.array(elbo)
