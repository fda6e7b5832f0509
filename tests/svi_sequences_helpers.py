"""The resident SVI loop on minibatches of whole sequences (svihmm_svi_sequences / svihmm_svi_iteration_sequences):
referee of the sequence step and of the bound with the learned initial-state factor, float64 restatements of the
device's expressions, the cases and the host-stepped route.  Shared by tests/test_svi_sequences_ref.py (CPU) and
tests/test_gpu_svi_sequences.py; built on tests/svi_referee.py, tests/svi_cases.py and tests/svi_family_helpers.py,
which it imports unchanged.  Only tests import this module.

The sequence step (include/svihmm.h), bf = N / M:
  var_init' = (1 - rho) var_init + rho (prior_init + bf q0)
  var_tran' = ((1 - rho)(var_tran - 1) + rho ((prior_tran - 1) + bf A_raw)) + 1                 (the prior once)
  NIW, diagonal, Poisson factors: the window loop's blends with bE = bf (they take the prior once already)
  Categorical, multi-column Categorical: alpha' = ((1 - rho)(alpha - 1) + rho ((alpha0 - 1) + bf counts)) + 1
  elbo = bf lb + dirichlet(prior_init, var_init') + sum_i dirichlet_row_i(prior_tran, var_tran') + sum_k vlb_k
"""
import mpmath as mp
import numpy as np

from tests import svi_cases as C
from tests import svi_family_helpers as H
from tests import svi_referee as R
from tests.svi_referee import LD, ld

TRANS_WRAP, MASK_AS_NAN = 2, 1
LENGTHS = (1, 2, 9, 17, 33, 64, 70)          # T = 196
IDX = (5, 0, 3, 3, 6)                        # a duplicate and a one-row sequence
BF = 7.0 / 5.0
POIS_C = H.POIS_C

# (family, K, shape, lengths, idx)   shape = D (niw, diag, poisson), V (cat) or the tuple of V_d (mcat)
SEQ_CASES = [
    ("niw", 5, 3, LENGTHS, IDX),
    ("niw", 4, 20, LENGTHS, IDX),                      # the merged step-and-theta launch (D = 17 .. 32)
    ("diag", 5, 3, LENGTHS, IDX),
    ("cat", 5, 70, LENGTHS, IDX),
    ("mcat", 5, (2, 3, 1, 70), LENGTHS, IDX),
    ("poisson", 65, 2, LENGTHS, IDX),                  # k_seq_block, two-trip loops
    ("poisson", 4, 2, (2100, 40, 9), (0, 2)),          # the chain-routed scan inside the loop
]
RHOS = (1.0, 0.37)


def case_id(c):
    shp = c[2]
    s = "x".join(str(v) for v in shp) if isinstance(shp, tuple) else str(shp)
    return "%s-K%d-%s-T%d" % (c[0], c[1], s, sum(c[3]))


def offsets(lengths):
    return np.concatenate(([0], np.cumsum(lengths))).astype(np.int64)


def seq_case(fam, K, shape, lengths, idx, rho):
    """Factors, priors and the transition factor of the window-loop cases (tests/svi_cases.step_case,
    tests/svi_family_helpers.family_case: kappa over 1e-2 .. 1e6, Gamma shapes over 1e-2 .. 1e6, ...) on
    sum(lengths) resident rows of the family's kind; var_init spread over 1e-2 .. 1e4, prior_init in 0.5 .. 1.5."""
    T = int(sum(lengths))
    if fam in ("niw", "diag", "cat"):
        b = C.step_case(fam, K, shape, rho, "counts")
    else:
        b = H.family_case(fam, K, shape, rho, "counts")
    rng = np.random.default_rng(4000 + 17 * K + T)
    c = dict(fam=fam, K=K, shape=shape, D=b["D"], rho=float(rho), lengths=tuple(lengths), idx=np.asarray(idx, dtype=np.int32),
             T=T, bf=len(lengths) / float(len(idx)), var_tran=b["var_tran"], prior_tran=b["prior_tran"],
             factors=b["factors"], prior=b["prior"], mask=None)
    sts = np.repeat(rng.integers(0, K, size=T // 6 + 1), 6)[:T]
    if fam in ("niw", "diag"):
        c["obs"] = np.asarray(b["factors"][0])[sts] + rng.normal(size=(T, b["D"]))
    elif fam == "cat":
        c["obs"] = rng.integers(0, shape, size=(T, 1)).astype(np.float64)
    elif fam == "mcat":
        c["obs"] = np.stack([rng.integers(0, v, size=T) for v in shape], axis=1).astype(np.float64)
    else:
        obs = rng.poisson(5.0, size=(T, shape))
        wild = rng.random((T, shape)) < 0.1
        obs[wild] = rng.integers(0, POIS_C + 1, size=int(wild.sum()))
        c["obs"] = obs.astype(np.float64)
    c["var_init"] = 10.0 ** (rng.permutation(np.linspace(-2.0, 4.0, K)) if K > 1 else np.array([1.0]))
    c["prior_init"] = 0.5 + rng.random(K)
    return c


def state_of(c, var_tran, fac):
    """(var_tran, factor arrays ..) in the layout the referees of the family take"""
    return (var_tran,) + ((fac,) if c["fam"] == "cat" else tuple(fac))


def prior_of(c):
    return (c["prior_tran"],) + ((c["prior"],) if c["fam"] == "cat" else tuple(c["prior"]))


def begin(eng, c, maxit=2):
    """set_obs + set_sequences + svi_begin* + svi_sequences of a case"""
    from pysvihmm_amd.distributions import niw_prior_logpart
    eng.set_obs(c["obs"], c["mask"])
    eng.set_sequences(np.asarray(c["lengths"]))
    begin_family(eng, c["fam"], c["prior_tran"], c["var_tran"], c["prior"], c["factors"], maxit)
    eng.svi_sequences(c["prior_init"], c["var_init"])


def begin_family(eng, fam, prior_tran, var_tran, prior, factors, maxit, max_count=POIS_C):
    from pysvihmm_amd.distributions import niw_prior_logpart
    if fam == "niw":
        eng.svi_begin(prior_tran, var_tran, prior, factors, niw_prior_logpart(prior[1], prior[3]), maxit, 1.0)
    elif fam == "diag":
        eng.svi_begin_diag(prior_tran, var_tran, prior, factors, maxit)
    elif fam == "cat":
        eng.svi_begin_cat(prior_tran, var_tran, prior, factors, maxit)
    elif fam == "mcat":
        eng.svi_begin_mcat(prior_tran, var_tran, prior, factors, maxit)
    else:
        eng.svi_begin_poisson(prior_tran, var_tran, prior, factors, max_count, maxit)


def read_state(eng, fam):
    """(var_tran, var_init, factors) of the loop, the factors as the family's begin call takes them"""
    if fam == "niw":
        s = eng.svi_read_state()
        return s[0], s[1], tuple(s[2:])
    return eng.svi_read_factors()


def q0_of(var_x, lengths, idx):
    """sum of the occurrences' first posterior rows, added in ascending m, from var_x [R, K] in the order of idx"""
    q0 = np.zeros(var_x.shape[1])
    r = 0
    for s in idx:
        q0 = q0 + var_x[r]
        r += int(lengths[s])
    return q0


# ---------------------------------------------------------------------------------------------------
#  referee of the step: {name: (value, scale)} in longdouble, as tests/svi_referee.global_step_*
# ---------------------------------------------------------------------------------------------------
def init_step(var_init, prior_init, q0, rho, bf):
    vi, pi, q = ld(var_init), ld(prior_init), ld(q0)
    rho, bf = LD(rho), LD(bf)
    new = (1 - rho) * vi + rho * (pi + bf * q)
    return new, np.abs(1 - rho) * np.abs(vi) + np.abs(rho) * (np.abs(pi) + np.abs(bf * q))


def tran_step(var_tran, prior_tran, A_raw, rho, bf):
    """(vt - 1 and pt - 1 are single correctly rounded operations on given numbers: the differences are the terms)"""
    vt, pt, A = ld(var_tran), ld(prior_tran), ld(A_raw)
    rho, bf = LD(rho), LD(bf)
    new = ((1 - rho) * (vt - 1) + rho * ((pt - 1) + bf * A)) + 1
    return new, np.abs(1 - rho) * np.abs(vt - 1) + np.abs(rho) * (np.abs(pt - 1) + np.abs(bf * A)) + 1


def dirichlet_step(alpha, alpha0, counts, rho, bf):
    al, al0, c = ld(alpha), ld(alpha0), ld(counts)
    rho, bf = LD(rho), LD(bf)
    new = ((1 - rho) * (al - 1) + rho * ((al0 - 1) + bf * c)) + 1
    return new, np.abs(1 - rho) * np.abs(al - 1) + np.abs(rho) * (np.abs(al0 - 1) + np.abs(bf * c)) + 1


_WINDOW_STEP = {"niw": R.global_step_niw, "diag": R.global_step_diag, "poisson": H.global_step_poisson}


def global_step(fam, state, prior, packed, q0, var_init, prior_init, rho, bf):
    """One sequence step.  ``state`` / ``prior`` as the family's window referee takes them.  The emission blends of
    NIW, diagonal and Poisson are the window referees' with bE = bf (the prior enters them once); their var_tran is
    replaced by the sequence form."""
    if fam in _WINDOW_STEP:
        out = _WINDOW_STEP[fam](state, prior, packed, rho, bf, bf, 1)
    elif fam == "cat":
        out = {"alpha": dirichlet_step(state[1], prior[1], packed.counts, rho, bf)}
    else:
        cat = lambda xs: np.concatenate([np.asarray(x) for x in xs], axis=1)
        out = {"alpha": dirichlet_step(cat(state[1:]), cat(prior[1:]), packed.flat, rho, bf)}
    out["var_tran"] = tran_step(state[0], prior[0], packed.A_raw, rho, bf)
    out["var_init"] = init_step(var_init, prior_init, q0, rho, bf)
    return out


# float64 restatements of the device expressions (svi_tran_step's sequence branch, svi_dirichlet_seq_step)
_WINDOW_STEP_F64 = {"niw": R.global_step_niw_f64, "diag": R.global_step_diag_f64, "poisson": H.global_step_poisson_f64}


def global_step_f64(fam, state, prior, packed, q0, var_init, prior_init, rho, bf):
    f = lambda a: np.asarray(a, dtype=np.float64)
    if fam in _WINDOW_STEP_F64:
        out = _WINDOW_STEP_F64[fam](state, prior, packed, rho, bf, bf, 1)
    elif fam == "cat":
        out = {"alpha": ((1.0 - rho) * (f(state[1]) - 1.0) + rho * ((f(prior[1]) - 1.0) + bf * packed.counts)) + 1.0}
    else:
        al, al0 = (np.concatenate([f(x) for x in s], axis=1) for s in (state[1:], prior[1:]))
        out = {"alpha": ((1.0 - rho) * (al - 1.0) + rho * ((al0 - 1.0) + bf * packed.flat)) + 1.0}
    out["var_tran"] = ((1.0 - rho) * (f(state[0]) - 1.0) + rho * ((f(prior[0]) - 1.0) + bf * packed.A_raw)) + 1.0
    out["var_init"] = (1.0 - rho) * f(var_init) + rho * (f(prior_init) + bf * f(q0))
    return out


def got_dict(fam, var_tran, var_init, fac):
    d = {"var_tran": var_tran, "var_init": var_init}
    if fam == "cat":
        d["alpha"] = fac
    elif fam == "mcat":
        d["alpha"] = np.concatenate(list(fac), axis=1)
    elif fam == "poisson":
        d["a"], d["b"] = fac
    else:
        d.update(zip(C.FACTOR_NAMES[fam], fac))
    return d


# ---------------------------------------------------------------------------------------------------
#  the global lower bound with the initial factor: (value, sum|terms|) in mpmath; the device's assembly in float64
# ---------------------------------------------------------------------------------------------------
_GLB = {"niw": R.global_lower_bound_niw, "diag": R.global_lower_bound_diag, "cat": R.global_lower_bound_cat,
        "mcat": H.global_lower_bound_mcat, "poisson": H.global_lower_bound_poisson}


def global_lower_bound(fam, state, prior, var_init, prior_init, dps=30):
    v, a = _GLB[fam](state, prior)
    vi, ai = R.dirichlet_rows(np.asarray(prior_init)[None, :], np.asarray(var_init)[None, :], dps)
    return v + vi, a + ai


def elbo_error(got, bf, lb, glb):
    """|got - (bf lb + glb)| in units of ELBO_MULT eps sum|terms| (sum|terms| of the global lower bound alone, as
    tests/svi_cases.elbo_error)"""
    v, a = glb
    with mp.workdps(40):
        lz = mp.mpf(float(bf)) * mp.mpf(float(lb))
        return float(abs(mp.mpf(float(got)) - (lz + v)) / (C.ELBO_MULT * R.F64_EPS * a))


def elbo_f64(fam, state, prior, var_init, prior_init, bf, lb):
    """k_svi_elbo_body with the initial factor's row: bf lb + ((sum rowterm + init term) + prior constants) + sum vlb"""
    from pysvihmm_amd.distributions import niw_prior_logpart
    rowterm, pc = R.rowterms_f64(prior[0], state[0])
    it, pci = R.rowterms_f64(np.asarray(prior_init)[None, :], np.asarray(var_init)[None, :])
    if fam == "niw":
        vlb = R.niw_vlb_f64(*(tuple(state[1:]) + tuple(prior[1:]) + (niw_prior_logpart(prior[2], prior[4]), 1.0)))
    elif fam == "diag":
        vlb = R.diag_vlb_f64(state[1:], prior[1:])
    elif fam == "cat":
        vlb = R.cat_vlb_f64(state[1], prior[1])
    elif fam == "mcat":
        vlb = H.mcat_vlb_f64(state[1:], prior[1:])
    else:
        vlb = H.poisson_vlb_f64(state[1], state[2], prior[1], prior[2])
    return R.elbo_f64(bf * float(lb), vlb, list(rowterm) + [it[0]], pc + pci)


# ---------------------------------------------------------------------------------------------------
#  statistics without an E-step (the CPU restatement tests): random posteriors over the listed rows
# ---------------------------------------------------------------------------------------------------
def synthetic_packed(c, seed=0):
    """(packed view, q0) of the case's listed sequences under random posteriors, in NumPy"""
    from pysvihmm_amd.engine import (PackedStats, PackedDiagStats, PackedCatStats, PackedMCatStats, PackedPoissonStats)
    K, D, fam = c["K"], c["D"], c["fam"]
    rng = np.random.default_rng(seed + K)
    cls, arg = {"niw": (PackedStats, D), "diag": (PackedDiagStats, D), "cat": (PackedCatStats, c["shape"]),
                "mcat": (PackedMCatStats, c["shape"]), "poisson": (PackedPoissonStats, D)}[fam]
    st = cls(np.zeros(cls.size(K, arg)), K, arg)
    off = offsets(c["lengths"])
    q0 = np.zeros(K)
    for s in c["idx"]:
        x = c["obs"][off[s]:off[s + 1]]
        n = x.shape[0]
        q = rng.dirichlet(np.full(K, 0.3), size=n)
        q0 += q[0]
        st.A_raw[:] += q[np.arange(-1, n - 1)].T @ q          # (wrap)
        if fam in ("niw", "diag"):
            st.xbar[:] += q.T @ x
            st.neff[:] += q.sum(0)
            if fam == "niw":
                st.S[:] += np.einsum("tk,ta,tb->kab", q, x, x)
            else:
                st.xsq[:] += q.T @ (x * x)
        elif fam == "cat":
            np.add.at(st.counts.T, x[:, 0].astype(int), q)
        else:
            xi = x.astype(int)
            for d in range(D):
                if fam == "mcat":
                    np.add.at(st.col_counts[d].T, xi[:, d], q)
                else:
                    st.sx[:, d] += q.T @ xi[:, d]
                    st.n[:, d] += q.sum(0)
        st.lb[0] -= 40.0 * rng.random()
    return st, q0


# ---------------------------------------------------------------------------------------------------
#  the host-stepped route at engine level: SciPy psi -> set_globals -> set_emission_* -> estep_sequence_subset -> the
#  NumPy rules of hmmbatchsgd._global_update_from_stats -> lower_bound
# ---------------------------------------------------------------------------------------------------
def _emitters(fam, K, prior, fac, max_count):
    from pysvihmm_amd.distributions import Gaussian, ProductCategorical, ProductPoisson
    out = []
    for k in range(K):
        if fam == "niw":
            # (mu / sigma given: no draw from the prior; the mean-field factor is (mu, sigma, kappa_mf, nu_mf))
            G = Gaussian(mu=fac[0][k], sigma=fac[1][k], mu_0=prior[0][k], sigma_0=prior[1][k], kappa_0=float(prior[2][k]),
                         nu_0=float(prior[3][k]), kappa_mf=float(fac[2][k]), nu_mf=float(fac[3][k]))
        elif fam == "mcat":
            G = ProductCategorical(weights=[x[k] / x[k].sum() for x in fac], alphav_0=[x[k] for x in prior],
                                   alpha_mf=[x[k] for x in fac])
        else:
            G = ProductPoisson(prior[0][k], prior[1][k], fac[0][k], fac[1][k], max_count)
        out.append(G)
    return np.array(out, dtype=object)


def host_stepped(eng, fam, lengths, prior_init, var_init, prior_tran, var_tran, prior, factors, iters, max_count):
    """``iters`` = [(idx, flags, rho)], obs and the declaration already on ``eng``.  One ``hmmbatchsgd.VBHMM`` object
    lends ``_sequence_subset_estep`` (SciPy psi -> set_globals -> set_emission_* -> estep_sequence_subset),
    ``_global_update_from_stats`` and ``lower_bound``; the engine's rows are the caller's (never uploaded again).
    -> (var_tran, var_init, emitters, elbo)."""
    from pysvihmm_amd import hmmbatchsgd
    from pysvihmm_amd.engine import rewrap_packed
    K, N = var_tran.shape[0], len(lengths)
    m = hmmbatchsgd.VBHMM.__new__(hmmbatchsgd.VBHMM)
    off = offsets(lengths)
    emit = _emitters(fam, K, prior, factors, max_count)
    m.__dict__.update(prior_init=np.array(prior_init, dtype=float), prior_tran=np.array(prior_tran, dtype=float),
                      var_init=np.array(var_init, dtype=float), var_tran=np.array(var_tran, dtype=float), var_emit=emit,
                      K=K, D=eng.D, T=int(off[-1]), seq_off=off, _engine=eng, obs=np.zeros((int(off[-1]), eng.D)),
                      mask=np.zeros(int(off[-1]), dtype=bool), _obs_dirty=False, seq_minibatch=1, _lZ=None)
    eng._obs_owner = id(m)
    elbo = []
    for idx, flags, rho in iters:
        m.lrate = rho
        m.batchfactor = bf = N / float(len(idx))
        m._psi_expectations()
        m._push_globals()
        m._push_emission()
        st, _, q0 = eng.estep_sequence_subset(idx, flags=flags)
        m._q0 = q0
        m._lZ = bf * float(st.lb[0])
        m._global_update_from_stats(rewrap_packed(st, st.buf * bf))
        elbo.append(m.lower_bound())
    return m.var_tran, m.var_init, m.var_emit, np.array(elbo)


def emitter_factors(fam, emit):
    if fam == "niw":
        return [np.array([np.asarray(getattr(g, n), dtype=float) for g in emit]) for n in ("mu_mf", "sigma_mf", "kappa_mf", "nu_mf")]
    if fam == "mcat":
        return [np.array([g.alpha_mf[d] for g in emit]) for d in range(emit[0].D)]
    return [np.array([g.alpha_mf for g in emit]), np.array([g.beta_mf for g in emit])]
