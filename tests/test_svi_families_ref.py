"""CPU: hmmsgd_metaobs.VBHMM on ProductCategorical / ProductPoisson emitters (the host loop, on the oracle engine)
and the referees of tests/svi_family_helpers.py.

The oracle engine has neither family, so the class runs the literal per-window loop there: lliks from the emitters'
``expected_log_likelihood``, ``_intermediate`` per window, ``global_update``.  Rules:
  ProductCategorical  per column the Categorical rule (hmmsgd_metaobs.py:907-926, 1071-1084): every window
                      contributes alpha0 + counts - 1
  ProductPoisson      a' = (1 - lrate) a + lrate (a0 + bE sx),  b' = (1 - lrate) b + lrate (b0 + bE n)
"""
import copy

import numpy as np
import numpy.random as npr
import pytest

from oracle import ref_numpy as O
from oracle.engine import OracleEngine
from pysvihmm_amd import hmmsgd_metaobs
from pysvihmm_amd.distributions import Categorical, ProductCategorical, ProductPoisson
from pysvihmm_amd.engine import PackedMCatStats, PackedPoissonStats
from pysvihmm_amd.hmmbase import dirichlet_elbo
from tests import svi_cases as C
from tests import svi_family_helpers as H
from tests import svi_referee as R

EPS = R.F64_EPS
HALF, MB, MAXIT, SEED = 6, 5, 3, 4


def _data(fam, T, seed, V=(2, 3, 1), D=2, holes=False):
    """[T, D] symbols / counts from a sticky 3-state chain, 10 % masked rows; ``holes``: column 1 NaN in a third of
    the rows, out-of-range entries in column 0."""
    rng = np.random.default_rng(seed)
    sts = np.repeat(rng.integers(0, 3, size=T // 8 + 1), 8)[:T]
    if fam == "mcat":
        th = [rng.dirichlet(np.ones(v) * 0.5, size=3) for v in V]
        obs = np.stack([[rng.choice(len(t[s]), p=t[s]) for s in sts] for t in th], axis=1).astype(float)
    else:
        obs = rng.poisson(np.array([1.0, 6.0, 15.0])[sts][:, None] * np.linspace(1.0, 2.0, D)[None, :]).astype(float)
    mask = rng.random(T) < 0.1
    if holes:
        obs[rng.permutation(T)[:T // 3], 1] = np.nan
        bad = rng.permutation(T)[:T // 10]
        obs[bad[::2], 0] = -1.0
        obs[bad[1::2], 0] = 1e6
    return obs, mask


def _emitters(fam, K, V=(2, 3, 1), D=2):
    if fam == "mcat":
        return np.array([ProductCategorical(alphav_0=[np.ones(v) * 1.5 for v in V]) for _ in range(K)])
    return np.array([ProductPoisson(np.full(D, 2.0), np.full(D, 0.5), max_count=60) for _ in range(K)])


def _make(fam, obs, mask, engine, K=3, emit=None, maxit=MAXIT, **kw):
    np.random.seed(SEED)
    emit = _emitters(fam, K, D=obs.shape[1]) if emit is None else emit
    return hmmsgd_metaobs.VBHMM(obs.copy(), np.ones(K), np.ones((K, K)), emit, tau=1.0, kappa=0.7, metaobs_half=HALF,
                                mb_sz=MB, mask=mask, maxit=maxit, seed=SEED, engine=engine, **kw)


def _window_inter(fam, emit, q, x, m):
    """``_intermediate``'s emission part for one window by explicit row loops: per state the columns' alpha0 + counts
    - 1 side by side, respectively [sx | n]."""
    K = q.shape[1]
    out = []
    for k in range(K):
        G = emit[k]
        if fam == "mcat":
            cnt = [np.zeros(len(a0)) for a0 in G.alphav_0]
            for t in range(x.shape[0]):
                if m[t]:
                    continue
                for d, a0 in enumerate(G.alphav_0):
                    v = x[t, d]
                    if not np.isnan(v) and 0 <= int(v) < len(a0):
                        cnt[d][int(v)] += q[t, k]
            out.append(np.concatenate([a0 + c - 1.0 for a0, c in zip(G.alphav_0, cnt)]))
        else:
            sx, n = np.zeros(G.D), np.zeros(G.D)
            for t in range(x.shape[0]):
                if m[t]:
                    continue
                for d in range(G.D):
                    v = x[t, d]
                    if v >= 0.0 and v < G.max_count + 1:
                        sx[d] += q[t, k] * int(v)
                        n[d] += q[t, k]
            out.append(np.stack([sx, n]))
    return out


def _literal_loop(fam, model):
    """The host loop of hmmsgd_metaobs.VBHMM.infer restated in NumPy from a freshly constructed ``model`` (not
    inferred): same random stream, per window E-step from the emitters' expected_log_likelihood, the rules of the
    module docstring, ELBO from get_vlb.  -> (var_tran, emitters, elbo_vec, var_x of the last window)."""
    obs, mask, T, K = model.obs, model.mask, model.T, model.K
    pt, vt = model.prior_tran.copy(), model.var_tran.copy()
    emit = [copy.deepcopy(e) for e in model.var_emit]
    ada_G = np.ones((K, K)) if model.adagrad else None
    bA = (T - 2 * HALF - 1) / (2.0 * HALF * MB)
    bE = (T - 2 * HALF - 1) / ((2.0 * HALF + 1.0) * MB)
    elbo = np.empty(model.maxit)
    np.random.seed(model.seed)
    q = None
    for it in range(model.maxit):
        lrate = (it + model.tau) ** (-model.kappa)
        A_inter = np.zeros((K, K))
        e_inter = None
        lb = 0.0
        for c in npr.randint(HALF, T - 1 - HALF + 1, MB):
            lo, hi = c - HALF, c + HALF
            A_mean = vt / vt.sum(1)[:, None]
            pi = np.linalg.solve(A_mean.T - np.eye(K) + 1.0, np.ones(K))
            mod_init, mod_tran = O.psi_expectations(pi / np.sqrt(pi @ pi), vt)
            x, m = obs[lo:hi + 1], mask[lo:hi + 1]
            ll = np.stack([np.nan_to_num(e.expected_log_likelihood(x)) for e in emit], axis=1)
            la = O.forward_msgs(ll, mod_init, mod_tran)
            q = O.posterior(la, O.backward_msgs(ll, mod_tran))
            lb += O.local_lower_bound(la)
            A_inter += (pt - 1.0) + O.transition_stat_wrap(q)
            w = _window_inter(fam, emit, q, x, m)
            e_inter = w if e_inter is None else [a + b for a, b in zip(e_inter, w)]
        nat = vt - 1.0
        if ada_G is not None:
            ada_G += nat ** 2
            am = ada_G ** 0.25
            vt = (1.0 - 1.0 / am) * nat + bA * A_inter / am + 1.0
        else:
            vt = (1.0 - lrate) * nat + lrate * (bA * A_inter) + 1.0
        for k, G in enumerate(emit):
            if fam == "mcat":
                new = (1.0 - lrate) * (np.concatenate(G.alpha_mf) - 1.0) + lrate * bE * e_inter[k] + 1.0
                G._set_alpha(np.split(new, np.cumsum(G.V)[:-1]))
            else:
                sx, n = e_inter[k]
                G._set_mf((1.0 - lrate) * G.alpha_mf + lrate * (G.alpha_0 + bE * sx),
                          (1.0 - lrate) * G.beta_mf + lrate * (G.beta_0 + bE * n))
        elbo[it] = lb + dirichlet_elbo(pt, vt) + sum(G.get_vlb() for G in emit)
    return vt, emit, elbo, q


def _factor_arrays(fam, G):
    return list(G.alpha_mf) if fam == "mcat" else [G.alpha_mf, G.beta_mf]


def _assert_matches_literal(fam, a, ref):
    vt, emit, elbo, q = ref
    np.testing.assert_allclose(a.var_tran, vt, rtol=1e-10, atol=1e-9)
    np.testing.assert_allclose(a.elbo_vec, elbo, rtol=1e-8)
    for G, H_ in zip(a.var_emit, emit):
        for x, y in zip(_factor_arrays(fam, G), _factor_arrays(fam, H_)):
            np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-9)
        if fam == "mcat":
            for x, y in zip(G.weights, H_.weights):
                np.testing.assert_allclose(x, y, rtol=1e-10, atol=1e-10)
    np.testing.assert_allclose(a.var_x, q, rtol=1e-9, atol=1e-11)


@pytest.mark.parametrize("adagrad", [False, True])
@pytest.mark.parametrize("fam", ["poisson", "mcat"])
def test_host_loop_runs_and_matches_a_literal_restatement(fam, adagrad):
    """K = 3, T = 400, ProductPoisson with D = 2 / ProductCategorical with V = (2, 3, 1) on the oracle engine:
    infer() runs the host loop and equals its NumPy restatement at the tolerances of test_categorical._close_cat
    with rtol 1e-10.  (Before the families entered the class, the loop raised in util.NIW_zero_nat_pars.)"""
    obs, mask = _data(fam, 400, 11)
    a = _make(fam, obs, mask, OracleEngine(), adagrad=adagrad)
    assert not a._svi_device_ok()          # the oracle engine has no svi_begin_mcat / _poisson: the host loop
    ref = _literal_loop(fam, _make(fam, obs, mask, OracleEngine(), adagrad=adagrad))
    a.infer()
    assert np.all(np.isfinite(a.elbo_vec))
    _assert_matches_literal(fam, a, ref)
    for G in a.var_emit:
        assert min(x.min() for x in _factor_arrays(fam, G)) > 0


@pytest.mark.parametrize("adagrad", [False, True])
def test_one_column_product_categorical_reproduces_categorical(adagrad):
    """ProductCategorical with D = 1 against Categorical, same data and seed: var_tran, alpha_mf and elbo_vec are
    equal.  Both run the literal per-window loop (``fused=False`` for Categorical, whose default on this engine takes
    the minibatch's counts in one call and so adds the windows in another order, 1e-14 apart; the oracle engine
    offers ProductCategorical no other route)."""
    V, K, T = 5, 3, 400
    rng = np.random.default_rng(2)
    obs = rng.integers(0, V, size=(T, 1)).astype(float)
    mask = rng.random(T) < 0.1
    np.random.seed(SEED)
    a = _make("cat", obs, mask, OracleEngine(), emit=np.array([Categorical(alphav_0=np.ones(V) * 1.5) for _ in range(K)]),
              adagrad=adagrad)
    np.random.seed(SEED)
    b = _make("mcat", obs, mask, OracleEngine(),
              emit=np.array([ProductCategorical(alphav_0=[np.ones(V) * 1.5]) for _ in range(K)]), adagrad=adagrad)
    for k in range(K):
        np.testing.assert_array_equal(a.var_emit[k].alpha_mf, b.var_emit[k].alpha_mf[0])
    a.infer(fused=False)
    b.infer()
    np.testing.assert_array_equal(a.var_tran, b.var_tran)
    np.testing.assert_array_equal(a.elbo_vec, b.elbo_vec)
    for k in range(K):
        np.testing.assert_array_equal(a.var_emit[k].alpha_mf, b.var_emit[k].alpha_mf[0])
    assert not np.array_equal(a.var_tran, np.ones((K, K)))


@pytest.mark.parametrize("fam", ["poisson", "mcat"])
def test_missing_data_reaches_the_step_per_column(fam):
    """Column 1 NaN in a third of the rows, out-of-range entries in column 0, masked rows: ``_intermediate`` equals
    the explicit row loops, the statistics differ between the columns (n[k][0] != n[k][1]), ``_stats_to_inter`` of
    the same statistics in the engine's packed layout gives the same direction, and the whole loop still equals its
    restatement."""
    obs, mask = _data(fam, 400, 12, holes=True)
    a = _make(fam, obs, mask, OracleEngine())
    K, lo, hi = a.K, 100, 130
    rng = np.random.default_rng(0)
    q = rng.dirichlet(np.ones(K), size=hi - lo + 1)
    assert mask[lo:hi + 1].any() and np.isnan(obs[lo:hi + 1, 1]).any()
    A_i, e_i = a._intermediate(q, lo, hi)
    want = _window_inter(fam, a.var_emit, q, obs[lo:hi + 1], mask[lo:hi + 1])
    np.testing.assert_allclose(A_i, (a.prior_tran - 1.0) + O.transition_stat_wrap(q), rtol=1e-13)
    for k in range(K):
        np.testing.assert_allclose(e_i[k], want[k], rtol=1e-13, atol=1e-14)
    if fam == "poisson":
        st = PackedPoissonStats(np.zeros(PackedPoissonStats.size(K, 2)), K, 2)
        for k in range(K):
            st.sx[k], st.n[k] = want[k]
            assert abs(st.n[k, 0] - st.n[k, 1]) > 1e-3         # per column: the holes differ
    else:
        V = a.var_emit[0].V
        st = PackedMCatStats(np.zeros(PackedMCatStats.size(K, V)), K, V)
        for k in range(K):
            st.flat[k] = want[k] - (np.concatenate(a.var_emit[k].alphav_0) - 1.0)
        tot = [c.sum(1) for c in st.col_counts]
        assert np.all(np.abs(tot[0] - tot[1]) > 1e-3)
    st.A_raw[:] = O.transition_stat_wrap(q)
    A_s, e_s = a._stats_to_inter(st, 1)
    np.testing.assert_allclose(A_s, A_i, rtol=1e-13)
    for k in range(K):
        np.testing.assert_allclose(e_s[k], e_i[k], rtol=1e-13, atol=1e-14)
    ref = _literal_loop(fam, _make(fam, obs, mask, OracleEngine()))
    a.infer()
    _assert_matches_literal(fam, a, ref)


def test_vlb_referees_against_the_host_classes():
    """mcat_vlb / poisson_vlb (mpmath) against ProductCategorical / ProductPoisson.get_vlb on mild parameters, and the
    Poisson term vanishes at the prior."""
    rng = np.random.default_rng(5)
    V = (2, 5, 1)
    al = [0.2 + 5 * rng.random(v) for v in V]
    al0 = [0.5 + rng.random(v) for v in V]
    v, s = H.mcat_vlb(al, al0)
    g = ProductCategorical(weights=[x / x.sum() for x in al], alphav_0=al0, alpha_mf=al)
    assert abs(float(v) - g.get_vlb()) <= 64 * EPS * float(s)
    a, b, a0, b0 = 0.3 + 9 * rng.random(4), 0.2 + 3 * rng.random(4), 0.5 + rng.random(4), 0.5 + rng.random(4)
    v, s = H.poisson_vlb(a, b, a0, b0)
    assert abs(float(v) - ProductPoisson(a0, b0, a, b).get_vlb()) <= 64 * EPS * float(s)
    assert float(v) < 0
    v, s = H.poisson_vlb(a0, b0, a0, b0)
    assert abs(float(v)) <= 1e-25 * float(s)


_CASES = [pytest.param(c, id=H.family_case_id(c)) for c in H.FAMILY_CASES]


@pytest.mark.skipif(not R.have_extended_precision(), reason="np.longdouble is not wider than double on this host")
@pytest.mark.parametrize("case", _CASES)
def test_float64_step_and_elbo_restatements_pass_the_gpu_bounds(case):
    """Every case of the GPU test, on the host: the float64 restatements of the device's expressions
    (k_svi_global_step_simple_body fam 3 / svi_pois_step, svi_tran_step, k_svi_vlb_simple_body fam 3 / 4, svi_rowterm,
    k_svi_elbo_body), fed NumPy statistics of random posteriors, are held to the bounds the device is held to: 8 eps
    scale per output element of the step, 16 eps sum|terms| for the ELBO."""
    c = H.family_case(*case)
    rec = dict(pre=(c["var_tran"],) + tuple(c["factors"]), packed=H.synthetic_packed(c),
               ada_pre=np.ones((c["K"], c["K"])) if "adagrad" in c["opts"] else None)
    got = H.case_step_f64(c, rec)
    rec["post"] = (got["var_tran"],) + (tuple(np.split(got["alpha"], np.cumsum(c["shape"])[:-1], axis=1))
                                        if c["fam"] == "mcat" else (got["a"], got["b"]))
    ref, glb = H.case_reference(c, rec)
    errs = R.step_errors(got, ref, C.STEP_MULT)
    lb = rec["packed"].lb[0]
    e_elbo = H.elbo_error(H.elbo_f64_of(c, rec["post"], lb), lb, glb)
    print("%s: step %s, ELBO %.4f of bound (sum|terms| %.3g)"
          % (H.family_case_id(case), {n: round(v, 3) for n, v in errs.items()}, e_elbo, float(glb[1])))
    assert set(errs) == set(ref) and max(errs.values()) <= 1.0, errs
    assert e_elbo <= 1.0, e_elbo
    for x in rec["post"][1:]:
        assert np.all(np.isfinite(x))
    if c["fam"] == "poisson":
        assert min(x.min() for x in rec["post"][1:]) > 0         # positive for every rho in [0, 1]
