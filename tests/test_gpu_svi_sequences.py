"""GPU: the resident SVI loop on minibatches of whole sequences (svihmm_svi_sequences /
svihmm_svi_iteration_sequences, ``hmmbatchsgd.VBHMM.infer(device_loop=...)``).

Base layout: N = 7 sequences of lengths (1, 2, 9, 17, 33, 64, 70), T = 196; idx = [5, 0, 3, 3, 6] (a duplicate and a
one-row sequence); SVIHMM_TRANS_WRAP; bf = 7 / 5.  Referee tests run with automatic centring off, as
tests/test_gpu_svi_globals.py.  Bounds (tests/svi_cases.py): step outputs 8 eps scale, ELBO 16 eps sum|terms|, globals
32 eps max(1, |terms|); tests/test_svi_sequences_ref.py shows a float64 NumPy restatement of each device expression
inside them.  The loop runs on stream order and events: svi_recoveries() stays 0."""
import ctypes

import numpy as np
import pytest

from tests import svi_cases as C
from tests import svi_referee as R
from tests import svi_sequences_helpers as S

pytestmark = pytest.mark.gpu
needs_ld = pytest.mark.skipif(not R.have_extended_precision(), reason="np.longdouble is not wider than double on this host")
WRAP = S.TRANS_WRAP


def _engine(centring_off=True):
    from pysvihmm_amd.engine import HipEngine
    eng = HipEngine(0)
    if centring_off:
        eng.set_variant("centring", 1)
    return eng


# ---------------------------------------------------------------------------------------------------
#  1. step and ELBO against the referee
# ---------------------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("rho", S.RHOS)
@pytest.mark.parametrize("case", [pytest.param(c, id=S.case_id(c)) for c in S.SEQ_CASES])
def test_sequence_step_and_elbo(case, rho):
    """One iteration per case: the state after it against the referee's sequence step fed the state read before, the
    packed statistics the step consumed (read_packed) and q0 formed from var_x of the R listed rows (the occurrences'
    first rows, added in ascending m); svi_read_elbo against bf lb + the referee's bound of the state read back,
    initial factor included.  niw D = 20 takes the merged step-and-theta launch, poisson K = 65 k_seq_block, lengths
    (2100, 40, 9) the chain-routed scan.
    Largest on the device, in units of the bound: sigma 0.198 (niw K = 5, rho 0.37), var_tran 0.156, var_init 0.094;
    ELBO 0.173 on the base layout and 0.906 for the chain-routed case at rho = 1, where bf lb = -9.6e7 stands against
    sum|terms| = 2.7e6 of the global bound (sum|terms| leaves bf lb out, as tests/svi_cases.elbo_error): half an ulp
    of the total alone is 0.79 of that bound."""
    c = S.seq_case(*case, rho=rho)
    fam, idx, bf = c["fam"], c["idx"], c["bf"]
    Rrows = int(sum(c["lengths"][s] for s in idx))
    eng = _engine()
    try:
        S.begin(eng, c)
        vt0, vi0, fac0 = S.read_state(eng, fam)
        eng.svi_iteration_sequences(0, idx, WRAP, rho, bf)
        packed = eng.read_packed()
        var_x = eng.read_rows("var_x", 0, Rrows)
        vt1, vi1, fac1 = S.read_state(eng, fam)
        elbo = float(eng.svi_read_elbo(1)[0][0])
        assert eng.svi_recoveries() == 0
    finally:
        eng.close()
    np.testing.assert_array_equal(vt0, c["var_tran"])
    np.testing.assert_array_equal(vi0, c["var_init"])
    np.testing.assert_allclose(var_x.sum(1), 1.0, rtol=1e-12)
    q0 = S.q0_of(var_x, c["lengths"], idx)
    prior = S.prior_of(c)
    ref = S.global_step(fam, S.state_of(c, vt0, fac0), prior, packed, q0, vi0, c["prior_init"], rho, bf)
    got = S.got_dict(fam, vt1, vi1, fac1)
    assert set(got) == set(ref)
    errs = R.step_errors(got, ref, C.STEP_MULT)
    glb = S.global_lower_bound(fam, S.state_of(c, vt1, fac1), prior, vi1, c["prior_init"])
    e_elbo = S.elbo_error(elbo, bf, packed.lb[0], glb)
    print("FIG seq step %s rho %g: %s ELBO %.4f of bound (elbo %.10g, sum|terms| %.3g)"
          % (S.case_id(case), rho, {n: round(v, 3) for n, v in errs.items()}, e_elbo, elbo, float(glb[1])))
    assert np.isfinite(elbo)
    assert max(errs.values()) <= 1.0, errs
    assert e_elbo <= 1.0, e_elbo


# ---------------------------------------------------------------------------------------------------
#  2. globals
# ---------------------------------------------------------------------------------------------------
@needs_ld
@pytest.mark.parametrize("K", [5, 65, 256])
def test_globals_from_the_learned_initial_factor(K):
    """After the first iteration (M = 1, a 9-row sequence) read_globals returns the globals its E-step ran under:
    mod_init = psi(var_init + eps) - psi(sum + eps) of the learned var_init uploaded (no stationary vector), ltran of
    var_tran; both within 32 eps max(1, |psi|, |psi sum|) of mpmath."""
    c = S.seq_case("poisson", K, 2, (9, 4), (0,), rho=0.37)
    c["var_tran"] = R.tran_family("blocks", K)
    eng = _engine()
    try:
        S.begin(eng, c)
        eng.svi_iteration_sequences(0, c["idx"], WRAP, 0.37, 2.0)
        mi, lt = eng.read_globals()
        assert np.isfinite(eng.svi_read_elbo(1)[0][0])
        assert eng.svi_recoveries() == 0
    finally:
        eng.close()
    ltr, lts, mir, mis = R.psi_expectations(c["var_tran"], c["var_init"])
    e_lt, e_mi = R.err_in_bound(lt, ltr, lts, C.PSI_MULT), R.err_in_bound(mi, mir, mis, C.PSI_MULT)
    print("FIG seq globals K=%d: ltran %.3f, mod_init %.3f of bound" % (K, e_lt, e_mi))
    assert e_lt <= 1.0 and e_mi <= 1.0


# ---------------------------------------------------------------------------------------------------
#  3. three iterations against the host-stepped route on the same device
# ---------------------------------------------------------------------------------------------------
MAXC = 60
ITER_IDX = ([5, 0, 3, 3, 6], [1, 2, 4], [6, 6, 0, 2])


def _problem(fam, holes):
    K, D, T = 5, 3, int(sum(S.LENGTHS))
    rng = np.random.default_rng({"niw": 6, "mcat": 7, "poisson": 8}[fam])
    sts = np.repeat(rng.integers(0, K, size=T // 10 + 1), 10)[:T]
    if fam == "niw":
        means = 3.0 * rng.normal(size=(K, D))
        obs = means[sts] + rng.normal(size=(T, D))
        prior = (np.tile(obs.mean(0), (K, 1)), np.tile(0.75 * np.cov(obs.T), (K, 1, 1)), np.full(K, 0.01), np.full(K, D + 2.0))
        nu = D + 3.0 + 5.0 * rng.random(K)
        fac = (means + 0.3 * rng.normal(size=(K, D)), np.tile(np.eye(D), (K, 1, 1)) * (nu - D - 1.0)[:, None, None],
               1.0 + rng.random(K), nu)
    elif fam == "mcat":
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
        mask = rng.random(T) < 0.15
        if fam != "niw":                   # (a NaN entry of an unmasked Gaussian row has no statistics)
            obs[rng.permutation(T)[:T // 3], 1] = np.nan
            bad = rng.permutation(T)[:T // 10]
            obs[bad[::2], 0] = -1.0
            obs[bad[1::2], 0] = 1e6
    return dict(K=K, D=D, T=T, obs=obs, mask=mask, prior=prior, fac=fac, prior_tran=1.0 + rng.random((K, K)),
                var_tran=1.0 + 10.0 * rng.random((K, K)), prior_init=0.5 + rng.random(K), var_init=0.2 + 3.0 * rng.random(K))


def _loop(eng, fam, p, iters, maxit=3):
    """set_obs .. svi_sequences, then the iterations; -> (var_tran, var_init, factors, elbo)"""
    eng.set_obs(p["obs"], p["mask"])
    eng.set_sequences(np.asarray(S.LENGTHS))
    S.begin_family(eng, fam, p["prior_tran"], p["var_tran"], p["prior"], p["fac"], maxit, MAXC)
    eng.svi_sequences(p["prior_init"], p["var_init"])
    N = len(S.LENGTHS)
    for it, (idx, flags, rho) in enumerate(iters):
        eng.svi_iteration_sequences(it, idx, flags, rho, N / float(len(idx)))
    elbo = eng.svi_read_elbo(len(iters))[0]
    vt, vi, fac = S.read_state(eng, fam)
    return vt, vi, list(fac), elbo


@pytest.mark.parametrize("variant", ["plain", "holes"])
@pytest.mark.parametrize("fam", ["niw", "mcat", "poisson"])
def test_three_iterations_equal_the_host_stepped_route(fam, variant):
    """K = 5, D = 3 on the base layout, another idx per iteration.  The host-stepped route (SciPy psi -> set_globals ->
    set_emission_* -> estep_sequence_subset -> hmmbatchsgd._global_update_from_stats -> lower_bound) runs on the same
    device; the project's tolerances for this comparison: state rtol 1e-6 / atol 1e-9, ELBO rtol 1e-9.  `holes`:
    masked rows under SVIHMM_MASK_AS_NAN, for the table families a column NaN in a third of the rows and
    out-of-range entries."""
    p = _problem(fam, variant == "holes")
    flags = WRAP | (S.MASK_AS_NAN if variant == "holes" else 0)
    iters = [(np.array(ix), flags, (it + 1.0) ** -0.7) for it, ix in enumerate(ITER_IDX)]
    eng = _engine(centring_off=False)
    try:
        vt, vi, fac, elbo = _loop(eng, fam, p, iters)
        assert eng.svi_recoveries() == 0
    finally:
        eng.close()
    ref = _engine(centring_off=False)
    try:
        ref.set_obs(p["obs"], p["mask"])
        ref.set_sequences(np.asarray(S.LENGTHS))
        rvt, rvi, remit, relbo = S.host_stepped(ref, fam, S.LENGTHS, p["prior_init"], p["var_init"], p["prior_tran"],
                                                p["var_tran"], p["prior"], p["fac"], iters, MAXC)
    finally:
        ref.close()
    assert np.all(np.isfinite(elbo))
    np.testing.assert_allclose(vt, rvt, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(vi, rvi, rtol=1e-6, atol=1e-9)
    for x, y in zip(fac, S.emitter_factors(fam, remit)):
        np.testing.assert_allclose(x, y, rtol=1e-6, atol=1e-9)
    np.testing.assert_allclose(elbo, relbo, rtol=1e-9)


# ---------------------------------------------------------------------------------------------------
#  4. the class
# ---------------------------------------------------------------------------------------------------
CLASS_LENGTHS = (12, 30, 7, 1, 25, 18, 40, 9, 33, 2, 21, 16)


def _class_model(fam, K=4, D=3):
    from pysvihmm_amd import hmmbatchsgd
    from pysvihmm_amd.distributions import Gaussian, ProductCategorical, ProductPoisson
    T = int(sum(CLASS_LENGTHS))
    rng = np.random.default_rng({"niw": 31, "mcat": 32, "poisson": 33}[fam])
    sts = np.repeat(rng.integers(0, K, size=T // 8 + 1), 8)[:T]
    np.random.seed(4)
    if fam == "niw":
        obs = 3.0 * rng.normal(size=(K, D))[sts] + rng.normal(size=(T, D))
        emit = np.array([Gaussian(mu_0=obs.mean(0), sigma_0=0.75 * np.cov(obs.T), kappa_0=0.01, nu_0=D + 2) for _ in range(K)])
    elif fam == "mcat":
        th = [rng.dirichlet(np.ones(v) * 0.5, size=K) for v in (2, 3, 4)]
        obs = np.stack([[rng.choice(len(t[s]), p=t[s]) for s in sts] for t in th], axis=1).astype(np.float64)
        emit = np.array([ProductCategorical(alphav_0=[np.ones(v) * 1.5 for v in (2, 3, 4)]) for _ in range(K)])
    else:
        obs = rng.poisson(np.linspace(1.0, 20.0, K)[sts][:, None] * np.linspace(1.0, 2.0, D)[None, :]).astype(np.float64)
        emit = np.array([ProductPoisson(np.full(D, 2.0), np.full(D, 0.5), max_count=MAXC) for _ in range(K)])
    mask = rng.random(T) < 0.1
    off = S.offsets(CLASS_LENGTHS)
    seqs = [obs[off[s]:off[s + 1]].copy() for s in range(len(CLASS_LENGTHS))]
    masks = [mask[off[s]:off[s + 1]].copy() for s in range(len(CLASS_LENGTHS))]
    return hmmbatchsgd.VBHMM(seqs, np.ones(K), np.ones((K, K)), emit, mask=masks, maxit=6, seq_minibatch=3)


def _class_factors(fam, G):
    if fam == "niw":
        return [np.asarray(G.mu_mf), np.asarray(G.sigma_mf), np.asarray(G.kappa_mf, dtype=float), np.asarray(G.nu_mf, dtype=float)]
    return list(G.alpha_mf) if fam == "mcat" else [G.alpha_mf, G.beta_mf]


@pytest.mark.parametrize("fam", ["niw", "mcat", "poisson"])
def test_class_device_loop_equals_the_host_route(fam, monkeypatch):
    """hmmbatchsgd.VBHMM on 12 short sequences, K = 4, 6 iterations, M = 3: infer(device_loop=True) against
    infer(device_loop=False) from the same seed at test_gpu_svi_families._close's tolerances (state 1e-7 / 1e-9,
    ELBO 1e-8, var_x 1e-6 / 1e-11); both draw the same idx."""
    draws = []
    choice = np.random.choice

    def recording(*a, **kw):
        out = choice(*a, **kw)
        draws[-1].append(np.array(out))
        return out

    monkeypatch.setattr(np.random, "choice", recording)
    runs = []
    for dl in (True, False):
        m = _class_model(fam)
        assert m._svi_sequences_refusal() is None
        draws.append([])
        np.random.seed(99)
        m.infer(device_loop=dl)
        runs.append(m)
    a, b = runs
    assert a.engine.name == "hip" and a.engine.svi_recoveries() == 0
    assert len(draws[0]) == len(draws[1]) == 6
    for x, y in zip(*draws):
        np.testing.assert_array_equal(x, y)
    assert len({tuple(np.sort(d)) for d in draws[0]}) > 1
    assert len(a.elbo_vec) == 6 and np.all(np.isfinite(a.elbo_vec))
    assert np.all(np.isfinite(a.iter_time)) and np.all(a.iter_time > 0)
    rtol = 1e-7
    np.testing.assert_allclose(a.var_tran, b.var_tran, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(a.var_init, b.var_init, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(a.elbo_vec, b.elbo_vec, rtol=1e-8)
    for G, H_ in zip(a.var_emit, b.var_emit):
        for x, y in zip(_class_factors(fam, G), _class_factors(fam, H_)):
            np.testing.assert_allclose(x, y, rtol=rtol, atol=1e-9)
    np.testing.assert_allclose(a.var_x, b.var_x, rtol=rtol * 10, atol=1e-11)
    a.engine.close(); b.engine.close()


def test_class_refuses_device_loop_true_with_its_reason():
    m = _class_model("poisson")
    m.prior_tran = np.full((4, 4), 0.5)
    with pytest.raises(RuntimeError, match="device_loop=True.*prior_tran has entries below 1"):
        m.infer(device_loop=True)
    m = _class_model("poisson")
    m.var_init = np.array([1e-4, 1.0, 1.0, 1.0])
    with pytest.raises(RuntimeError, match="device_loop=True.*var_init has entries below"):
        m.infer(device_loop=True)
    # a piece of the host route wrapped on the instance, or an engine call it makes: the host route, which calls them
    m = _class_model("poisson")
    stats = m._seq_minibatch_stats
    m._seq_minibatch_stats = lambda: stats()
    assert m._svi_sequences_refusal() == "_seq_minibatch_stats is overridden"
    del m._seq_minibatch_stats
    assert m._svi_sequences_refusal() is None
    sub = m.engine.estep_sequence_subset
    calls = []
    m.engine.estep_sequence_subset = lambda *a, **k: calls.append(1) or sub(*a, **k)
    assert m._svi_sequences_refusal() == "the engine's estep_sequence_subset is replaced on the instance"
    np.random.seed(1)
    m.infer()
    assert len(calls) == 6 and len(m.elbo_vec) == 6
    m.engine.close()


# ---------------------------------------------------------------------------------------------------
#  5. reproducibility and hygiene
# ---------------------------------------------------------------------------------------------------
def _push_host_state(eng, fam, p):
    from scipy.special import digamma
    vi, vt = p["var_init"], p["var_tran"]
    eng.set_globals(digamma(vi + 1e-9) - digamma(vi.sum() + 1e-9), digamma(vt + 1e-9) - digamma(vt.sum(1)[:, None] + 1e-9))
    a, b = p["fac"]
    eng.set_emission_poisson(digamma(a) - np.log(b), a / b, MAXC)


def test_runs_are_reproducible_and_the_handle_stays_clean():
    """Two identical 3-iteration runs: array_equal state and ELBO.  After a loop estep_sequences() on the same handle
    returns the bits it returned before the loop (same uploaded globals and emission), estep_sequence_subset the bits
    of a fresh handle."""
    fam = "poisson"
    p = _problem(fam, True)
    flags = WRAP | S.MASK_AS_NAN
    iters = [(np.array(ix), flags, (it + 1.0) ** -0.7) for it, ix in enumerate(ITER_IDX)]
    out = []
    for _ in range(2):
        eng = _engine(centring_off=False)
        try:
            eng.set_obs(p["obs"], p["mask"])
            eng.set_sequences(np.asarray(S.LENGTHS))
            _push_host_state(eng, fam, p)
            before = eng.estep_sequences(flags=flags)
            res = _loop(eng, fam, p, iters)
            assert eng.svi_recoveries() == 0
            _push_host_state(eng, fam, p)
            after = eng.estep_sequences(flags=flags)
            sub = eng.estep_sequence_subset(ITER_IDX[0], flags=flags)
            sub_x = eng.read_rows("var_x", 0, int(sum(S.LENGTHS[s] for s in ITER_IDX[0])))
            out.append((res, before, after, sub, sub_x))
        finally:
            eng.close()
    (ra, ba, aa, sa, xa), (rb, _, _, _, _) = out
    for x, y in zip(ra[:2] + tuple(ra[2]) + (ra[3],), rb[:2] + tuple(rb[2]) + (rb[3],)):
        np.testing.assert_array_equal(x, y)
    np.testing.assert_array_equal(ba[0].buf, aa[0].buf)
    np.testing.assert_array_equal(ba[1], aa[1])
    np.testing.assert_array_equal(ba[2], aa[2])
    fresh = _engine(centring_off=False)
    try:
        fresh.set_obs(p["obs"], p["mask"])
        fresh.set_sequences(np.asarray(S.LENGTHS))
        _push_host_state(fresh, fam, p)
        fs = fresh.estep_sequence_subset(ITER_IDX[0], flags=flags)
        fx = fresh.read_rows("var_x", 0, xa.shape[0])
    finally:
        fresh.close()
    np.testing.assert_array_equal(sa[0].buf, fs[0].buf)
    np.testing.assert_array_equal(sa[1], fs[1])
    np.testing.assert_array_equal(sa[2], fs[2])
    np.testing.assert_array_equal(xa, fx)


# ---------------------------------------------------------------------------------------------------
#  6. refusals
# ---------------------------------------------------------------------------------------------------
def _raw_iteration(eng, it, idx, M, flags, rho, bf):
    from pysvihmm_amd import _lib as L
    ptr = None if idx is None else np.ascontiguousarray(idx, dtype=np.int32).ctypes.data_as(ctypes.POINTER(ctypes.c_int32))
    rc = eng._lib.svihmm_svi_iteration_sequences(eng._h, it, ptr, M, flags, rho, bf)
    return rc, L.last_error()


def test_refusals_leave_the_handle_usable():
    from pysvihmm_amd import _lib as L
    c = S.seq_case("poisson", 4, 2, S.LENGTHS, S.IDX, rho=0.37)
    K, idx, bf = c["K"], c["idx"], c["bf"]
    pi, vi = c["prior_init"], c["var_init"]
    eng = _engine()
    try:
        # ---- svihmm_svi_sequences
        eng.set_obs(c["obs"], None)
        with pytest.raises(RuntimeError, match="svihmm_svi_sequences: no loop"):
            eng.svi_sequences(pi, vi)
        S.begin_family(eng, "poisson", c["prior_tran"], c["var_tran"], c["prior"], c["factors"], 8)
        with pytest.raises(RuntimeError, match="svihmm_svi_sequences: no sequences declared"):
            eng.svi_sequences(pi, vi)
        eng.set_sequences(np.asarray(S.LENGTHS))
        with pytest.raises(RuntimeError, match="svihmm_svi_iteration_sequences: .*call svihmm_svi_sequences first"):
            eng.svi_iteration_sequences(0, idx, WRAP, 0.5, bf)
        for a, b, msg in ((None, vi, "prior_init is NULL"), (pi, None, "var_init is NULL")):
            rc = eng._lib.svihmm_svi_sequences(eng._h, L.dptr(a), L.dptr(b))
            assert rc != 0 and msg in L.last_error(), L.last_error()
        for bad, name in ((np.nan, "prior_init"), (np.inf, "prior_init"), (1e-3, "prior_init"),
                          (np.nan, "var_init"), (np.inf, "var_init"), (1e-3, "var_init")):
            x = (pi if name == "prior_init" else vi).copy()
            x[2] = bad
            with pytest.raises(RuntimeError, match=r"svihmm_svi_sequences: %s\[2\]" % name):
                eng.svi_sequences(x if name == "prior_init" else pi, x if name == "var_init" else vi)
        eng.svi_set_adagrad(np.ones((K, K)))
        with pytest.raises(RuntimeError, match="svihmm_svi_sequences: an AdaGrad accumulator is set"):
            eng.svi_sequences(pi, vi)
        eng.svi_set_adagrad(None)
        # (the window loop is still what runs: nothing above touched its state)
        eng.svi_iteration(0, np.array([3, 12]), 2, 5, WRAP, 0.5, 3.0, 3.0)
        assert np.isfinite(eng.svi_read_elbo(1)[0][0])
        np.testing.assert_array_equal(eng.svi_read_factors()[1] > 0, True)
        # ---- after the switch
        eng.svi_sequences(pi, vi)
        with pytest.raises(RuntimeError, match="svihmm_svi_iteration: .*svihmm_svi_iteration_sequences"):
            eng.svi_iteration(1, np.array([3, 12]), 2, 5, WRAP, 0.5, 3.0, 3.0)
        with pytest.raises(RuntimeError, match="svihmm_svi_set_adagrad: .*sequences"):
            eng.svi_set_adagrad(np.ones((K, K)))
        eng.svi_set_adagrad(None)
        # ---- svihmm_svi_iteration_sequences, each before any device work
        state = S.read_state(eng, "poisson")
        bad_calls = [
            ((-1, idx, len(idx), WRAP, 0.5, bf), "it = -1 is outside"),
            ((8, idx, len(idx), WRAP, 0.5, bf), "it = 8 is outside"),
            ((1, None, 5, WRAP, 0.5, bf), "idx is NULL"),
            ((1, idx, 0, WRAP, 0.5, bf), "M = 0"),
            ((1, [5, 0, 7, 3], 4, WRAP, 0.5, bf), "idx[2] = 7 is outside [0, N = 7)"),
            ((1, [5, -1], 2, WRAP, 0.5, bf), "idx[1] = -1 is outside"),
            ((1, idx, len(idx), WRAP | L.USE_HOST_LLIKS, 0.5, bf), "SVIHMM_USE_HOST_LLIKS"),
            ((1, idx, len(idx), WRAP | L.SVI_KEEP_WINDOW, 0.5, bf), "SVIHMM_SVI_KEEP_WINDOW"),
            ((1, idx, len(idx), WRAP, np.nan, bf), "rho is not finite"),
            ((1, idx, len(idx), WRAP, 0.5, np.inf), "bfact is not finite"),
        ]
        for args, msg in bad_calls:
            rc, err = _raw_iteration(eng, *args)
            assert rc != 0 and err.startswith("svihmm_svi_iteration_sequences: ") and msg in err, (args, err)
            for x, y in zip((state[0], state[1]) + tuple(state[2]), (lambda s: (s[0], s[1]) + tuple(s[2]))(S.read_state(eng, "poisson"))):
                np.testing.assert_array_equal(x, y)
        # a valid iteration afterwards succeeds
        eng.svi_iteration_sequences(1, idx, WRAP, 0.5, bf)
        assert np.isfinite(eng.svi_read_elbo(2)[0][1])
        vt, vi1, fac = S.read_state(eng, "poisson")
        assert np.all(np.isfinite(vt)) and np.all(vi1 > 0) and all(np.all(x > 0) for x in fac)
        assert np.any(vt != state[0])
        # the declaration gone: the iteration says so; the next begin starts a window loop again
        eng.set_sequences(None)
        rc, err = _raw_iteration(eng, 2, idx, len(idx), WRAP, 0.5, bf)
        assert rc != 0 and "no sequences declared" in err
        S.begin_family(eng, "poisson", c["prior_tran"], c["var_tran"], c["prior"], c["factors"], 8)
        eng.svi_iteration(0, np.array([3, 12]), 2, 5, WRAP, 0.5, 3.0, 3.0)
        assert np.isfinite(eng.svi_read_elbo(1)[0][0])
        assert eng.svi_recoveries() == 0
    finally:
        eng.close()


def test_row_offsets_beyond_the_statistics_gemm_are_refused():
    """R beyond the statistics GEMM's 32-bit row offsets: duplicates of one long sequence (host check only)."""
    K, n = 4, 40000
    rng = np.random.default_rng(3)
    obs = rng.poisson(3.0, size=(n + 5, 1)).astype(np.float64)
    eng = _engine()
    try:
        eng.set_obs(obs, None)
        eng.set_sequences(np.array([n, 5]))
        a = 1.0 + rng.random((K, 1))
        S.begin_family(eng, "poisson", np.ones((K, K)), np.ones((K, K)), (a, a), (a, a), 2, 30)
        eng.svi_sequences(np.ones(K), np.ones(K))
        M = (1 << 31) // n + 2
        rc, err = _raw_iteration(eng, 0, np.zeros(M, dtype=np.int32), M, WRAP, 0.5, 2.0)
        assert rc != 0 and "too many for the statistics GEMM" in err, err
        eng.svi_iteration_sequences(0, [1], WRAP, 0.5, 2.0)
        assert np.isfinite(eng.svi_read_elbo(1)[0][0])
    finally:
        eng.close()
