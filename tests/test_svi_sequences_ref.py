"""CPU: the referee of the resident SVI loop's sequence step and bound (tests/svi_sequences_helpers.py) against float64
restatements of the device's expressions, and ``hmmbatchsgd.VBHMM.infer(device_loop=...)`` on an engine without the
loop (the oracle engine has no ``svi_iteration_sequences``: the host route, unchanged)."""
import numpy as np
import pytest

from oracle.engine import OracleEngine
from pysvihmm_amd import hmmbatchsgd
from sequences_helpers import build_model, class_data
from tests import svi_cases as C
from tests import svi_referee as R
from tests import svi_sequences_helpers as S

needs_ld = pytest.mark.skipif(not R.have_extended_precision(), reason="np.longdouble is not wider than double on this host")
_CASES = [pytest.param(c, rho, id="%s-rho%g" % (S.case_id(c), rho)) for c in S.SEQ_CASES for rho in S.RHOS]


@needs_ld
@pytest.mark.parametrize("case,rho", _CASES)
def test_float64_restatements_pass_the_gpu_bounds(case, rho):
    """The device's sequence step (svi_tran_step's sequence branch, svi_dirichlet_seq_step, the families' blends with
    bE = bf) and its ELBO assembly with the initial factor's row, restated in float64 NumPy on synthetic statistics of
    the listed sequences: inside STEP_MULT eps scale and ELBO_MULT eps sum|terms| of the referee -- the bounds of
    tests/test_gpu_svi_sequences.py."""
    c = S.seq_case(*case, rho=rho)
    fam = c["fam"]
    packed, q0 = S.synthetic_packed(c)
    pre, prior = S.state_of(c, c["var_tran"], c["factors"]), S.prior_of(c)
    ref = S.global_step(fam, pre, prior, packed, q0, c["var_init"], c["prior_init"], rho, c["bf"])
    got = S.global_step_f64(fam, pre, prior, packed, q0, c["var_init"], c["prior_init"], rho, c["bf"])
    assert set(got) == set(ref)
    errs = R.step_errors(got, ref, C.STEP_MULT)
    assert max(errs.values()) <= 1.0, errs
    # the bound of the stepped state
    post_fac = [got[n] for n in ("mu", "sigma", "kappa", "nu")] if fam == "niw" else \
        [got[n] for n in ("mu", "nus", "alphas", "betas")] if fam == "diag" else \
        got["alpha"] if fam == "cat" else \
        np.split(got["alpha"], np.cumsum(c["shape"])[:-1], axis=1) if fam == "mcat" else [got["a"], got["b"]]
    post = S.state_of(c, got["var_tran"], post_fac)
    glb = S.global_lower_bound(fam, post, prior, got["var_init"], c["prior_init"])
    e = S.elbo_error(S.elbo_f64(fam, post, prior, got["var_init"], c["prior_init"], c["bf"], packed.lb[0]),
                     c["bf"], packed.lb[0], glb)
    assert e <= 1.0, e


def test_the_sequence_rule_is_not_the_window_rule_with_a_reciprocal_window_count():
    """nwin = 1 / bf in the window expression gives the same real number and other roundings: the rule is its own
    branch.  (Equal to 4 eps here, different in the last bit somewhere.)"""
    c = S.seq_case("cat", 5, 70, S.LENGTHS, S.IDX, rho=0.37)
    packed, _ = S.synthetic_packed(c)
    bf, rho = c["bf"], 0.37
    seq = ((1.0 - rho) * (c["var_tran"] - 1.0) + rho * ((c["prior_tran"] - 1.0) + bf * packed.A_raw)) + 1.0
    win, _ = R.tran_step_f64(c["var_tran"], c["prior_tran"], packed.A_raw, 1.0 / bf, rho, bf)
    np.testing.assert_allclose(seq, win, rtol=4 * R.F64_EPS)
    assert np.any(seq != win)


def test_initial_factor_term_of_the_bound_is_hmmbases():
    """referee bound = window referee bound + dirichlet_elbo(prior_init, var_init), hmmbase.lower_bound's pi_term"""
    from pysvihmm_amd.hmmbase import dirichlet_elbo
    c = S.seq_case("poisson", 4, 2, (2100, 40, 9), (0, 2), rho=1.0)
    st, pr = S.state_of(c, c["var_tran"], c["factors"]), S.prior_of(c)
    with_init = S.global_lower_bound("poisson", st, pr, c["var_init"], c["prior_init"])
    without = S.H.global_lower_bound_poisson(st, pr)
    want = dirichlet_elbo(c["prior_init"][None, :], c["var_init"][None, :])
    assert float(with_init[0] - without[0]) == pytest.approx(want, rel=1e-12)
    assert with_init[1] > without[1]


# ---------------------------------------------------------------------------------------------------
#  the class on an engine without the loop
# ---------------------------------------------------------------------------------------------------
LENGTHS = (40, 1, 300, 17)
SEED = 12345


def _factors(emit):
    return [np.array([np.asarray(getattr(g, n), dtype=float) for g in emit])
            for n in ("mu_mf", "sigma_mf", "kappa_mf", "nu_mf")]


def _run(**kw):
    seqs, masks = class_data(LENGTHS)
    hmm = build_model(hmmbatchsgd, seqs, masks, OracleEngine(), maxit=3, seq_minibatch=2)
    np.random.seed(SEED)
    hmm.infer(**kw)
    return hmm


def test_class_without_the_loop_keeps_the_host_route():
    """infer() and infer(device_loop=False) on the oracle engine: the host route, bit for bit"""
    a, b = _run(), _run(device_loop=False)
    assert len(a.elbo_vec) == 3 and np.all(np.isfinite(a.elbo_vec))
    for n in ("var_tran", "var_init", "elbo_vec", "var_x"):
        assert np.array_equal(getattr(a, n), getattr(b, n)), n
    for x, y in zip(_factors(a.var_emit), _factors(b.var_emit)):
        assert np.array_equal(x, y)
    assert a._svi_sequences_refusal() == "the engine has no svi_sequences / svi_iteration_sequences"


def test_class_device_loop_true_raises_where_the_loop_cannot_run():
    with pytest.raises(RuntimeError, match="device_loop=True.*engine has no svi_sequences"):
        _run(device_loop=True)
    seqs, masks = class_data(LENGTHS)
    hmm = build_model(hmmbatchsgd, seqs, masks, OracleEngine(), maxit=2)        # no seq_minibatch
    with pytest.raises(RuntimeError, match="device_loop=True.*seq_minibatch is not set"):
        hmm.infer(device_loop=True)


def test_lifted_helpers_live_on_the_base_class():
    """_svi_family, the begin dispatch and _svi_pull_state are hmmbase's: one copy for both SVI classes"""
    from pysvihmm_amd import hmmsgd_metaobs
    from pysvihmm_amd.hmmbase import VariationalHMMBase
    for name in ("_svi_family", "_svi_begin", "_svi_pull_state", "_svi_plain_vlb"):
        assert getattr(hmmsgd_metaobs.VBHMM, name) is getattr(VariationalHMMBase, name), name
        assert getattr(hmmbatchsgd.VBHMM, name) is getattr(VariationalHMMBase, name), name
