"""One handle walked through every ordered pair (A, B) of the six emission families: a handle that has been under
family A behaves under family B as B's own tests say it should.

Per pair: one E-step under A, then B is set and one E-step runs; both are compared with the family's referee at the
tolerance of the family's own E-step test (nothing new is introduced here):

  niw      ref_c.estep_minibatch, whole buffer rtol 1e-6 / atol 1e-8          (tests/test_gpu_parity.py)
  diag     OracleEngine.estep, ``_close`` of tests/test_gpu_diag.py with xs = 1
  cat      OracleEngine.estep, A_raw / counts rtol 1e-6 with atol 1e-9 x rows, lb rtol 1e-10   (tests/test_categorical.py)
  mcat, poisson, pgauss
           the helper module's NumPy lliks through the oracle's recursions and its statistics of those posteriors,
           ``check_stats`` of tests/test_gpu_mcat.py / test_gpu_poisson.py / test_gpu_pgauss.py

Shapes: K = 3, two columns (one under the Categorical family), two windows of 48 rows.  One data set serves every
family: entries 0..3 are reals, symbols of a 4-symbol column and counts alike.  The observations are uploaded again
only when the column count changes (into and out of the Categorical family), always under the family that is being
left: an upload under a table family is left uncentred for the Gaussian family that follows, an upload under a Gaussian
family is centred and the table family that follows takes the centre out again.  T = 128 rows makes every column mean
a dyadic rational, so centring and un-centring small integers is exact and the walk does not depend on its order."""
import itertools
import re

import numpy as np
import pytest

from oracle import ref_c
from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib as L
from tests import mcat_helpers as MH
from tests import pgauss_helpers as GH
from tests import poisson_helpers as PH
from tests.helpers import make_problem
from tests.test_gpu_diag import _close as close_diag
from tests.test_gpu_mcat import check_stats as check_mcat
from tests.test_gpu_pgauss import check_stats as check_pgauss
from tests.test_gpu_poisson import check_stats as check_poisson

pytestmark = pytest.mark.gpu

FAMILIES = ("niw", "diag", "cat", "mcat", "poisson", "pgauss")
K, D, T, LM = 3, 2, 128, 48
STARTS = np.array([5, 70], dtype=np.int64)
ROWS = len(STARTS) * LM
FLAGS = L.TRANS_WRAP
VS, C = (4, 4), 15


def _problem():
    rng = np.random.default_rng(2024)
    p = make_problem(K, D, T, seed=11)
    p["x"] = rng.integers(0, 4, size=(T, D)).astype(np.float64)
    p["mask"] = rng.random(T) < 0.1
    p["mu"] = 1.5 + rng.normal(size=(K, D))
    p["diag"] = (p["mu"], 0.5 + 4 * rng.random((K, D)), 2.0 + 5 * rng.random((K, D)), 1.0 + 6 * rng.random((K, D)))
    p["logp"] = MH.make_model(K, VS, rng)[0]
    pois = PH.make_model(K, D, rng, base=np.array([1.5, 1.5]))
    p["elog"], p["erate"] = pois["elog"], pois["erate"]
    al = rng.uniform(2.0, 20.0, size=(K, D))
    p["pg"] = GH.tables(p["mu"], rng.uniform(1.0, 50.0, size=(K, D)), al, al * rng.uniform(0.5, 2.0, size=(K, D)))
    p["origin"] = GH.data_origin(p["x"])
    return p


P = _problem()
_ref = {}


def _table_referee(ll, stats):
    """The NumPy lliks of the windows through the oracle's recursions, the helper's statistics of its posteriors."""
    o = OracleEngine()
    o.set_globals(P["mod_init"], P["ltran"])
    o.set_lliks(ll.reshape(len(STARTS), LM, K))
    res = o.forward_backward(None, LM, flags=FLAGS | L.USE_HOST_LLIKS, want=("var_x", "local_lb"), B=len(STARTS))
    q = res["var_x"]
    return sum(R.transition_stat_wrap(q[b]) for b in range(len(STARTS))), stats(q.reshape(ROWS, K)), float(res["local_lb"].sum())


def referee(name):
    """Computed once per family and left unchanged."""
    if name in _ref:
        return _ref[name]
    x, mask = P["x"], P["mask"]
    rows = MH.window_rows(STARTS, LM)
    xr, mr = x[rows], mask[rows]
    if name == "niw":
        r = ref_c.estep_minibatch(x, mask, STARTS, LM, P["mod_init"], P["ltran"], P["mu"], P["sigma"], P["kappa"],
                                  P["nu"], flags=FLAGS)
    elif name in ("diag", "cat"):
        o = OracleEngine()
        o.set_obs(x if name == "diag" else x[:, :1], mask)
        o.set_globals(P["mod_init"], P["ltran"])
        if name == "diag":
            o.set_emission_diag(*P["diag"])
        else:
            o.set_emission_cat(np.ascontiguousarray(P["logp"][:, :VS[0]]))
        r = o.estep(STARTS, LM, flags=FLAGS)
    elif name == "mcat":
        r = _table_referee(MH.mcat_lliks(xr, mr, VS, P["logp"], FLAGS), lambda q: MH.mcat_counts(xr, mr, VS, q))
    elif name == "poisson":
        r = _table_referee(PH.poisson_lliks(xr, mr, P["elog"], P["erate"], PH.logfact_table(C), FLAGS),
                           lambda q: PH.poisson_stats(xr, mr, C, q))
    else:
        r = _table_referee(GH.pgauss_lliks(xr, mr, *P["pg"], flags=FLAGS),
                           lambda q: GH.pgauss_stats(xr, mr, P["origin"], q))
    _ref[name] = r
    return r


def enter(e, name):
    """Bring the handle under ``name``: the rows first when their column count changes, then the family."""
    cols = 1 if name == "cat" else D
    if (e.T, e.D) != (T, cols):
        e.set_obs(P["x"][:, :cols], P["mask"])
    if name == "niw":
        e.set_emission_niw(P["mu"], P["sigma"], P["kappa"], P["nu"])
    elif name == "diag":
        e.set_emission_diag(*P["diag"])
    elif name == "cat":
        e.set_emission_cat(np.ascontiguousarray(P["logp"][:, :VS[0]]))
    elif name == "mcat":
        e.set_emission_mcat(MH.split_tables(P["logp"], VS))
    elif name == "poisson":
        e.set_emission_poisson(P["elog"], P["erate"], C)
    else:
        e.set_emission_pgauss(*P["pg"], origin=P["origin"])


def estep_and_check(e, name):
    from pysvihmm_amd import engine as E
    st = e.estep(STARTS, LM, flags=FLAGS)
    want = referee(name)
    cls, size = {"niw": (E.PackedStats, K * K + K * D + K + K * D * D + 1),
                 "diag": (E.PackedDiagStats, K * K + 2 * K * D + K + 1),
                 "cat": (E.PackedCatStats, K * K + K * VS[0] + 1),
                 "mcat": (E.PackedMCatStats, K * K + K * sum(VS) + 1),
                 "poisson": (E.PackedPoissonStats, K * K + 2 * K * D + 1),
                 "pgauss": (E.PackedGaussTrackStats, K * K + 3 * K * D + 1)}[name]
    assert type(st) is cls and st.buf.size == size == int(e._lib.svihmm_packed_len(e._h))
    # the Gaussian families keep the resident rows centred, the table families as uploaded
    assert np.any(e.get_shift() != 0.0) == (name in ("niw", "diag"))
    if name == "niw":
        np.testing.assert_allclose(st.buf, want, rtol=1e-6, atol=1e-8)
    elif name == "diag":
        close_diag(st, want, K, D, ROWS, 1.0)
    elif name == "cat":
        np.testing.assert_allclose(st.A_raw, want.A_raw, rtol=1e-6, atol=1e-9 * ROWS)
        np.testing.assert_allclose(st.counts, want.counts, rtol=1e-6, atol=1e-9 * ROWS)
        np.testing.assert_allclose(st.lb[0], want.lb[0], rtol=1e-10)
    elif name == "mcat":
        check_mcat(st, *want, scale=ROWS)
    elif name == "poisson":
        check_poisson(st, *want, scale=ROWS, cmax=3.0)
    else:
        check_pgauss(st, *want, scale=ROWS, rmax=GH.residual_scale(P["x"], P["mask"], P["origin"]))
        assert np.array_equal(st.origin, P["origin"])


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    e.set_globals(P["mod_init"], P["ltran"])
    yield e
    e.close()


@pytest.mark.parametrize("a,b", list(itertools.permutations(FAMILIES, 2)), ids=lambda n: n)
def test_family_b_after_family_a(eng, a, b):
    enter(eng, a)
    estep_and_check(eng, a)
    enter(eng, b)
    estep_and_check(eng, b)


PRED_REFUSALS = {
    "mcat": "svihmm_pred_logprob: NIW emission only (the multi-column Categorical family of svihmm_set_emission_mcat is not taken)",
    "poisson": "svihmm_pred_logprob: NIW emission only (the Poisson family of svihmm_set_emission_poisson is not taken)",
    "pgauss": "svihmm_pred_logprob: NIW emission only (the family of svihmm_set_emission_pgauss is not taken)",
}


@pytest.mark.parametrize("before", ["niw", "cat"])
@pytest.mark.parametrize("name", sorted(PRED_REFUSALS))
def test_pred_logprob_refuses_after_a_switch(eng, name, before):
    enter(eng, before)
    enter(eng, name)
    with pytest.raises(RuntimeError, match=re.escape(PRED_REFUSALS[name]) + "$"):
        eng.pred_logprob(STARTS, LM)
    estep_and_check(eng, name)           # the refusal left the family in force


ENTRY_REFUSAL = ("svihmm_heldout_entries: entry-wise scores are defined for the families that skip single entries: "
                 "besides the Gaussian tracks of svihmm_set_emission_pgauss, the multi-column Categorical and the "
                 "Poisson family only (svihmm_set_emission_mcat / svihmm_set_emission_poisson); svihmm_heldout_rows "
                 "takes every family")


@pytest.mark.parametrize("name", FAMILIES)
def test_heldout_entries_takes_the_entrywise_families_only(eng, name):
    enter(eng, "mcat" if name != "mcat" else "poisson")      # an entry-wise family first
    enter(eng, name)
    estep_and_check(eng, name)
    if name in ("mcat", "poisson", "pgauss"):
        assert eng.heldout_entries([3], [1], [2.0], resident=False)[1] == 1
    else:
        with pytest.raises(RuntimeError, match=re.escape(ENTRY_REFUSAL) + "$"):
            eng.heldout_entries([3], [0], [2.0], resident=False)
