"""Held-out scores, host side: the NumPy statements the GPU tests compare against (tests/heldout_helpers.py) are
themselves checked against SciPy on point parameters, ``util.speckle_holdout`` keeps its invariants, the classes'
argument errors are raised before any engine is touched, and the shared cases are not vacuous (most entries count,
the referee's posteriors are soft)."""
import numpy as np
import pytest

from pysvihmm_amd import hmmbatchcd
from pysvihmm_amd.util import speckle_holdout
from pysvihmm_amd.distributions import ProductCategorical, ProductPoisson
from tests import heldout_helpers as H
from tests import poisson_helpers as PH


def test_poisson_entry_formula_is_the_logpmf_mixture():
    from scipy.stats import poisson
    rng = np.random.default_rng(0)
    K, D, C = 4, 3, 40
    lam = rng.uniform(0.5, 12.0, size=(K, D))
    p = dict(fam="poisson", K=K, D=D, C=C, elog=np.log(lam), erate=lam, logfact=PH.logfact_table(C))
    q = rng.dirichlet(np.ones(K), size=6)
    rows = np.array([0, 5, 2, 2, 3, 1, 4])
    cols = np.array([0, 2, 1, 1, 0, 2, 1])
    vals = np.array([3.0, 0.0, 17.0, 17.0, float(C), np.nan, float(C + 1)])
    lp, M = H.heldout_entries_numpy(p, q, rows, cols, vals)
    assert np.isnan(lp[5]) and np.isnan(lp[6]) and np.all(np.isfinite(lp[:5]))
    want = [np.log(np.sum((q[r] + 1e-9) * poisson.pmf(int(v), lam[:, c]))) for r, c, v in zip(rows[:5], cols[:5], vals[:5])]
    np.testing.assert_allclose(lp[:5], want, rtol=1e-12)
    assert lp[2] == lp[3] and H.mean_count(lp)[1] == 5
    assert np.all(M[:5] >= np.abs(np.log(q[rows[:5]] + 1e-9)).max(1))


def test_mcat_entry_formula_is_the_table_mixture():
    rng = np.random.default_rng(1)
    K, V = 5, [1, 2, 7]
    theta = [rng.dirichlet(np.ones(v), size=K) for v in V]
    p = dict(fam="mcat", K=K, D=3, V=V, logp=np.log(np.concatenate(theta, axis=1)))
    q = rng.dirichlet(np.ones(K), size=4)
    rows = np.array([0, 1, 2, 3, 3, 0, 1])
    cols = np.array([2, 1, 0, 2, 2, 1, 0])
    vals = np.array([6.0, 1.0, 0.0, 3.9, np.nan, 2.0, -1.0])          # 3.9 is symbol 3; NaN, V[d] and -1 are absent
    lp, _ = H.heldout_entries_numpy(p, q, rows, cols, vals)
    assert np.isnan(lp[4]) and np.isnan(lp[5]) and np.isnan(lp[6])
    want = [np.log(np.sum((q[r] + 1e-9) * theta[c][:, int(v)])) for r, c, v in zip(rows[:4], cols[:4], vals[:4])]
    np.testing.assert_allclose(lp[:4], want, rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(lp[2], np.log(1.0 + K * 1e-9), atol=1e-15)   # a one-symbol column tells nothing


def test_rows_formula_and_kernel_order_mean():
    rng = np.random.default_rng(2)
    q = rng.dirichlet(np.ones(3), size=5000)
    ll = rng.normal(size=(5000, 3)) * 5
    masked = rng.random(5000) < 0.3
    lp = H.heldout_rows_numpy(q, ll, masked)
    assert np.array_equal(np.isnan(lp), ~masked)
    want = np.logaddexp.reduce(np.log(q[masked] + 1e-9) + ll[masked], axis=1)
    np.testing.assert_allclose(lp[masked], want, rtol=1e-13)
    m, n = H.kernel_order_mean(lp)
    assert n == masked.sum()
    np.testing.assert_allclose(m, want.mean(), rtol=1e-13)
    assert H.kernel_order_mean(np.full(7, np.nan)) == (None, 0)


def test_speckle_holdout_invariants():
    rng = np.random.default_rng(3)
    x = rng.poisson(4.0, size=(60, 5)).astype(float)
    x[rng.random(x.shape) < 0.1] = np.nan
    orig = x.copy()
    xb, r, c, v = speckle_holdout(x, 0.2, seed=11)
    assert np.array_equal(x, orig, equal_nan=True) and xb is not x
    n_ok = int((~np.isnan(orig)).sum())
    assert len(r) == len(c) == len(v) == int(round(0.2 * n_ok)) and r.dtype == np.int64
    assert len(set(zip(r.tolist(), c.tolist()))) == len(r)             # without replacement
    assert not np.isnan(v).any() and np.array_equal(v, orig[r, c])
    newly = np.isnan(xb) & ~np.isnan(orig)
    want = np.zeros_like(newly)
    want[r, c] = True
    assert np.array_equal(newly, want)                                 # NaN exactly at the triples
    assert np.array_equal(xb[~newly], orig[~newly], equal_nan=True)
    again = speckle_holdout(x, 0.2, seed=11)
    assert np.array_equal(again[0], xb, equal_nan=True) and all(np.array_equal(a, b) for a, b in zip(again[1:], (r, c, v)))
    assert not np.array_equal(speckle_holdout(x, 0.2, seed=12)[1], r)
    # chosen columns only
    _, r2, c2, _ = speckle_holdout(x, 0.5, seed=5, cols=[1, 4])
    assert set(c2.tolist()) <= {1, 4} and len(r2) == int(round(0.5 * (~np.isnan(orig[:, [1, 4]])).sum()))
    # a list is numbered over the concatenation and comes back as a list of the same lengths
    parts = [x[:7], x[7:8], x[8:]]
    lb, rl, cl, vl = speckle_holdout(parts, 0.2, seed=11)
    assert [len(a) for a in lb] == [7, 1, 52]
    assert np.array_equal(np.concatenate(lb), xb, equal_nan=True)
    assert np.array_equal(rl, r) and np.array_equal(cl, c) and np.array_equal(vl, v)
    assert all(np.array_equal(a, b, equal_nan=True) for a, b in zip(parts, [orig[:7], orig[7:8], orig[8:]]))
    assert len(speckle_holdout(x, 0.0, seed=1)[1]) == 0


class _Plug(object):
    """An emitter the device has no family for."""

    def expected_log_likelihood(self, x):
        return np.zeros(len(x))


def _model(emit, x, mask=None):
    K = len(emit)
    m = hmmbatchcd.VBHMM(x, np.ones(K), np.ones((K, K)), np.array(emit), mask=mask, maxit=1)
    assert m._engine is None
    return m


def test_class_errors_are_raised_without_an_engine():
    rng = np.random.default_rng(4)
    x = rng.poisson(3.0, size=(30, 2)).astype(float)
    xb, r, c, v = speckle_holdout(x, 0.2, seed=0)
    plug = _model([_Plug() for _ in range(3)], x, mask=np.arange(30) < 4)
    with pytest.raises(NotImplementedError, match="no device family"):
        plug.heldout_logprob()
    with pytest.raises(NotImplementedError, match="ProductCategorical or ProductPoisson"):
        plug.heldout_entries_logprob(r, c, v)
    pois = [ProductPoisson(np.ones(2), np.ones(2), max_count=50) for _ in range(3)]
    m = _model(pois, x)                       # the data were NOT blanked
    with pytest.raises(ValueError, match="not blanked"):
        m.heldout_entries_logprob(r, c, v)
    m = _model(pois, xb)
    with pytest.raises(ValueError, match="outside obs"):
        m.heldout_entries_logprob([30], [0], [1.0])
    with pytest.raises(ValueError, match="one length"):
        m.heldout_entries_logprob(r, c[:-1], v)
    bad = xb.copy()
    bad[r[3], c[3]] = 2.0                     # one entry of the list still holds a value
    with pytest.raises(ValueError, match=r"obs\[%d, %d\]" % (r[3], c[3])):
        _model(pois, bad).heldout_entries_logprob(r, c, v)
    assert m.heldout_logprob() is None        # no masked rows: nothing to score, no engine either
    mc = [ProductCategorical(alphav_0=[np.ones(2), np.ones(5)]) for _ in range(3)]
    assert _model(mc, x)._heldout_family() == "mcat" and m._heldout_family() == "poisson"
    for mod in (plug, m):
        assert mod._engine is None


CASES = ([("poisson", i) for i in range(len(PH.SHAPES))] + [("mcat", i) for i in range(len(H.MCAT_K))])
CASE_IDS = ["pois-" + s for s in PH.IDS] + ["mcat-" + s for s in H.MCAT_IDS]


@pytest.mark.parametrize("fam,i", CASES, ids=CASE_IDS)
def test_shared_cases_are_not_vacuous(fam, i):
    """Of every case's entry list at least 0.9 count (the deliberately absent ones are few), every kind the families
    define is in it, and on the referee's posteriors at least a tenth of the scored rows -- the entries' rows and the
    masked rows -- have max_k q < 0.99: the comparison is not one between one-hot rows."""
    for kind in ("chain", "windows"):
        cs = H.e2e_case(fam, i, kind)
        p, rows, cols, vals = cs["p"], cs["rows"], cs["cols"], cs["vals"]
        _, ok = H.entry_present(p, cols, vals)
        assert ok.mean() >= 0.9 and (~ok).sum() == len(H.absent_values(p, 0))
        assert rows.max() == len(cs["res"]) - 1 and (cols == p["D"] - 1).any()
        assert np.isnan(cs["xb"][cs["res"][rows[:cs["ns"]]], cols[:cs["ns"]]]).all()
        top = np.array([H.top_value(p, d) for d in cols])
        assert (ok & (vals == top)).any()
        pairs = list(zip(rows.tolist(), cols.tolist()))
        assert pairs[cs["ns"]] == pairs[0] and pairs[cs["ns"] + 1] == pairs[cs["ns"] // 2]      # the two duplicates
        q = cs["q"]
        assert np.mean(q[rows[ok]].max(1) < 0.99) >= 0.1
        assert cs["masked"].sum() >= 3 and np.mean(q[cs["masked"]].max(1) < 0.99) >= 0.1
        lp, _ = H.heldout_entries_numpy(p, q, rows, cols, vals)
        assert np.array_equal(np.isnan(lp), ~ok) and np.all(np.isfinite(lp[ok]))
