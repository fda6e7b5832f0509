"""Posterior expectations of per-state tables, the parts that need no GPU: the two entry points are declared, and the
classes' ``posterior_expect`` / ``reconstruct`` / ``impute`` on the oracle engine (the NumPy route on ``var_x``)."""
import os
import re

import numpy as np
import pytest

from oracle.engine import OracleEngine
from pysvihmm_amd import _lib
from tests import posterior_expect_helpers as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, T, D = 3, 40, 2
NAMES = ("niw", "diag", "pgauss", "poisson", "mcat")


def test_entry_points_are_declared():
    code = open(os.path.join(ROOT, "include", "svihmm.h")).read()
    for fn in ("svihmm_posterior_expect", "svihmm_posterior_expect_entries"):
        assert fn in _lib.SIGNATURES
        assert re.search(r"\bint\s+%s\s*\(" % fn, code)
    assert len(_lib.SIGNATURES["svihmm_posterior_expect"][1]) == 4
    assert len(_lib.SIGNATURES["svihmm_posterior_expect_entries"][1]) == 7
    assert re.search(r"#define\s+SVIHMM_ABI_VERSION\s+3\b", code)
    assert not hasattr(OracleEngine, "posterior_expect") and not hasattr(OracleEngine, "posterior_expect_entries")


def fitted(name):
    """A model after infer() whose data then gets absent entries (NaN; for pgauss a sentinel, for the counts a negative
    one too): the NIW and diagonal families cannot be fitted on NaN rows, every family can be imputed."""
    x = P.small_data(name, T, D)
    rng = np.random.default_rng(8)
    holes = rng.random(x.shape) < 0.2
    holes[7] = True                                    # a row with nothing present
    if name in ("pgauss", "poisson", "mcat"):
        x[holes] = np.nan
        if name == "pgauss":
            x[3, 1] = 1e308
        if name == "poisson":
            x[3, 1] = -1.0
    m = P.small_model(name, x, K=K, engine=OracleEngine(), maxit=2)
    m.mask[[2, 7, 11]] = True                          # masked rows are not special
    m.infer(fused=name in ("niw", "diag"))             # (the oracle engine evaluates the product families on the host)
    if name in ("niw", "diag"):
        m.obs[holes] = np.nan
    absent = holes.copy()
    absent[3, 1] |= name in ("pgauss", "poisson")
    return m, absent


@pytest.mark.parametrize("name", NAMES)
def test_reconstruct_and_impute_on_the_oracle_engine(name):
    m, absent = fitted(name)
    assert m.var_x.shape == (T, K) and np.all(np.isfinite(m.var_x))
    tab = P.family_table(m, name)
    rec = m.reconstruct()
    np.testing.assert_array_equal(rec, m.var_x @ tab)
    assert rec.shape == (T, 6 if name == "mcat" else D)
    np.testing.assert_array_equal(m.posterior_expect(tab), rec)
    np.testing.assert_array_equal(m.posterior_expect(tab[:, 0]), (m.var_x @ tab[:, :1]))
    if name == "mcat":
        np.testing.assert_allclose(rec[:, :3].sum(axis=1), 1.0, rtol=1e-12)
        with pytest.raises(NotImplementedError, match=r"reconstruct\(\)"):
            m.impute()
        return
    before = m.obs.copy()
    out = m.impute()
    np.testing.assert_array_equal(m.obs, before)                     # a copy: the data stay
    assert out.shape == before.shape and absent.sum() > D
    np.testing.assert_array_equal(out[~absent].view(np.uint64), before[~absent].view(np.uint64))
    rows, cols = np.nonzero(absent)
    want = P.entry_loop(m.var_x, tab, rows, cols)
    np.testing.assert_array_equal(out[rows, cols], want)
    np.testing.assert_array_equal(m.posterior_expect_entries(tab, rows, cols), want)
    assert np.all(np.isfinite(out))
    np.testing.assert_allclose(out[rows, cols], rec[rows, cols], rtol=1e-13)


def test_list_obs_comes_back_as_a_list():
    lengths = (17, 1, 22)
    x = P.small_data("diag", sum(lengths), D)
    off = np.concatenate(([0], np.cumsum(lengths)))
    m = P.small_model("diag", [x[a:b] for a, b in zip(off[:-1], off[1:])], K=K, engine=OracleEngine(), maxit=2)
    m.infer()
    x = m.obs                                          # (the concatenated rows the model holds)
    x[np.random.default_rng(2).random(x.shape) < 0.2] = np.nan
    tab = P.family_table(m, "diag")
    rec, out = m.reconstruct(), m.impute()
    assert isinstance(rec, list) and [len(r) for r in rec] == list(lengths)
    assert isinstance(out, list) and [len(r) for r in out] == list(lengths)
    np.testing.assert_array_equal(np.concatenate(rec), m.var_x @ tab)
    rows, cols = np.nonzero(np.isnan(x))
    np.testing.assert_array_equal(np.concatenate(out)[rows, cols], P.entry_loop(m.var_x, tab, rows, cols))
    # rows are numbered over the concatenation
    np.testing.assert_array_equal(m.posterior_expect_entries(tab, [off[2]], [1]),
                                  P.entry_loop(m.var_x, tab, [off[2]], [1]))


def test_other_emitters_and_bad_tables_are_refused():
    m, _ = fitted("pgauss")

    class Other(object):
        pass
    keep = m.var_emit
    m.var_emit = np.array([Other() for _ in range(K)])
    with pytest.raises(NotImplementedError, match=r"posterior_expect\(table\)"):
        m.reconstruct()
    with pytest.raises(NotImplementedError, match=r"posterior_expect\(table\)"):
        m.impute()
    m.var_emit = keep
    with pytest.raises(ValueError, match="table must be a"):
        m.posterior_expect(np.zeros((K + 1, 2)))
    with pytest.raises(ValueError, match="one length"):
        m.posterior_expect_entries(np.zeros((K, 2)), [0, 1], [0])
    with pytest.raises(ValueError, match="outside"):
        m.posterior_expect_entries(np.zeros((K, 2)), [T], [0])
