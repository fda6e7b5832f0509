"""The emission family is one value on the Python side too: ``hmmbase.FAMILIES`` (which family a model is, what the
classes do per family) and ``engine.FAMILY_STATS`` (the packed statistics of a family).  No GPU: the oracle engine,
with the three ``set_emission_*`` the product families ask an engine for, stands in where a predicate wants one.

The tests whose name ends in ``_table`` name the two tables; the others state the same facts through the methods the
classes had before the tables and hold without them."""
import numpy as np
import pytest

from oracle.engine import OracleEngine
from pysvihmm_amd import engine as E
from pysvihmm_amd import hmmbase, hmmbatchcd
from pysvihmm_amd.distributions import (Categorical, DiagonalGaussian, Gaussian, ProductCategorical, ProductGaussian,
                                        ProductPoisson)

ORDER = ("niw", "diag", "cat", "mcat", "poisson", "pgauss")
SVI = {"niw": "niw", "diag": "diag", "cat": "cat", "mcat": "mcat", "poisson": "poisson", "pgauss": None}
ENTRYWISE = ("mcat", "poisson", "pgauss")
PRED = {n: "_%s_fastpath" % n for n in ORDER}
K, T = 3, 40


class _EveryFamily(OracleEngine):
    """An engine that offers every family's setter (the predicates only ask whether it is there)."""
    set_emission_mcat = set_emission_poisson = set_emission_pgauss = None


def _model(name, engine=None):
    rng = np.random.default_rng(3)
    np.random.seed(1)
    D = 1 if name == "cat" else 2
    if name in ("niw", "diag", "pgauss"):
        x = rng.normal(size=(T, D))
    else:
        x = rng.integers(0, 3, size=(T, D)).astype(float)
    kw = dict(mu_0=np.zeros(D), nus_0=0.1, alphas_0=2.0, betas_0=2.0)
    emit = {"niw": lambda: Gaussian(mu=rng.normal(size=D), sigma=np.eye(D), mu_0=np.zeros(D), sigma_0=np.eye(D),
                                    kappa_0=0.5, nu_0=D + 2.0),
            "diag": lambda: DiagonalGaussian(mu=rng.normal(size=D), **kw),
            "cat": lambda: Categorical(alphav_0=np.ones(3)),
            "mcat": lambda: ProductCategorical(alphav_0=[np.ones(3), np.ones(3)]),
            "poisson": lambda: ProductPoisson(np.ones(D), np.ones(D), max_count=20),
            "pgauss": lambda: ProductGaussian(mu=rng.normal(size=D), sigmas=np.ones(D), **kw)}[name]
    return hmmbatchcd.VBHMM(x, np.ones(K), np.ones((K, K)), np.array([emit() for _ in range(K)]),
                            mask=np.zeros(T, bool), maxit=1, engine=engine or _EveryFamily())


@pytest.mark.parametrize("name", ORDER)
def test_one_predicate_holds_per_model_and_the_methods_agree(name):
    m = _model(name)
    assert [n for n in ORDER if getattr(m, PRED[n])()] == [name]
    assert m._device_family()
    assert m._svi_family() == SVI[name]
    assert m._heldout_family() == name
    if SVI[name]:
        assert m._svi_plain_vlb(name)
    # entry-wise held-out scores: refused by the model's family before anything else is looked at
    if name not in ENTRYWISE:
        with pytest.raises(NotImplementedError, match="entry-wise scores need"):
            m.heldout_entries_logprob([0], [0], [1.0])
    else:
        with pytest.raises(ValueError, match="not blanked"):
            m.heldout_entries_logprob([0], [0], [1.0])


def test_product_gaussian_is_not_the_diagonal_family():
    m = _model("pgauss")
    assert not m._diag_fastpath() and m._pgauss_fastpath()
    assert not hmmbase.is_diag_gaussian(m.var_emit[0])
    m = _model("pgauss", OracleEngine())          # an engine without the family: host lliks, no device family at all
    assert not m._pgauss_fastpath() and not m._diag_fastpath() and not m._device_family()
    assert m._heldout_family() == "pgauss"        # (what the emitters' types say)


def test_batch_stats_route_filters_by_family():
    class WithStats(_EveryFamily):
        suffstats = None
    for name in ORDER:
        m = _model(name, WithStats())
        lit = hmmbatchcd.VBHMM.global_update
        assert m._batch_stats_route(lit)
        assert m._batch_stats_route(lit, ("niw", "diag")) == (name in ("niw", "diag"))


STATS = {"niw": (E.PackedStats, (2,)), "diag": (E.PackedDiagStats, (2,)), "cat": (E.PackedCatStats, (5,)),
         "mcat": (E.PackedMCatStats, ((2, 4),)), "poisson": (E.PackedPoissonStats, (2,)),
         "pgauss": (E.PackedGaussTrackStats, (2, np.array([0.5, -1.0])))}
SHAPE_FIELDS = ("K", "D", "V", "Vs", "F")


@pytest.mark.parametrize("name", ORDER)
def test_rewrap_packed_keeps_class_and_shape(name):
    cls, args = STATS[name]
    n = cls.size(K, args[0])
    st = cls(np.arange(n, dtype=np.float64), K, *args)
    assert st.lb.shape == (1,) and st.lb[0] == n - 1           # the view covers the buffer to its last entry
    other = np.zeros(n)
    re = E.rewrap_packed(st, other)
    assert type(re) is cls and re.buf is other
    for f in SHAPE_FIELDS:
        assert getattr(re, f, None) == getattr(st, f, None)
    if name == "pgauss":
        assert re.origin is st.origin


def test_rewrap_packed_takes_the_oracle_engines_views():
    """The batch classes sum the per-sequence statistics of whatever engine they run on."""
    from oracle import engine as O
    for cls, w in ((O._Packed, 2), (O._PackedDiag, 2), (O._PackedCat, 5)):
        size = {O._Packed: E.PackedStats, O._PackedDiag: E.PackedDiagStats, O._PackedCat: E.PackedCatStats}[cls].size
        st = cls(np.zeros(size(K, w)), K, w)
        other = np.ones(size(K, w))
        re = E.rewrap_packed(st, other)
        assert type(re) is cls and re.buf is other and re.K == K
        assert getattr(re, "V", None) == getattr(st, "V", None) and getattr(re, "D", None) == getattr(st, "D", None)


# ---- the tables themselves
def test_order_of_the_family_table():
    assert tuple(f.name for f in hmmbase.FAMILIES) == ORDER
    assert tuple(f.pred for f in hmmbase.FAMILIES) == tuple(PRED[n] for n in ORDER)
    assert set(E.FAMILY_STATS) == set(ORDER) and hmmbase.FAMILY == {f.name: f for f in hmmbase.FAMILIES}


@pytest.mark.parametrize("name", ORDER)
def test_model_methods_agree_with_the_family_table(name):
    m = _model(name)
    f = m._family()
    assert f is hmmbase.FAMILY[name]
    assert m._device_family() and m._heldout_family() == f.name and f.by_type(m)
    assert m._svi_family() == (f.name if f.svi_method else None)
    assert (f.svi_method is None) == (f.svi_args is None) == (f.svi_pull is None) == (f.emitter is None) == (SVI[name] is None)
    assert f.heldout == ("entries" if name in ENTRYWISE else "rows")
    assert type(m.var_emit[0]) is f.emitter or name == "pgauss"
    assert [g.name for g in hmmbase.FAMILIES if g.by_type(m)] == [name]
    assert _model(name, OracleEngine())._family() is (f if name in ("niw", "diag", "cat") else None)


def test_family_asks_the_predicates_in_order_and_stops_table():
    asked = []

    class Spy(hmmbatchcd.VBHMM):
        pass
    for n in ORDER:
        setattr(Spy, PRED[n], lambda self, n=n: asked.append(n) or n == "cat")
    m = _model("cat")
    m.__class__ = Spy
    assert m._family().name == "cat" and asked == ["niw", "diag", "cat"]
    del asked[:]
    assert m._svi_family() == "cat" and asked == ["niw", "diag", "cat"]


@pytest.mark.parametrize("name", ORDER)
def test_engine_stats_table(name):
    cls, args = STATS[name]
    fam = E.FAMILY_STATS[name]
    assert fam.stats is cls and fam.size(K, args[0]) == cls.size(K, args[0])
    st = cls(np.zeros(cls.size(K, args[0])), K, *args)
    got = [getattr(st, a) for a in fam.fields]
    assert len(got) == len(args) and all(g is a or g == a for g, a in zip(got, args))
    if name == "pgauss":
        assert fam.block is None and fam.split is None
        return
    blk = np.arange(fam.block(K, args[0]), dtype=np.float64)
    parts = fam.split(blk, K, args[0])
    parts = [parts] if isinstance(parts, np.ndarray) else list(parts)
    assert sum(p.size for p in parts) == blk.size
    np.testing.assert_array_equal(np.concatenate([p.ravel() for p in parts]) if name != "mcat" else
                                  np.concatenate(parts, axis=1).ravel(), blk)
