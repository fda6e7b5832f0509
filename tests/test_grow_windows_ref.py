"""The growth rule of svihmm_grow_windows in NumPy (tests/grow_helpers.py), without a GPU: the literal
per-candidate statement against the matrix formulation the product kernel uses, the margin the shared inputs
keep from the rule's threshold, the class methods on the CPU engine, and the new symbol's export."""
import ctypes

import numpy as np
import pytest

from oracle import ref_numpy
from pysvihmm_amd import _lib
from tests.grow_helpers import (CASES, EXPECTED_HALF, grow_case, grow_direct, grow_products, niw_lliks)

_cache = {}


def _both(name):
    """(half, traces, compared values) of both formulations on case ``name``, computed once."""
    if name not in _cache:
        p, centers, r = grow_case(name)
        ll = niw_lliks(p)
        out = {"direct": ([], [], []), "products": ([], [], [])}
        for key, fn in (("direct", grow_direct), ("products", grow_products)):
            for c in centers:
                h, tr = fn(ll, p["mod_init"], p["ltran"], p["T"], c, compared=out[key][2], **r)
                out[key][0].append(h)
                out[key][1].append(tr)
        _cache[name] = (out, r)
    return _cache[name]


@pytest.mark.parametrize("name", sorted(CASES))
def test_products_equal_direct(name):
    out, r = _both(name)
    hd, td, _ = out["direct"]
    hp, tp, _ = out["products"]
    assert hd == hp
    worst = 0.0
    for a, b in zip(td, tp):
        assert a.shape == b.shape
        if len(a):
            worst = max(worst, float(np.max(np.abs(a - b))))
    print("case %s: half-widths %s, largest trace deviation %.3g" % (name, hd, worst))
    assert worst <= 1e-10
    for h, a in zip(hd, td):
        assert h == r["half0"] + r["inc"] * len(a)
    if r["m"] == 0:                                       # one probe row: both residuals are the same number
        for a in td + tp:
            np.testing.assert_array_equal(a[:, 0], a[:, 1])
    if name in EXPECTED_HALF:
        assert (min(hd), max(hd)) == EXPECTED_HALF[name]
    else:
        assert hd == [3, 8, 7, 3]                         # case F: the sequence ends stop the growth
    if name == "E":
        assert all(h > r["cutoff"] for h in hd)           # the cutoff stops it


@pytest.mark.parametrize("name", sorted(CASES))
def test_inputs_keep_a_margin_from_epsilon(name):
    """Every value the rule compares with eps lies at least 1e-8 away from it, under both formulations: an
    agreement of the half-widths within the 1e-10 the traces are held to is then decided by the inputs, not by
    rounding."""
    out, r = _both(name)
    for key in ("direct", "products"):
        v = np.array(out[key][2])
        assert len(v)
        margin = float(np.min(np.abs(v - r["eps"])))
        print("case %s (%s): %d compared values, smallest distance from eps %.3g" % (name, key, len(v), margin))
        assert margin >= 1e-8


def _model(p, engine):
    from pysvihmm_amd import hmmsgd_metaobs
    from pysvihmm_amd.distributions import Gaussian
    K, D = p["K"], p["D"]
    emit = []
    for k in range(K):
        e = Gaussian(mu=p["mu"][k], sigma=np.eye(D), mu_0=np.zeros(D), sigma_0=np.eye(D), kappa_0=0.1, nu_0=D + 2.0)
        e.mu_mf, e.sigma_mf = p["mu"][k].copy(), p["sigma"][k].copy()
        e.kappa_mf, e.nu_mf = float(p["kappa"][k]), float(p["nu"][k])
        emit.append(e)
    hmm = hmmsgd_metaobs.VBHMM(p["obs"].copy(), np.ones(K), np.ones((K, K)), np.array(emit), metaobs_half=5,
                               mb_sz=2, mask=p["mask"], init_tran=p["var_tran"], maxit=1, seed=1, engine=engine)
    hmm.var_init = p["var_init"].copy()
    hmm.var_tran = p["var_tran"].copy()
    return hmm


def class_route_expectation(p, seed, n, half0, m, inc, cutoff, eps, rule, ll=None):
    """What select_L / select_buffer must return after ``np.random.seed(seed)``: the same index draw, the rule
    per index, the largest half-width."""
    np.random.seed(seed)
    idx = np.random.choice(p["T"] - 2 * half0 - 1, size=n) + half0
    mod_init, ltran = ref_numpy.psi_expectations(p["var_init"], p["var_tran"])
    ll = niw_lliks(p) if ll is None else ll
    return max(grow_direct(ll, mod_init, ltran, p["T"], c, half0, m, inc, cutoff, eps, rule)[0] for c in idx)


def test_class_methods_on_the_cpu_engine():
    from oracle.engine import OracleEngine
    p, _, _ = grow_case("A")
    hmm = _model(p, OracleEngine())
    assert not hasattr(hmm.engine, "grow_windows") and hmm.device_growth
    np.random.seed(7)
    assert hmm.select_L(numIndices=3, epsilon=1e-5, minHalfL=2) == class_route_expectation(p, 7, 3, 2, 0, 1, 1000, 1e-5, 0)
    np.random.seed(8)
    assert (hmm.select_L(numIndices=3, epsilon=1e-4, minHalfL=1, avgResidual=True, Lincrement=2)
            == class_route_expectation(p, 8, 3, 1, 0, 2, 1000, 1e-4, 1))
    np.random.seed(9)
    assert hmm.select_buffer(numIndices=3, epsilon=1e-5, halfL=5) == class_route_expectation(p, 9, 3, 5, 5, 1, 1000, 1e-5, 0)
    with pytest.raises(RuntimeError):
        hmm.select_buffer(avgResidual=True)


def test_symbol_declared_and_exported():
    assert "svihmm_grow_windows" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["svihmm_grow_windows"]
    assert res is ctypes.c_int and len(args) == 15
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "svihmm_grow_windows")
    assert _lib.GROW_METHOD == {"auto": 0, "literal": 1, "products": 2}
    assert _lib.load().svihmm_abi_version() == 3
