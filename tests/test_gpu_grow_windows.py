"""svihmm_grow_windows / HipEngine.grow_windows / VBHMM.select_L, select_buffer on the MI355X.

Both routes (the matrix-product kernel and the literal per-candidate loop kept on the device) are held to the
rule's NumPy statement (tests/grow_helpers.grow_direct) evaluated on the device's OWN lliks (eng.loglik), so the
emission kernels' error is out of the comparison: half-widths and step counts exact, residual traces within 1e-10
absolute (the bound test_golden_windows holds the sweeps to; the NumPy model of the product formulation stays
within 3.1e-12 of the literal rule on these inputs).  The inputs keep every value the rule compares with eps at
least 1e-8 away from it, asserted here on the device's lliks as well."""
import re

import numpy as np
import pytest
from scipy.special import digamma

from oracle import ref_numpy
from pysvihmm_amd import _lib as L
from tests.grow_helpers import (CASES, grow_batch, grow_case, grow_direct, grow_problem, reach_windows)

pytestmark = pytest.mark.gpu
CAP = 64          # trace rows kept: more than any case takes steps


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


def _fresh():
    from pysvihmm_amd.engine import HipEngine
    return HipEngine(0)


def _family_case(kind):
    """Small inputs of the other emission families / the mask flag: (p, em, centers, rule, flags)."""
    p = grow_problem(5, 3, 500, seed=31, sep=.5, stick=30, miss=0.2 if kind == "mask" else 0)
    rng = p["rng"]
    K, D, T = p["K"], p["D"], p["T"]
    flags = 0
    if kind == "mask":
        em = ("niw", (p["mu"], p["sigma"], p["kappa"], p["nu"]))
        r = dict(half0=4, m=2, inc=1, cutoff=1000, eps=1e-5, rule=0)
        flags = L.MASK_AS_NAN
        assert p["mask"].sum() > 50
    elif kind == "diag":
        em = ("diag", (p["mu"], 1.0 + rng.random((K, D)), 2.0 + rng.random((K, D)), 1.0 + rng.random((K, D))))
        r = dict(half0=3, m=3, inc=1, cutoff=1000, eps=1e-5, rule=0)
    else:
        V = 7
        theta = rng.dirichlet(np.ones(V) * 2.0, size=K)
        p["obs"] = np.array([rng.choice(V, p=theta[s]) for s in p["sts"]], dtype=float)[:, None]
        a = 0.5 + 40 * theta
        em = ("cat", (digamma(a) - digamma(a.sum(1))[:, None],))
        r = dict(half0=2, m=0, inc=2, cutoff=1000, eps=1e-5, rule=1)
    centers = (rng.integers(0, T - 2 * r["half0"] - 1, size=4) + r["half0"]).astype(np.int64)
    return p, em, centers, r, flags


_inputs = {}


def _case(name):
    if name not in _inputs:
        if name in CASES:
            p, centers, r = grow_case(name)
            _inputs[name] = (p, ("niw", (p["mu"], p["sigma"], p["kappa"], p["nu"])), centers, r, 0)
        else:
            _inputs[name] = _family_case(name)
    return _inputs[name]


def _push(e, p, em):
    e.set_obs(p["obs"], p["mask"])
    e.set_globals(p["mod_init"], p["ltran"])
    getattr(e, "set_emission_" + em[0])(*em[1])


_refs = {}


def _reference(e, name):
    """grow_direct on the device's own lliks of every row a centre can reach; computed once per case (the engine
    must hold the case's model)."""
    if name not in _refs:
        p, em, centers, r, flags = _case(name)
        starts, W = reach_windows(centers, p["T"], r["half0"], r["inc"], r["cutoff"])
        ll = e.loglik(starts, W, flags=flags)
        compared = []
        half, steps, trace = grow_batch(lambda *a, **k: grow_direct(*a, compared=compared, **k), ll, starts,
                                        p["mod_init"], p["ltran"], p["T"], centers, trace_cap=CAP, **r)
        margin = float(np.min(np.abs(np.array(compared) - r["eps"])))
        print("case %s: reference half-widths %s, smallest distance of a compared value from eps %.3g"
              % (name, half.tolist(), margin))
        assert margin >= 1e-8
        assert steps.max() < CAP
        _refs[name] = (half, steps, trace)
    return _refs[name]


def _call(e, centers, r, flags=0, method="auto", trace_cap=CAP):
    return e.grow_windows(centers, r["half0"], probe_off=r["m"], increment=r["inc"], cutoff=r["cutoff"],
                          epsilon=r["eps"], rule=r["rule"], flags=flags, method=method, trace_cap=trace_cap)


def _check(name, method, got, want):
    half, steps, trace = got
    rh, rs, rt = want
    assert half.dtype == np.int32 and steps.dtype == np.int32
    dev = float(np.nanmax(np.abs(trace - rt))) if np.isfinite(rt).any() else 0.0
    print("case %s, %s: half-widths %s, steps %s, largest trace deviation from NumPy %.3g"
          % (name, method, half.tolist(), steps.tolist(), dev))
    np.testing.assert_array_equal(half, rh)
    np.testing.assert_array_equal(steps, rs)
    np.testing.assert_array_equal(np.isnan(trace), np.isnan(rt))      # NaN exactly past a centre's steps
    assert dev <= 1e-10


@pytest.mark.parametrize("method", ["products", "literal"])
@pytest.mark.parametrize("name", sorted(CASES) + ["diag", "cat", "mask"])
def test_cases_against_numpy_on_device_lliks(eng, name, method):
    p, em, centers, r, flags = _case(name)
    _push(eng, p, em)
    want = _reference(eng, name)
    got = _call(eng, centers, r, flags, method)
    _check(name, method, got, want)
    if r["m"] == 0:
        np.testing.assert_array_equal(got[2][:, :, 0], got[2][:, :, 1])
    # a trace buffer shorter than the steps: truncated, same half-widths and step counts; no trace at all
    h2, s2, t2 = _call(eng, centers, r, flags, method, trace_cap=2)
    np.testing.assert_array_equal(h2, got[0])
    np.testing.assert_array_equal(s2, got[1])
    np.testing.assert_array_equal(t2, got[2][:, :2])
    h0, s0, t0 = _call(eng, centers, r, flags, method, trace_cap=0)
    assert t0 is None
    np.testing.assert_array_equal(h0, got[0])
    np.testing.assert_array_equal(s0, got[1])


def test_auto_dispatch_wide_model(eng):
    """K = 100: outside the product kernel; PRODUCTS says so, AUTO takes the literal route."""
    p = grow_problem(100, 2, 400, seed=41, sep=.5, stick=150)
    centers = (p["rng"].integers(0, 400 - 2 * 3 - 1, size=3) + 3).astype(np.int64)
    r = dict(half0=3, m=3, inc=1, cutoff=1000, eps=1e-5, rule=0)
    _inputs["wide"] = (p, ("niw", (p["mu"], p["sigma"], p["kappa"], p["nu"])), centers, r, 0)
    _push(eng, p, _inputs["wide"][1])
    with pytest.raises(RuntimeError, match=re.escape(
            "svihmm_grow_windows: method PRODUCTS needs K <= 64 and every ltran entry >= SVIHMM_LTRAN_LINEAR_MIN (K = 100)")):
        _call(eng, centers, r, method="products")
    _check("wide", "auto", _call(eng, centers, r, method="auto"), _reference(eng, "wide"))


def test_auto_dispatch_sparse_transitions(eng):
    """K = 16 with pseudo-counts of 1e-3 in var_tran: ltran entries near -1000, outside the linear range."""
    p = grow_problem(16, 3, 400, seed=42, sep=.4, stick=60)
    vt = p["var_tran"].copy()
    vt[p["rng"].random((16, 16)) < 0.2] = 1e-3
    vt[np.arange(16), np.arange(16)] = 61.0
    p["mod_init"], p["ltran"] = ref_numpy.psi_expectations(p["var_init"], vt)
    assert p["ltran"].min() < -600
    centers = (p["rng"].integers(0, 400 - 2 * 2 - 1, size=3) + 2).astype(np.int64)
    r = dict(half0=2, m=1, inc=1, cutoff=1000, eps=1e-5, rule=0)
    _inputs["sparse"] = (p, ("niw", (p["mu"], p["sigma"], p["kappa"], p["nu"])), centers, r, 0)
    _push(eng, p, _inputs["sparse"][1])
    with pytest.raises(RuntimeError, match=re.escape(
            "method PRODUCTS needs K <= 64 and every ltran entry >= SVIHMM_LTRAN_LINEAR_MIN (K = 16, ltran below the linear range)")):
        _call(eng, centers, r, method="products")
    _check("sparse", "auto", _call(eng, centers, r, method="auto"), _reference(eng, "sparse"))


def test_a_centre_does_not_depend_on_its_batch(eng):
    p, em, centers, r, flags = _case("C")
    _push(eng, p, em)
    hb, sb, tb = _call(eng, centers, r, flags, "products")
    h1, s1, t1 = _call(eng, centers[:1], r, flags, "products")
    assert h1[0] == hb[0] and s1[0] == sb[0] and s1[0] > 5
    np.testing.assert_array_equal(t1[0], tb[0])                       # bit-identical, NaN padding included
    # ... nor on its place in the batch
    h2, s2, t2 = _call(eng, centers[::-1], r, flags, "products")
    np.testing.assert_array_equal(t2[::-1], tb)


def test_failures_leave_the_engine_usable():
    rng = np.random.default_rng(0)
    T, K, D = 300, 4, 3
    obs = rng.normal(size=(T, D))
    e = _fresh()
    try:
        def bad(msg, *a, **k):
            e.profile_reset()
            with pytest.raises(RuntimeError, match="^" + re.escape("svihmm_grow_windows failed: svihmm_grow_windows: " + msg) + "$"):
                e.grow_windows(*a, **k)
            assert not e.profile_read()                   # nothing was launched or copied

        def raw(msg, centers, out_half, eps=1e-5):           # (C ABI: NULL pointers, non-finite epsilon)
            e.profile_reset()
            c = None if centers is None else L.i64ptr(centers)
            with pytest.raises(RuntimeError, match=re.escape("svihmm_grow_windows: " + msg)):
                L.check(e._lib.svihmm_grow_windows(e._h, c, 1, 2, 0, 1, 1000, eps, 0, 0, 0,
                                                   None if out_half is None else out_half.ctypes.data, None, None, 0),
                        "svihmm_grow_windows")
            assert not e.profile_read()
        e.profile(True)
        one, half = np.array([50], dtype=np.int64), np.empty(1, dtype=np.int32)
        bad("no globals: call svihmm_set_globals first", [50], 2)
        mi = np.log(rng.dirichlet(np.ones(K)))
        lt = np.log(rng.dirichlet(np.ones(K), size=K))
        e.set_globals(mi, lt)
        bad("no observations: call svihmm_set_obs first", [50], 2)
        e.set_obs(obs)
        bad("no emission family: call svihmm_set_emission_niw / _diag / _cat first", [50], 2)
        A = rng.normal(size=(K, D, D))
        niw = (rng.normal(size=(K, D)), np.einsum('kij,klj->kil', A, A) + D * np.eye(D), np.ones(K), D + 2.0 + np.zeros(K))
        e.set_emission_niw(*niw)
        e.profile(False)
        good = e.grow_windows([50, 200], 2, trace_cap=4)
        e.profile(True)
        raw("centers and out_half must be given", None, half)
        raw("centers and out_half must be given", one, None)
        raw("epsilon must be finite", one, half, eps=float("nan"))
        raw("epsilon must be finite", one, half, eps=float("inf"))
        bad("n must be positive", [], 2)
        bad("increment must be positive", [50], 2, increment=0)
        bad("need 0 <= probe_off <= half0", [50], -1)
        bad("need 0 <= probe_off <= half0", [50], 2, probe_off=-1)
        bad("need 0 <= probe_off <= half0", [50], 2, probe_off=3)
        bad("rule must be 0 (last residual) or 1 (running average)", [50], 2, rule=2)
        bad("start window of centre 1 reaches outside [0, T)", [50, 1], 2)
        bad("start window of centre 0 reaches outside [0, T)", [T - 2], 2)
        bad("SVIHMM_USE_HOST_LLIKS is not supported (host lliks have no row axis to grow along)", [50], 2,
            flags=L.USE_HOST_LLIKS)
        e.set_globals(np.log(rng.dirichlet(np.ones(K + 1))), np.log(rng.dirichlet(np.ones(K + 1), size=K + 1)))
        bad("K of the globals (%d) differs from the emission family's K (%d)" % (K + 1, K), [50], 2)
        lt2 = lt.copy()
        lt2[0, 1] = -700.0
        e.set_globals(mi, lt2)
        bad("method PRODUCTS needs K <= 64 and every ltran entry >= SVIHMM_LTRAN_LINEAR_MIN (K = 4, ltran below the linear range)",
            [50], 2, method="products")
        # still usable, same answer
        e.profile(False)
        e.set_globals(mi, lt)
        again = e.grow_windows([50, 200], 2, trace_cap=4)
        for a, b in zip(good, again):
            np.testing.assert_array_equal(a, b)
    finally:
        e.close()


@pytest.mark.parametrize("method", ["products", "literal"])
def test_state_after_a_call(method):
    p, em, centers, r, flags = _case("B")
    e = _fresh()
    try:
        _push(e, p, em)
        starts = np.random.default_rng(1).integers(0, p["T"] - 33, size=8)
        e.estep(starts, 33, flags=L.TRANS_WRAP, read=False)
        want = e.read_packed().buf.copy()
        e.set_precision("f32")
        mode = e.precision()
        half, steps, _ = _call(e, centers[:1] if method == "literal" else centers, r, flags, method)
        assert e.precision() == mode
        e.set_precision("f64")
        np.testing.assert_array_equal(e.read_packed().buf, want)
        # the lliks readable afterwards are those of the grown windows: the reach windows of the emission pass
        # (products), the last candidate = the grown window itself for a single centre (literal)
        if method == "products":
            st, W = reach_windows(centers, p["T"], r["half0"], r["inc"], r["cutoff"])
            got = e.read_intermediate("lliks", len(centers), W)
        else:
            st, W = centers[:1] - half[0], 2 * int(half[0]) + 1
            got = e.read_intermediate("lliks", 1, W)
        np.testing.assert_array_equal(got, e.loglik(st, W, flags=flags))
    finally:
        e.close()


class _Counting(object):
    def __init__(self, engine):
        self.n = {"grow_windows": 0, "forward_backward": 0}
        for nm in self.n:
            setattr(engine, nm, self._wrap(nm, getattr(engine, nm)))

    def _wrap(self, nm, fn):
        def f(*a, **k):
            self.n[nm] += 1
            return fn(*a, **k)
        return f


def test_class_route():
    from pysvihmm_amd import hmmsgd_metaobs
    from tests.test_grow_windows_ref import _model
    p, _, _ = grow_case("A")
    hmm = _model(p, None)
    assert hmm.engine.name == "hip" and hmm.device_growth
    cnt = _Counting(hmm.engine)
    calls = [("select_L", dict(numIndices=4, epsilon=1e-5, minHalfL=2)),
             ("select_L", dict(numIndices=3, epsilon=1e-4, minHalfL=1, avgResidual=True, Lincrement=2)),
             ("select_buffer", dict(numIndices=4, epsilon=1e-5, halfL=5)),
             ("select_buffer", dict(numIndices=2, epsilon=1e-9, halfL=3, Lincrement=2, Lcutoff=12))]
    results = []
    for i, (nm, kw) in enumerate(calls):
        hmm.device_growth = True
        before = dict(cnt.n)
        np.random.seed(20 + i)
        dev = getattr(hmm, nm)(**kw)
        state = np.random.get_state()[1].copy()
        assert cnt.n["grow_windows"] == before["grow_windows"] + 1
        assert cnt.n["forward_backward"] == before["forward_backward"]
        hmm.device_growth = False
        np.random.seed(20 + i)
        host = getattr(hmm, nm)(**kw)
        np.testing.assert_array_equal(np.random.get_state()[1], state)      # the same draws were consumed
        assert cnt.n["grow_windows"] == before["grow_windows"] + 1
        assert cnt.n["forward_backward"] > before["forward_backward"]
        print("%s(%s): device route %d, host route %d" % (nm, kw, dev, host))
        assert isinstance(dev, int) and dev == host
        results.append(dev)
    hmm.device_growth = True
    assert hmm.select_L(numIndices=0) == -1 and hmm.select_buffer(numIndices=0) == -1
    with pytest.raises(RuntimeError):
        hmm.select_buffer(avgResidual=True)

    # a type that overrides one of the per-window hooks keeps the host loop
    class Sub(hmmsgd_metaobs.VBHMM):
        def get_marginal(self, var_over_x, index):
            return super(Sub, self).get_marginal(var_over_x, index)
    sub = _model(p, hmm.engine)
    sub.__class__ = Sub
    before = dict(cnt.n)
    np.random.seed(20)
    assert sub.select_L(**calls[0][1]) == results[0]
    assert cnt.n["grow_windows"] == before["grow_windows"] and cnt.n["forward_backward"] > before["forward_backward"]
