"""Lean staging and epilogue of the row-tile orbit emission kernel (csrc/kernels_emission.h, k_emission_orbit).

Workgroups that lie wholly inside the batch (K = 16 NT, fp64 storage) stage their rows and leave their results with
less work around the same operations; slot 5 = 6 (default dispatch) / 7 (the 128-row form forced, as 2) keeps the
generic code in every workgroup.  The two must agree bit for bit -- packed statistics and posteriors -- and match the
C oracle at the tolerances of test_gpu_emission_orbit.py / test_gpu_epoch_layout.py / test_gpu_f32.py.
"""
import numpy as np
import pytest

from tests.helpers import make_problem, unpack, effective_cores

pytestmark = pytest.mark.gpu
NCORE = effective_cores()
NCU = 256      # MI355X


def _windows(Lm):
    """B = 16 n + 3 windows above both thresholds of the step-major path (test_gpu_epoch_layout.py: _windows)."""
    need = max(4 * NCU + 1, -(-128 * NCU // Lm))
    return 16 * (-(-need // 16)) + 3


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.set_variant("emission_orbit", 0)
    e.close()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _both(eng, starts, Lm, flags, lean_code, generic_code):
    """(packed statistics, posteriors) under the lean and the generic edges, after asserting that they are the same."""
    from pysvihmm_amd import _lib as L  # noqa: F401
    res = []
    try:
        for code in (lean_code, generic_code):
            eng.set_variant("emission_orbit", code)
            st = eng.estep(starts, Lm, flags=flags)
            res.append((st.buf.copy(), eng.read_intermediate("var_x", len(starts), Lm)))
    finally:
        eng.set_variant("emission_orbit", 0)
    assert np.array_equal(_bits(res[0][0]), _bits(res[1][0])), "packed statistics differ"
    assert np.array_equal(_bits(res[0][1]), _bits(res[1][1])), "posteriors differ"
    return res[0]


# ---- 1. row-major, the 128-row form forced: 60 interior workgroups and one ragged one --------------------------
@pytest.mark.parametrize("D", [8, 16, 24, 32, 40])
def test_row_major_128_row_form(eng, D):
    from pysvihmm_amd import _lib as L
    from oracle import ref_c
    K, T, Lm, B = 64, 9000, 37, 211               # 7807 rows
    pb = make_problem(K, D, T, seed=6400 + D, miss=0.07)
    starts = np.random.default_rng(D).integers(0, T - Lm + 1, size=B)
    eng.set_obs(pb["obs"], pb["mask"])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    for flags in (L.TRANS_WRAP, L.TRANS_WRAP | L.MASK_AS_NAN):
        buf, _ = _both(eng, starts, Lm, flags, L.EMISSION_ORBIT_128, L.EMISSION_ORBIT_128_GENERIC_EDGES)
        ref = ref_c.estep_minibatch(pb["obs"], pb["mask"], starts, Lm, pb["mod_init"], pb["ltran"],
                                    pb["mu"], pb["sigma"], pb["kappa"], pb["nu"], flags)
        np.testing.assert_allclose(buf, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())


# ---- 2. step-major path: every wave holds window starts (Lm = 2), most hold none (257), the smallest batch (32) --
@pytest.mark.parametrize("Lm", [2, 32, 257])
def test_step_major_window_start_density(eng, Lm):
    from pysvihmm_amd import _lib as L
    from oracle import ref_c
    K, D = 64, 32
    B = _windows(Lm)
    pb = make_problem(K, D, B * Lm, seed=4321 + Lm)
    mask = np.zeros(B * Lm, bool)
    mask[[0, 1, Lm - 1, Lm, 7 * Lm + Lm // 2, (B - 2) * Lm // 2, B * Lm // 3]] = True      # a few masked rows
    starts = np.arange(B, dtype=np.int64) * Lm
    flags = L.TRANS_WRAP | L.MASK_AS_NAN
    eng.set_obs(pb["obs"], mask)
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    buf, q_all = _both(eng, starts, Lm, flags, 0, L.EMISSION_ORBIT_GENERIC_EDGES)
    par = (pb["mod_init"], pb["ltran"], pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    ref = ref_c.estep_minibatch(pb["obs"], mask, starts, Lm, *par, flags=flags, threads=NCORE)
    A, xbar, neff, S, lb = unpack(ref, K, D)
    g = unpack(buf, K, D)
    sc = B * Lm
    np.testing.assert_allclose(g[0], A, rtol=1e-6, atol=1e-10 * sc)
    np.testing.assert_allclose(g[1], xbar, rtol=1e-6, atol=1e-9 * sc)
    np.testing.assert_allclose(g[2], neff, rtol=1e-6, atol=1e-10 * sc)
    np.testing.assert_allclose(g[3], S, rtol=1e-6, atol=1e-8 * sc)
    np.testing.assert_allclose(g[4], lb, rtol=1e-11)
    for b in (0, 16, B - 1):
        s0 = int(starts[b])
        ll = ref_c.lliks_niw(pb["obs"][s0:s0 + Lm], pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        ll[mask[s0:s0 + Lm]] = 0.0
        q, _ = ref_c.posterior(ref_c.forward(ll, pb["mod_init"], pb["ltran"]), ref_c.backward(ll, pb["ltran"]))
        np.testing.assert_allclose(q_all[b], q, rtol=1e-6, atol=1e-12)


# ---- 3. non-finite accumulators in interior tiles: the wave-level test must send those waves down the clamps ------
def test_non_finite_accumulators_bit_identity(eng):
    from pysvihmm_amd import _lib as L
    K, D, Lm = 64, 32, 32
    B = _windows(Lm)
    n = B * Lm
    pb = make_problem(K, D, n, seed=77)
    obs = pb["obs"].copy()
    rng = np.random.default_rng(5)
    big = rng.choice(n - 256, size=9, replace=False)            # interior tiles only: the last workgroup is ragged
    obs[big, rng.integers(0, D, size=9)] = np.where(rng.random(9) < 0.5, 1e160, -1e160)
    obs[big[:3], (rng.integers(0, D, size=3) + 1) % D] = -1e160  # two huge entries in one row: inf - inf on the way
    nan_rows = rng.choice(n - 256, size=7, replace=False)
    obs[nan_rows, rng.integers(0, D, size=7)] = np.nan
    starts = np.arange(B, dtype=np.int64) * Lm
    try:
        eng.set_variant("centring", 1)            # a mean over 1e160 would move every row out of range
        eng.set_obs(obs, None)
        eng.set_globals(pb["mod_init"], pb["ltran"])
        eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        _both(eng, starts, Lm, L.TRANS_WRAP, 0, L.EMISSION_ORBIT_GENERIC_EDGES)
    finally:
        eng.set_variant("centring", 0)


# ---- 4. paths that must not change: ragged K and fp32 storage keep the generic code under every code ------------
def test_ragged_k_unchanged(eng):
    from pysvihmm_amd import _lib as L
    from oracle import ref_c
    K, D, T, Lm, B = 50, 32, 9000, 37, 211
    pb = make_problem(K, D, T, seed=5032, miss=0.07)
    starts = np.random.default_rng(50).integers(0, T - Lm + 1, size=B)
    eng.set_obs(pb["obs"], pb["mask"])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    flags = L.TRANS_WRAP | L.MASK_AS_NAN
    buf, _ = _both(eng, starts, Lm, flags, L.EMISSION_ORBIT_128, L.EMISSION_ORBIT_128_GENERIC_EDGES)
    ref = ref_c.estep_minibatch(pb["obs"], pb["mask"], starts, Lm, pb["mod_init"], pb["ltran"],
                                pb["mu"], pb["sigma"], pb["kappa"], pb["nu"], flags)
    np.testing.assert_allclose(buf, ref, rtol=1e-6, atol=1e-9 * np.abs(ref).max())


def test_f32_mode_unchanged(eng):
    from pysvihmm_amd import _lib as L
    from oracle import ref_c
    K, D, T, Lm, B = 64, 32, 9000, 37, 211
    pb = make_problem(K, D, T, seed=6432, miss=0.0, sep=4.0)
    starts = np.random.default_rng(64).integers(0, T - Lm + 1, size=B)
    try:
        eng.set_precision("f32")
        eng.set_obs(pb["obs"], None)
        eng.set_globals(pb["mod_init"], pb["ltran"])
        eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        buf, _ = _both(eng, starts, Lm, L.TRANS_WRAP, L.EMISSION_ORBIT_128, L.EMISSION_ORBIT_128_GENERIC_EDGES)
        assert eng.precision() == ("f32", True)
    finally:
        eng.set_precision("f64")
    ref = ref_c.estep_minibatch(pb["obs"], None, starts, Lm, pb["mod_init"], pb["ltran"], pb["mu"], pb["sigma"],
                                pb["kappa"], pb["nu"], flags=2, threads=NCORE)
    A, xbar, neff, S, lb = unpack(ref, K, D)
    g = unpack(buf, K, D)
    sc, xs = B * Lm, np.abs(pb["obs"]).max()
    for got, want, scale in ((g[0], A, sc), (g[2], neff, sc), (g[1], xbar, sc * xs), (g[3], S, sc * xs ** 2)):
        assert np.all(np.abs(got - want) <= 1e-3 * np.abs(want) + 1e-6 * scale)      # test_gpu_f32.py: _close
    np.testing.assert_allclose(g[4], lb, rtol=1e-6)
