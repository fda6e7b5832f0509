"""Step-major message layout of the tiled fp64 epoch E-step (csrc/kernels_msg_layout.h).

The dispatch stores Eh / ah / bh step-major exactly where the sweeps are k_sweeps_lin<4, true, 0> behind the
row-tile orbit emission kernel (svihmm_hip.hip, step_major_ok): K = 64, fp64, NIW emission with D % 8 == 0, and

* B >= lin_wave_max = 4 * CUs + 1 windows (below it the wave-per-window / fused kernels run), and
* B * Lm >= 128 * CUs rows (at least one 128-row emission workgroup per CU).

Every case here has B = 16 n + 3 windows above both thresholds at the MI355X's 256 CUs, so the last 16-window
group is partial.  Variant 17 = 1 forces the row-major layout on the same path.  The layout only moves
rows: the packed statistics and the posteriors must be bit-identical between the two, and match the C oracle at
the tolerances of test_gpu_parity.py / test_gpu_fullsize.py.
"""
import numpy as np
import pytest

from tests.helpers import make_problem, unpack, effective_cores

pytestmark = pytest.mark.gpu
K, D = 64, 32
NCORE = effective_cores()


NCU = 256      # MI355X; both thresholds grow with the CU count, so a smaller device takes the same path


def _windows(Lm):
    ncu = NCU
    need = max(4 * ncu + 1, -(-128 * ncu // Lm))
    B = 16 * (-(-need // 16)) + 3
    assert B >= 4 * ncu + 1 and B * Lm >= 128 * ncu and B % 16 == 3
    return B


_PROBLEMS = {}


def _problem(Lm):
    if Lm not in _PROBLEMS:
        B = _windows(Lm)
        pb = make_problem(K, D, B * Lm, seed=1234 + Lm)
        mask = np.zeros(B * Lm, bool)
        mask[[0, 1, Lm - 1, Lm, 7 * Lm + Lm // 2, (B - 2) * Lm // 2, B * Lm // 3]] = True      # a few masked rows
        pb["mask"] = mask
        _PROBLEMS[Lm] = (B, pb)
    return _PROBLEMS[Lm]


CASES = [
    # Lm, TRANS_WRAP, MASK_AS_NAN, overlapping starts
    (2, True, False, False), (2, False, True, True),
    (5, True, True, True), (5, False, False, False),
    (257, True, False, False), (257, False, True, True), (257, True, True, False), (257, False, False, True),
]


@pytest.fixture(scope="module")
def eng():
    from pysvihmm_amd.engine import HipEngine
    e = HipEngine(0)
    yield e
    e.close()


@pytest.mark.parametrize("Lm,wrap,masked,overlap", CASES,
                         ids=["L%d-%s-%s-%s" % (c[0], "wrap" if c[1] else "nowrap", "nan" if c[2] else "plain",
                                                "overlap" if c[3] else "tiled") for c in CASES])
def test_epoch_layout(eng, Lm, wrap, masked, overlap):
    from pysvihmm_amd import _lib as L
    from oracle import ref_c
    B, pb = _problem(Lm)
    stride = max(1, Lm // 2) if overlap else Lm       # overlapping windows start half a window apart
    starts = np.arange(B, dtype=np.int64) * stride
    flags = (L.TRANS_WRAP if wrap else 0) | (L.MASK_AS_NAN if masked else 0)
    par = (pb["mod_init"], pb["ltran"], pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    eng.set_obs(pb["obs"], pb["mask"])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    res = {}
    try:
        for name, v in (("step", 0), ("row", 1)):
            eng.set_variant("msg_layout", v)
            st = eng.estep(starts, Lm, flags=flags)
            res[name] = (st.buf.copy(), eng.read_intermediate("var_x", B, Lm))
    finally:
        eng.set_variant("msg_layout", 0)
    # (b), (c): bit-identical statistics and posteriors under the two layouts
    assert np.array_equal(res["step"][0], res["row"][0])
    assert np.array_equal(res["step"][1], res["row"][1])
    # (a) against the C oracle: the whole step ...
    ref = ref_c.estep_minibatch(pb["obs"], pb["mask"], starts, Lm, *par, flags=flags, threads=NCORE)
    A, xbar, neff, S, lb = unpack(ref, K, D)
    g = unpack(res["step"][0], K, D)
    sc = B * Lm
    np.testing.assert_allclose(g[0], A, rtol=1e-6, atol=1e-10 * sc)
    np.testing.assert_allclose(g[1], xbar, rtol=1e-6, atol=1e-9 * sc)
    np.testing.assert_allclose(g[2], neff, rtol=1e-6, atol=1e-10 * sc)
    np.testing.assert_allclose(g[3], S, rtol=1e-6, atol=1e-8 * sc)
    np.testing.assert_allclose(g[4], lb, rtol=1e-11)
    # ... and the posteriors of windows in the first, a middle and the partial last group
    q_all = res["step"][1]
    for b in (0, 15, 16, 16 * (B // 32) + 5, B - 3, B - 1):
        s0 = int(starts[b])
        ll = ref_c.lliks_niw(pb["obs"][s0:s0 + Lm], pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        if masked:
            ll[pb["mask"][s0:s0 + Lm]] = 0.0
        q, _ = ref_c.posterior(ref_c.forward(ll, pb["mod_init"], pb["ltran"]), ref_c.backward(ll, pb["ltran"]))
        np.testing.assert_allclose(q_all[b], q, rtol=1e-6, atol=1e-12)
