"""Staging loads of the barrier-free fp64 statistics GEMM (csrc/kernels_stats.h, template parameter SG).

For a whole batch of the scaled sweeps at K = 64 the kernel k_stats_mfma4<5, 2, 2, XK, true, false, double, double, 3, 1>
reads obs / ah / bh with buffer loads: 32-bit lane offsets, rows that contribute nothing out of the descriptors' range.
Variant stats_lds3 = 2 keeps the flat loads from clamped addresses behind value selects (SG = 0) on the same path.  The
route only changes how a value reaches LDS: the packed statistics and the posteriors must be bit-identical between
the two, and match the C oracle at the tolerances of test_gpu_epoch_layout.py.

Every case has B = 16 n + 3 windows above both dispatch thresholds of the tiled epoch (test_gpu_epoch_layout.py), so
the step-major layout is in force and the last 16-window group is partial.  Lm = 2, 5: several windows per 32-row
stage, predecessors across stage and chunk boundaries; 33: a window one row longer than a stage; 257: the bench shape.
Masked rows sit on a window's first and last row and on the last row of a chunk of the statistics launch.

After each batch on the buffer-load route, a call restricted to an inner segment of the windows (off != 0: flat loads,
messages of a longer window) is checked against statistics formed from the oracle's posteriors.
"""
import numpy as np
import pytest

from tests.helpers import make_problem, unpack, effective_cores
from tests.test_gpu_epoch_layout import _windows

pytestmark = pytest.mark.gpu
K, D = 64, 32
NCORE = effective_cores()
FLAT = 2        # SVIHMM_STATS_LDS3_FLAT


def _chunk_rows(n, ncu=256):
    """rows per chunk of the statistics launch (tu_stats.hip, stats_plan: 128 chunks on 256 CUs, whole 32-row stages)"""
    rpc = -(-n // (ncu // 2))
    return -(-rpc // 32) * 32


_PROBLEMS = {}


def _problem(Lm):
    if Lm not in _PROBLEMS:
        B = _windows(Lm)
        n = B * Lm
        pb = make_problem(K, D, n, seed=4321 + Lm)
        rpc = _chunk_rows(n)
        mask = np.zeros(n, bool)
        # tiled starts: batch row = observation row.  First / last row of windows (first, a middle, the last group),
        # the last row of the first two chunks and the row behind it, the batch's last row
        rows = [0, Lm - 1, Lm, 7 * Lm, 8 * Lm - 1, (B - 2) * Lm, (B - 1) * Lm - 1, rpc - 1, rpc, 2 * rpc - 1, n - 1,
                n // 3]
        # starts half a window apart: batch row g is observation row (g // Lm) * stride + g % Lm
        stride = max(1, Lm // 2)
        for g in (rpc - 1, 2 * rpc - 1, 5 * Lm, 6 * Lm - 1):
            rows.append((g // Lm) * stride + g % Lm)
        mask[rows] = True
        pb["mask"] = mask
        _PROBLEMS[Lm] = (B, pb)
    return _PROBLEMS[Lm]


def _inner_reference(pb, starts, Lm, off, ln, wrap, masked):
    """[A_raw, xbar, neff, S] of the segment [off, off + ln) of every window from the oracle's posteriors: the sweeps
    run over the whole window, the segment's first row takes the segment's last row as predecessor under TRANS_WRAP."""
    from oracle import ref_c
    A = np.zeros((K, K)); xbar = np.zeros((K, D)); neff = np.zeros(K); S = np.zeros((K, D, D))
    qs, xs, ws = [], [], []
    for s0 in map(int, starts):
        x = pb["obs"][s0:s0 + Lm]
        m = pb["mask"][s0:s0 + Lm]
        ll = ref_c.lliks_niw(x, pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
        if masked:
            ll[m] = 0.0
        q, _ = ref_c.posterior(ref_c.forward(ll, pb["mod_init"], pb["ltran"]), ref_c.backward(ll, pb["ltran"]))
        q = q[off:off + ln]
        A += q[:-1].T @ q[1:]
        if wrap:
            A += np.outer(q[-1], q[0])
        qs.append(q); xs.append(x[off:off + ln]); ws.append(~m[off:off + ln])
    q = np.concatenate(qs) * np.concatenate(ws)[:, None]
    x = np.concatenate(xs)
    neff = q.sum(0)
    xbar = q.T @ x
    S = np.einsum("tk,ti,tj->kij", q, x, x, optimize=True)
    return A, xbar, neff, S


CASES = [
    # Lm, TRANS_WRAP, MASK_AS_NAN, overlapping starts
    (2, True, False, False), (2, False, True, True),
    (5, True, True, True), (5, False, False, False),
    (33, True, True, False), (33, False, False, True),
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
def test_stats_staging(eng, Lm, wrap, masked, overlap):
    from pysvihmm_amd import _lib as L
    from oracle import ref_c
    B, pb = _problem(Lm)
    stride = max(1, Lm // 2) if overlap else Lm
    starts = np.arange(B, dtype=np.int64) * stride
    flags = (L.TRANS_WRAP if wrap else 0) | (L.MASK_AS_NAN if masked else 0)
    par = (pb["mod_init"], pb["ltran"], pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    eng.set_obs(pb["obs"], pb["mask"])
    eng.set_globals(pb["mod_init"], pb["ltran"])
    eng.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    res, kern = {}, {}
    try:
        for name, v in (("flat", FLAT), ("buffer", 0)):      # (the buffer-load batch last: the inner call follows it)
            eng.set_variant("stats_lds3", v)
            st = eng.estep(starts, Lm, flags=flags)
            kern[name] = eng.last_kernel("stats")
            res[name] = (st.buf.copy(), eng.read_intermediate("var_x", B, Lm))
    finally:
        eng.set_variant("stats_lds3", 0)
    # the two routes ran (on a device with another CU count the thresholds move with it: _windows)
    assert kern["buffer"] == "k_stats_mfma4<5, 2, 2, 3, true, false, double, double, 3, 1>"
    assert kern["flat"] == "k_stats_mfma4<5, 2, 2, 3, true, false, double, double, 3, 0>"
    # (a) bit-identical statistics and posteriors
    assert np.array_equal(res["buffer"][0], res["flat"][0])
    assert np.array_equal(res["buffer"][1], res["flat"][1])
    # (b) against the C oracle
    ref = ref_c.estep_minibatch(pb["obs"], pb["mask"], starts, Lm, *par, flags=flags, threads=NCORE)
    A, xbar, neff, S, lb = unpack(ref, K, D)
    g = unpack(res["buffer"][0], K, D)
    sc = B * Lm
    print("max abs err A %.3g xbar %.3g neff %.3g S %.3g, lb rel %.3g" % (
        np.abs(g[0] - A).max(), np.abs(g[1] - xbar).max(), np.abs(g[2] - neff).max(), np.abs(g[3] - S).max(),
        abs(g[4] - lb) / abs(lb)))
    np.testing.assert_allclose(g[0], A, rtol=1e-6, atol=1e-10 * sc)
    np.testing.assert_allclose(g[1], xbar, rtol=1e-6, atol=1e-9 * sc)
    np.testing.assert_allclose(g[2], neff, rtol=1e-6, atol=1e-10 * sc)
    np.testing.assert_allclose(g[3], S, rtol=1e-6, atol=1e-8 * sc)
    np.testing.assert_allclose(g[4], lb, rtol=1e-11)
    # (c) the next call is one the buffer-load route must not take: an inner segment of a few windows (off = 1)
    nb = 35
    off, ln = (1, Lm - 1) if Lm > 2 else (1, 1)
    st2 = eng.estep(starts[:nb], Lm, flags=flags, inner=(off, ln))
    assert not eng.last_kernel("stats").endswith(", 3, 1>")
    A2, xbar2, neff2, S2 = _inner_reference(pb, starts[:nb], Lm, off, ln, wrap and ln > 0, masked)
    g2 = unpack(st2.buf, K, D)
    sc2 = nb * ln
    np.testing.assert_allclose(g2[0], A2, rtol=1e-6, atol=1e-10 * sc2)
    np.testing.assert_allclose(g2[1], xbar2, rtol=1e-6, atol=1e-9 * sc2)
    np.testing.assert_allclose(g2[2], neff2, rtol=1e-6, atol=1e-10 * sc2)
    np.testing.assert_allclose(g2[3], S2, rtol=1e-6, atol=1e-8 * sc2)
