"""The NumPy draw rule the GPU tests of svihmm_ffbs_windows compare against (tests/ffbs_helpers.py), itself
checked against the reference-shaped sampler of the oracle, and the new symbol at the three places the C
ABI is declared.  CPU only."""
import ctypes
import os
import re

import numpy as np

from oracle import ref_numpy as R
from pysvihmm_amd import _lib
from tests.ffbs_helpers import EXCUSE, backward_sample, check_paths, draw, near_boundary_steps

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
DE = float(np.finfo(np.float64).eps)


def test_helper_sampler_against_the_oracle_on_the_golden_lalpha():
    """oracle.ref_numpy.ffbs_backward_sample normalises p and compares u <= cumsum(p); the helper compares
    u * tot <= cumsum(p): the same draw except within rounding of a boundary (the excuse rule)."""
    g = np.load(os.path.join(GOLDEN, "ffbs_K5_D3_T120.npz"))
    la, var_tran = g["lalpha"], g["var_tran"]
    logA = np.log(var_tran + DE)
    T = la.shape[0]
    excused = 0
    for seed in range(20):
        u = np.random.default_rng(100 + seed).random(T)
        z = backward_sample(la, logA, u)
        zref = R.ffbs_backward_sample(la, var_tran, u)
        assert z.dtype == np.int32 and z.shape == (T,)
        assert check_paths(z, la, logA, u) == 0                   # the walk agrees with its own vectorised recomputation
        excused += check_paths(zref.astype(np.int32), la, logA, u)
        assert near_boundary_steps(z, la, logA, u)[0] == 0
    assert excused <= 1


def test_draw_rule_edges():
    la = np.log(np.array([0.2, 0.3, 0.5]))
    assert draw(la, None, 0.0)[0] == 0
    assert draw(la, None, 0.2 - 1e-9)[0] == 0 and draw(la, None, 0.2 + 1e-9)[0] == 1
    assert draw(la, None, 0.999999)[0] == 2
    assert draw(la, None, 1.0 + 1e-9)[0] == 2                     # no k with u * tot <= c_k: K - 1
    col = np.array([0.0, -np.inf, 0.0])                           # -inf: probability zero, never drawn
    assert all(draw(la, col, u)[0] != 1 for u in np.linspace(0.0, 1.0, 101))
    k, c, tot = draw(la, col, 0.5)
    assert c[1] == c[0] and tot == c[-1]


def test_checker_flags_a_wrong_state_and_excuses_only_a_boundary():
    rng = np.random.default_rng(5)
    K, B, Lm, S = 7, 2, 30, 3
    la = rng.normal(size=(B, Lm, K)) * 3.0
    logA = np.log(rng.dirichlet(np.ones(K), size=K))
    u = rng.random((S, B, Lm))
    z = np.stack([[backward_sample(la[b], logA, u[s, b]) for b in range(B)] for s in range(S)])
    assert check_paths(z, la, logA, u) == 0
    bad = z.copy()
    bad[1, 0, 11] = (bad[1, 0, 11] + 1) % K                       # one wrong state: that step (and only the
    try:                                                          # recomputation of its predecessor) can complain
        check_paths(bad, la, logA, u)
    except AssertionError:
        pass
    else:
        raise AssertionError("a wrong state went unnoticed")
    # a uniform ON a boundary (a one-row window, so nothing cascades): either neighbour passes, one of them
    # as an excused step; a state further away, or the neighbour at a uniform off the boundary, does not
    row = np.log(np.array([[[0.2, 0.3, 0.5]]]))
    _, c, tot = draw(row[0, 0], None, 0.5)
    ub = np.array([[[c[0] / tot]]])
    counts = [check_paths(np.array([[[k]]], dtype=np.int32), row, logA[:3, :3], ub) for k in (0, 1)]
    assert sorted(counts) == [0, 1]
    assert abs(ub[0, 0, 0] * tot - c[0]) <= EXCUSE * tot
    for zz, uu in [(2, ub), (1, ub - 1e-6), (0, ub + 1e-6)]:
        try:
            check_paths(np.array([[[zz]]], dtype=np.int32), row, logA[:3, :3], uu)
        except AssertionError:
            continue
        raise AssertionError("state %d at u = %r went unnoticed" % (zz, uu))


def test_no_near_boundary_steps_at_the_gpu_tests_sizes():
    """The GPU tests allow ONE excused step each.  The count of steps within 1e-11 tot of a boundary, for
    random logits of the scales and state counts those tests use: none in 2e5 steps (the nearest ~1e-8)."""
    total, nearest = 0, 1.0
    steps = 0
    for K, scale, seed in [(3, 0.5, 1), (16, 3.0, 2), (17, 10.0, 3), (64, 40.0, 4), (200, 5.0, 5)]:
        rng = np.random.default_rng(seed)
        Lm, S = 200, 200
        la = rng.normal(size=(1, Lm, K)) * scale
        logA = np.log(rng.dirichlet(np.ones(K), size=K))
        u = rng.random((S, 1, Lm))
        z = rng.integers(0, K, size=(S, 1, Lm)).astype(np.int32)   # any z[t+1] gives a valid step distribution
        n, d = near_boundary_steps(z, la, logA, u)
        total += n
        nearest = min(nearest, d)
        steps += S * Lm
    assert steps == 200000 and total == 0 and nearest > 1e-10, (total, nearest)


def test_symbol_declared_bound_and_exported():
    """Fails before svihmm_ffbs_windows exists."""
    src = open(os.path.join(REPO, "include", "svihmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint\s+svihmm_ffbs_windows\s*\(", code)
    assert re.search(r"#define\s+SVIHMM_ABI_VERSION\s+3\b", code)
    assert "svihmm_ffbs_windows" in _lib.SIGNATURES
    res, args = _lib.SIGNATURES["svihmm_ffbs_windows"]
    assert res is ctypes.c_int and len(args) == 11 and args[8] is ctypes.c_uint64
    lib = ctypes.CDLL(_lib.LIB_PATH)
    assert hasattr(lib, "svihmm_ffbs_windows")
