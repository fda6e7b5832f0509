"""Allowed-state sets without a GPU: the bit layout (``util.pack_state_sets`` / ``unpack_state_sets``), the ctypes
prototype, the set generator's cases at the shapes tests/test_gpu_state_sets.py uses, and ``set_state_sets`` of the
batch classes on the oracle engine -- it has no ``set_state_sets``, so the model takes the host-lliks route and clamps
the lliks itself.  Tolerances: those of tests/test_labels_ref.py."""
import ctypes

import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import _lib, hmmbatchcd, hmmsgd_metaobs
from pysvihmm_amd.util import pack_state_sets, unpack_state_sets
from sequences_helpers import build_model, class_data, cut, offsets
from state_sets_helpers import check_cases, clamp_sets, make_sets, singleton_labels

K, D, T = 4, 2, 60
LENGTHS = (23, 1, 30, 6)


# ---- the bit layout --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 5, 64, 65, 256])
def test_pack_unpack_round_trip(k):
    rng = np.random.default_rng(k)
    a = rng.random((37, k)) < 0.4
    a[0] = True
    a[1] = False
    a[2] = False
    a[2, k - 1] = True
    p = pack_state_sets(a)
    W = (k + 63) // 64
    assert p.dtype == np.uint64 and p.shape == (37, W) and p.flags.c_contiguous
    for t in range(37):
        for j in range(W):
            word = int(p[t, j])
            for b in range(64):
                s = 64 * j + b
                assert (word >> b) & 1 == (int(a[t, s]) if s < k else 0), (t, s)      # bit k % 64 of word k // 64
    assert int(p[2, W - 1]) == 1 << ((k - 1) % 64) and not p[1].any()
    back = unpack_state_sets(p, k)
    assert back.dtype == np.bool_ and np.array_equal(back, a)


def test_pack_unpack_refuse_bad_shapes():
    with pytest.raises(ValueError, match="shape"):
        pack_state_sets(np.ones(5, bool))
    with pytest.raises(ValueError, match="uint64"):
        unpack_state_sets(np.zeros((3, 1), dtype=np.uint64), 65)
    with pytest.raises(ValueError, match="uint64"):
        unpack_state_sets(np.zeros((3, 1), dtype=np.int64), 5)


def test_signature_is_declared():
    res, args = _lib.SIGNATURES["svihmm_set_state_sets"]
    assert res is ctypes.c_int
    assert args == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_uint64), ctypes.c_int32]


# ---- the generator's cases, at the shapes of the GPU tests -----------------------------------------------------------
@pytest.mark.parametrize("k,t,starts,lm", [(5, 400, (0, 50, 120, 363), 37), (64, 200, (0, 50, 163), 37),
                                           (65, 200, (0, 50, 163), 37), (256, 200, (0, 50, 163), 37),
                                           (70, 300, (0, 100, 282), 18), (5, 2452, (0, 1, 3, 12, 52, 352), 1)])
def test_generator_yields_its_cases(k, t, starts, lm):
    rng = np.random.default_rng(k + t)
    ll = rng.normal(size=(t, k))
    inside = np.zeros(t, bool)
    for s in starts:
        inside[s:s + lm] = True
    masked = int(np.flatnonzero(inside)[5 % inside.sum()])
    ll[masked] = 0.0
    if lm == 1:                                  # (the sequences' first rows: the special rows lie anywhere)
        inside = None
    kw = dict(windows=[(s, lm) for s in starts], full_window=(starts[1], lm), masked_row=masked, inside=inside)
    a = make_sets(ll, k, np.random.default_rng(3), **kw)
    check_cases(a, k, **kw)
    assert np.all(a[np.arange(t), np.argmax(ll, axis=1)] | (a.sum(axis=1) == 1))
    c = clamp_sets(ll, a)
    assert np.array_equal(np.isneginf(c), ~a) and np.array_equal(c[a], ll[a])
    assert np.array_equal(unpack_state_sets(pack_state_sets(a), k), a)


# ---- the classes on the oracle engine --------------------------------------------------------------------------------
def _lliks(m, x):
    return R.lliks_niw(x, np.array([g.mu_mf for g in m.var_emit]), np.array([g.sigma_mf for g in m.var_emit]),
                       np.array([float(g.kappa_mf) for g in m.var_emit]), np.array([float(g.nu_mf) for g in m.var_emit]))


def _sets(m, x, lengths):
    off = offsets(lengths)
    wins = [(int(off[s]), int(lengths[s])) for s in range(len(lengths))]
    full = wins[-1] if len(wins) > 1 else (10, 6)
    a = make_sets(_lliks(m, x), K, np.random.default_rng(5), windows=wins, full_window=full)
    check_cases(a, K, windows=wins, full_window=full)
    return a


def _check_constrained(m, a):
    assert np.all(m.var_x[~a] == 0.0)                                     # exactly 0.0 at forbidden pairs
    np.testing.assert_allclose(np.where(a, m.var_x, 0.0).sum(axis=1), 1.0, rtol=0, atol=1e-12)
    assert np.array_equal(np.isneginf(m.lliks), ~a)


def _reference(m, x, a, lengths):
    ll = clamp_sets(_lliks(m, x), a)
    off = offsets(lengths)
    q, la, lZ = np.empty((len(x), K)), np.empty((len(x), K)), 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(len(lengths)):
            sl = slice(off[s], off[s + 1])
            la[sl] = R.forward_msgs(ll[sl], m.mod_init, m.mod_tran)
            q[sl] = R.posterior(la[sl], R.backward_msgs(ll[sl], m.mod_tran))
            lZ += R.local_lower_bound(la[sl])
    return q, la, lZ


def test_local_update_equals_forward_backward_on_clamped_lliks():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    a = _sets(m, seqs[0], (T,))
    m.set_state_sets(a)
    assert m._family() is None                   # no device family evaluates unclamped lliks
    m.local_update()
    q, la, lZ = _reference(m, seqs[0], a, (T,))
    np.testing.assert_allclose(m.var_x, q, rtol=1e-6, atol=1e-11)
    np.testing.assert_allclose(m.lalpha, la, rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(m._lZ, lZ, rtol=1e-8)
    _check_constrained(m, a)


def test_infer_on_an_array():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K, maxit=3)
    a = _sets(m, seqs[0], (T,))
    m.set_state_sets(a)
    m.infer()
    assert len(m.elbo_vec) == 3 and np.all(np.isfinite(m.elbo_vec))
    _check_constrained(m, a)


def test_infer_on_a_list_of_sequences():
    seqs, masks = class_data(LENGTHS, K=K, D=D)
    x = np.concatenate(seqs)
    m = build_model(hmmbatchcd, seqs, masks, OracleEngine(), K=K, maxit=3)
    a = _sets(m, x, LENGTHS)
    a[offsets(LENGTHS)[1]] = [False, True, True, False]          # the one-row sequence is constrained
    m.set_state_sets(cut(a, LENGTHS))
    m.infer()
    assert len(m.elbo_vec) == 3 and np.all(np.isfinite(m.elbo_vec))
    _check_constrained(m, a)
    first = m.var_x.copy()
    m2 = build_model(hmmbatchcd, seqs, masks, OracleEngine(), K=K, maxit=3)
    m2.set_state_sets(a)                                         # one concatenated array is taken as well
    m2.infer()
    assert np.array_equal(m2.var_x, first)


def test_singleton_sets_equal_labels_bit_for_bit():
    seqs, masks = class_data((T,), K=K, D=D)
    a = _sets(build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K), seqs[0], (T,))
    lab = np.where(a.sum(axis=1) < K, np.argmax(a, axis=1), -1).astype(np.int32)      # one state per constrained row
    single = np.ones((T, K), bool)
    rows = np.flatnonzero(lab >= 0)
    single[rows] = False
    single[rows, lab[rows]] = True
    assert np.array_equal(singleton_labels(single), lab)
    ms = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K, maxit=3)
    ms.set_state_sets(single)
    ms.infer()
    ml = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K, maxit=3)
    ml.set_labels(lab)
    ml.infer()
    for name in ("lliks", "lalpha", "lbeta", "var_x", "var_tran", "var_init"):
        assert np.array_equal(getattr(ms, name), getattr(ml, name)), name
    assert np.array_equal(ms.elbo_vec, ml.elbo_vec)


def test_the_later_of_sets_and_labels_stays():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    a = _sets(m, seqs[0], (T,))
    lab = np.full(T, -1, dtype=np.int32)
    lab[5] = int(np.argmax(_lliks(m, seqs[0])[5]))
    m.set_labels(lab)
    m.set_state_sets(a)
    assert m.labels is None and np.array_equal(m.state_sets, a)
    m.local_update()
    assert np.array_equal(np.isneginf(m.lliks), ~a)
    m.set_labels(lab)
    assert m.state_sets is None and np.array_equal(m.labels, lab)
    m.local_update()
    want = np.zeros((T, K), bool)
    want[5] = True
    want[5, lab[5]] = False
    assert np.array_equal(np.isneginf(m.lliks), want)
    m.set_state_sets(a)
    m.set_state_sets(None)                       # None removes only its own kind -- and labels were replaced
    assert m.state_sets is None and m.labels is None
    m.set_labels(lab)
    m.set_state_sets(None)
    assert np.array_equal(m.labels, lab)


def test_removing_the_sets_restores_the_free_result_exactly():
    seqs, masks = class_data((T,), K=K, D=D)
    a = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    a.local_update()
    b = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    b.set_state_sets(_sets(b, seqs[0], (T,)))
    b.local_update()
    assert not np.array_equal(a.var_x, b.var_x)
    b.set_state_sets(None)
    b.local_update()
    for name in ("lliks", "lalpha", "lbeta", "var_x"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name


def test_bad_sets_raise():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    with pytest.raises(ValueError, match="shape"):
        m.set_state_sets(np.ones((T - 1, K), bool))
    with pytest.raises(ValueError, match="shape"):
        m.set_state_sets(np.ones(T, bool))
    with pytest.raises(ValueError, match="5 columns, the model has K = 4"):
        m.set_state_sets(np.ones((T, K + 1), bool))
    bad = np.ones((T, K), bool)
    bad[7] = False
    bad[9] = False
    with pytest.raises(ValueError, match="row 7 allows no state"):
        m.set_state_sets(bad)
    with pytest.raises(ValueError, match="bool"):
        m.set_state_sets(np.ones((T, K)))
    assert m.state_sets is None
    ms = build_model(hmmbatchcd, *class_data(LENGTHS, K=K, D=D), OracleEngine(), K=K)
    with pytest.raises(ValueError, match="do not match the sequences"):
        ms.set_state_sets([np.ones((n, K), bool) for n in LENGTHS[::-1]])
    with pytest.raises(ValueError, match="columns"):
        ms.set_state_sets([np.ones((n, K - 1), bool) for n in LENGTHS])


def test_metaobs_class_refuses():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmsgd_metaobs, seqs[0], masks[0], OracleEngine(), K=K)
    with pytest.raises(NotImplementedError, match="do not take allowed-state sets"):
        m.set_state_sets(np.ones((T, K), bool))
    m.set_state_sets(None)
