"""``set_labels`` of the batch classes on the oracle engine (no GPU): the engine has no ``set_labels``, so the model
takes the host-lliks route and clamps the lliks itself.  Reference: ``oracle.ref_numpy``'s forward-backward on the
clamped lliks.  Tolerances: those tests/test_gpu_sequences.py holds the classes to against the oracle engine."""
import numpy as np
import pytest

from oracle import ref_numpy as R
from oracle.engine import OracleEngine
from pysvihmm_amd import hmmbatchcd, hmmsgd_metaobs
from labels_helpers import clamp, make_labels
from sequences_helpers import build_model, class_data, cut, offsets

K, D, T = 4, 2, 60
LENGTHS = (23, 1, 30, 6)


def _lliks(m, x):
    return R.lliks_niw(x, np.array([g.mu_mf for g in m.var_emit]), np.array([g.sigma_mf for g in m.var_emit]),
                       np.array([float(g.kappa_mf) for g in m.var_emit]), np.array([float(g.nu_mf) for g in m.var_emit]))


def _labels(m, x, lengths):
    off = offsets(lengths)
    wins = [(int(off[s]), int(lengths[s])) for s in range(len(lengths))]
    full = wins[-1] if len(wins) > 1 else (10, 6)           # a fully labelled sequence / stretch
    return make_labels(_lliks(m, x), K, np.random.default_rng(5), windows=wins, full_window=full)


def _reference(m, x, lab, lengths):
    """Per sequence: forward / backward / posterior of the clamped lliks under the model's psi-expectations."""
    ll = clamp(_lliks(m, x), lab)
    off = offsets(lengths)
    q, la, lZ = np.empty((len(x), K)), np.empty((len(x), K)), 0.0
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(len(lengths)):
            sl = slice(off[s], off[s + 1])
            la[sl] = R.forward_msgs(ll[sl], m.mod_init, m.mod_tran)
            q[sl] = R.posterior(la[sl], R.backward_msgs(ll[sl], m.mod_tran))
            lZ += R.local_lower_bound(la[sl])
    return ll, q, la, lZ


def _check(m, x, lab, lengths):
    ll, q, la, lZ = _reference(m, x, lab, lengths)
    np.testing.assert_allclose(m.var_x, q, rtol=1e-6, atol=1e-11)
    np.testing.assert_allclose(m.lalpha, la, rtol=1e-9, atol=1e-8)
    np.testing.assert_allclose(m._lZ, lZ, rtol=1e-8)
    assert np.array_equal(np.isneginf(m.lliks), np.isneginf(ll))
    rows = np.flatnonzero(lab >= 0)
    onehot = np.zeros((len(rows), K))
    onehot[np.arange(len(rows)), lab[rows]] = 1.0
    assert np.array_equal(m.var_x[rows] == 0.0, onehot == 0.0)            # exactly 0.0 at forbidden pairs
    np.testing.assert_allclose(m.var_x[rows], onehot, rtol=0, atol=1e-12)


def test_local_update_equals_forward_backward_on_clamped_lliks():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    lab = _labels(m, seqs[0], (T,))
    assert 0.2 < np.mean(lab >= 0) < 0.7 and np.any(lab == K - 1)
    m.set_labels(lab)
    assert m._family() is None                   # no device family evaluates unclamped lliks
    m.local_update()
    _check(m, seqs[0], lab, (T,))


def test_a_list_of_sequences_with_a_list_of_labels():
    seqs, masks = class_data(LENGTHS, K=K, D=D)
    x = np.concatenate(seqs)
    m = build_model(hmmbatchcd, seqs, masks, OracleEngine(), K=K)
    lab = _labels(m, x, LENGTHS)
    lab[offsets(LENGTHS)[1]] = 2                 # the one-row sequence is labelled
    m.set_labels(cut(lab, LENGTHS))
    m.local_update()
    _check(m, x, lab, LENGTHS)
    m.set_labels(lab)                            # one concatenated array is taken as well
    m.local_update()
    _check(m, x, lab, LENGTHS)


def test_removing_the_labels_restores_the_unlabelled_result_exactly():
    seqs, masks = class_data((T,), K=K, D=D)
    a = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    a.local_update()
    b = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    b.set_labels(_labels(b, seqs[0], (T,)))
    b.local_update()
    assert not np.array_equal(a.var_x, b.var_x)
    b.set_labels(None)
    b.local_update()
    for name in ("lliks", "lalpha", "lbeta", "var_x"):
        assert np.array_equal(getattr(a, name), getattr(b, name)), name
    assert a._lZ == b._lZ


def test_infer_runs_labelled_and_keeps_the_labelled_rows_one_hot():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K, maxit=3)
    lab = _labels(m, seqs[0], (T,))
    m.set_labels(lab)
    m.infer()
    assert len(m.elbo_vec) == 3 and np.all(np.isfinite(m.elbo_vec))
    rows = np.flatnonzero(lab >= 0)
    assert np.array_equal(np.argmax(m.var_x[rows], axis=1), lab[rows])


def test_metaobs_class_refuses():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmsgd_metaobs, seqs[0], masks[0], OracleEngine(), K=K)
    with pytest.raises(NotImplementedError, match="resident SVI loop and grow_windows do not take labels"):
        m.set_labels(np.full(T, -1))
    m.set_labels(None)


def test_bad_labels_raise():
    seqs, masks = class_data((T,), K=K, D=D)
    m = build_model(hmmbatchcd, seqs[0], masks[0], OracleEngine(), K=K)
    with pytest.raises(ValueError, match="shape"):
        m.set_labels(np.full(T - 1, -1))
    bad = np.full(T, -1)
    bad[7] = -2
    with pytest.raises(ValueError, match=r"labels\[7\] = -2"):
        m.set_labels(bad)
    bad[7] = K
    with pytest.raises(ValueError, match=r"labels\[7\] = 4"):
        m.set_labels(bad)
    with pytest.raises(ValueError, match="int-valued"):
        m.set_labels(np.full(T, 0.5))
    assert m.labels is None
    ms = build_model(hmmbatchcd, *class_data(LENGTHS, K=K, D=D), OracleEngine(), K=K)
    with pytest.raises(ValueError, match="do not match the sequences"):
        ms.set_labels([np.full(n, -1) for n in LENGTHS[::-1]])
