"""``viterbi()`` / ``ffbs_windows()`` of the batch classes on a LIST of sequences, on the NumPy decoding engine of
tests/decode_sequences_helpers.py (no GPU): every sequence is decoded on its own, from mod_init at its first
row; and the two new symbols at the places the C ABI is declared.  Fails before svihmm_viterbi_sequences /
svihmm_ffbs_sequences exist."""
import ctypes
import os
import re

import numpy as np
import pytest

from pysvihmm_amd import _lib, hmmbatchcd, hmmbatchsgd
from sequences_helpers import build_model, class_data, offsets
from tests.decode_sequences_helpers import DecodingOracle, check_paths_sequences, viterbi_sequences_numpy
from tests.ffbs_helpers import check_paths
from tests.viterbi_helpers import viterbi_numpy

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LENGTHS = (40, 1, 300, 17)
MODS = [("cd", hmmbatchcd), ("sgd", hmmbatchsgd)]
MASK_AS_NAN = 1


def test_symbols_declared_and_bound():
    src = open(os.path.join(REPO, "include", "svihmm.h")).read()
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"#define\s+SVIHMM_ABI_VERSION\s+3\b", code)
    for name, nargs in (("svihmm_viterbi_sequences", 4), ("svihmm_ffbs_sequences", 8)):
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
        assert name in _lib.SIGNATURES, name
        res, args = _lib.SIGNATURES[name]
        assert res is ctypes.c_int and len(args) == nargs
    assert _lib.SIGNATURES["svihmm_ffbs_sequences"][1][5] is ctypes.c_uint64
    # the header no longer sends the reader to a loop of single-sequence calls
    assert "decode them one by one" not in src


def _fitted(mod, obs, mask, maxit=3):
    hmm = build_model(mod, obs, mask, DecodingOracle(), maxit=maxit)
    hmm.infer()
    return hmm


@pytest.mark.parametrize("name,mod", MODS)
def test_viterbi_on_a_list(name, mod):
    seqs, masks = class_data(LENGTHS)
    hmm = _fitted(mod, seqs, masks)
    before = (hmm.var_tran.copy(), hmm.var_init.copy())
    zs, score = hmm.viterbi()
    assert isinstance(zs, list) and len(zs) == len(LENGTHS)
    assert [z.shape for z in zs] == [(n,) for n in LENGTHS] and all(z.dtype == np.int32 for z in zs)
    assert isinstance(score, np.ndarray) and score.shape == (len(LENGTHS),) and score.dtype == np.float64
    assert np.array_equal(hmm.var_tran, before[0]) and np.array_equal(hmm.var_init, before[1])
    # each sequence is the NumPy recursion on that sequence's lliks alone (masked rows: lliks 0)
    eng = hmm.engine
    ll = eng.loglik([0], hmm.T, MASK_AS_NAN)[0]
    off = offsets(LENGTHS)
    for s in range(len(LENGTHS)):
        zr, sr = viterbi_numpy(ll[off[s]:off[s + 1]], eng.mod_init, eng.ltran)
        np.testing.assert_array_equal(zs[s], zr)
        assert score[s] == sr
    # the joins matter: the one-chain decode of the same rows differs (asserted for this seed)
    z_chain, _ = viterbi_numpy(ll, eng.mod_init, eng.ltran)
    assert (np.concatenate(zs) != z_chain).any()


@pytest.mark.parametrize("name,mod", MODS)
def test_ffbs_windows_on_a_list(name, mod):
    seqs, masks = class_data(LENGTHS)
    hmm = _fitted(mod, seqs, masks)
    T, S = sum(LENGTHS), 3
    u = np.random.default_rng(12).random((S, T))
    zs = hmm.ffbs_windows(n_draws=S, uniforms=u)
    assert isinstance(zs, list) and [z.shape for z in zs] == [(S, n) for n in LENGTHS]
    assert all(z.dtype == np.int32 for z in zs)
    eng = hmm.engine                                     # (holds the filter's globals and the emission family)
    logA = np.log(hmm.var_tran + np.finfo(np.float64).eps)
    np.testing.assert_array_equal(eng.ltran, logA)
    ll = eng.loglik([0], T, 0)[0]
    off = offsets(LENGTHS)
    for s in range(len(LENGTHS)):
        la = eng._filter(ll[off[s]:off[s + 1]])
        assert check_paths(zs[s], la, logA, u[:, off[s]:off[s + 1]]) == 0
    # without uniforms: the engine's counter-based generator, reproducible through the seed
    a = hmm.ffbs_windows(n_draws=2, seed=5)
    b = hmm.ffbs_windows(n_draws=2, seed=5)
    assert all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name,mod", MODS)
def test_one_element_list_is_the_bare_array(name, mod):
    seqs, masks = class_data((358,))
    a = _fitted(mod, seqs[0].copy(), masks[0].copy())
    b = _fitted(mod, [seqs[0].copy()], [masks[0].copy()])
    za, sa = a.viterbi()
    zb, sb = b.viterbi()
    assert isinstance(zb, np.ndarray) and isinstance(sb, float)
    np.testing.assert_array_equal(za, zb)
    assert sa == sb
    u = np.random.default_rng(3).random((2, 1, 358))
    fa, fb = a.ffbs_windows(n_draws=2, uniforms=u), b.ffbs_windows(n_draws=2, uniforms=u)
    assert fb.shape == (2, 1, 358)
    np.testing.assert_array_equal(fa, fb)


def test_plain_array_returns_todays_tuple():
    seqs, masks = class_data((358,))
    hmm = _fitted(hmmbatchcd, seqs[0], masks[0])
    z, score = hmm.viterbi()
    assert z.shape == (358,) and z.dtype == np.int32 and isinstance(score, float)
    eng = hmm.engine
    zr, sr = viterbi_numpy(eng.loglik([0], 358, MASK_AS_NAN)[0], eng.mod_init, eng.ltran)
    np.testing.assert_array_equal(z, zr)
    assert score == sr
    f = hmm.ffbs_windows(n_draws=2, uniforms=np.random.default_rng(4).random((2, 1, 358)))
    assert f.shape == (2, 1, 358) and f.dtype == np.int32


def test_plugin_emission_goes_through_host_lliks():
    """An emission object without a device family: its lliks of the concatenated rows are uploaded as one
    [1, T, K] batch and decoded through the same call."""
    class Plug(object):
        def __init__(self, g):
            self.g = g

        def expected_log_likelihood(self, x):
            return self.g.expected_log_likelihood(x)

        def get_vlb(self):
            return 0.0

    seqs, masks = class_data(LENGTHS)
    hmm = _fitted(hmmbatchcd, seqs, masks)
    zs, score = hmm.viterbi()
    plug = hmmbatchcd.VBHMM(seqs, np.ones(4), np.ones((4, 4)), np.array([Plug(e) for e in hmm.var_emit]),
                            mask=masks, maxit=1, engine=DecodingOracle())
    plug.var_tran, plug.var_init = hmm.var_tran.copy(), hmm.var_init.copy()
    zp, sp = plug.viterbi()
    assert plug.engine._host_ll.shape == (1, sum(LENGTHS), 4)
    for a, b in zip(zs, zp):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_allclose(sp, score, rtol=1e-9)
    u = np.random.default_rng(8).random((2, sum(LENGTHS)))
    fp = plug.ffbs_windows(n_draws=2, uniforms=u)
    la = np.concatenate([plug.engine._filter(w) for w in
                         np.split(plug.engine._host_ll[0], offsets(LENGTHS)[1:-1])])
    assert check_paths_sequences(np.concatenate(fp, axis=1), la, plug.engine.ltran, u, offsets(LENGTHS)) == 0


def test_helper_drivers_cut_at_the_joins():
    rng = np.random.default_rng(0)
    K, lengths = 3, (4, 1, 6)
    off = offsets(lengths)
    ll = rng.normal(size=(11, K))
    mi, lt = np.log(rng.dirichlet(np.ones(K))), np.log(rng.dirichlet(np.ones(K), size=K))
    z, score = viterbi_sequences_numpy(ll, off, mi, lt)
    assert z.dtype == np.int32 and z.shape == (11,) and score.shape == (3,)
    assert z[4] == np.argmax(mi + ll[4]) and score[1] == (mi + ll[4]).max()
