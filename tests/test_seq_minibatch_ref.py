"""``hmmbatchsgd.VBHMM(seq_minibatch=M)`` on a list of sequences (host logic on the oracle engine, no GPU): SVI over
whole sequences -- M of the N sequences per iteration, their statistics times N / M, a Robbins-Monro step."""
import numpy as np
import pytest

from oracle.engine import OracleEngine
from pysvihmm_amd import hmmbatchsgd
from seq_minibatch_helpers import hand_loop_minibatch
from sequences_helpers import build_model, class_data, offsets

LENGTHS = (40, 1, 300, 17)          # those of test_sequences_ref.py
SEED = 12345


def _factors(emit):
    return [np.array([np.asarray(getattr(g, n), dtype=float) for g in emit])
            for n in ("mu_mf", "sigma_mf", "kappa_mf", "nu_mf")]


def test_minibatch_loop_matches_hand_written_loop():
    seqs, masks = class_data(LENGTHS)
    hmm = build_model(hmmbatchsgd, seqs, masks, OracleEngine(), maxit=4, seq_minibatch=2)
    assert hmm.seq_minibatch == 2 and hmm.batchfactor == 1.
    ref = hand_loop_minibatch(build_model(hmmbatchsgd, seqs, masks, OracleEngine()), seqs, masks, 4, 2, SEED)
    assert len({tuple(d) for d in ref[4]}) > 1             # (the iterations do not all draw the same pair)
    np.random.seed(SEED)
    hmm.infer()
    assert hmm.batchfactor == 2.0
    np.testing.assert_allclose(hmm.var_tran, ref[0], rtol=1e-9)
    np.testing.assert_allclose(hmm.var_init, ref[1], rtol=1e-9)
    for got, want in zip(_factors(hmm.var_emit), _factors(ref[2])):
        np.testing.assert_allclose(got, want, rtol=1e-9)
    assert len(hmm.elbo_vec) == 4
    np.testing.assert_allclose(hmm.elbo_vec, ref[3], rtol=1e-9)
    assert np.all(np.isnan(hmm.pred_logprob_mean)) and np.all(np.isnan(hmm.pred_logprob_std))
    # per-row attributes: all T rows under the final parameters, each sequence's first row a start from mod_init
    T = sum(LENGTHS)
    assert hmm.var_x.shape == hmm.lalpha.shape == hmm.lbeta.shape == hmm.lliks.shape == (T, 4)
    np.testing.assert_allclose(hmm.var_x.sum(1), 1.0, rtol=1e-12)
    off = offsets(LENGTHS)
    np.testing.assert_array_equal(hmm.lbeta[off[1:] - 1], 0.0)
    np.testing.assert_allclose(hmm.lalpha[off[:-1]], hmm.mod_init + hmm.lliks[off[:-1]], rtol=1e-12)
    assert hmm.pred_logprob() is not None


def test_a_seeded_run_is_reproducible():
    seqs, masks = class_data(LENGTHS)
    runs = []
    for _ in range(2):
        hmm = build_model(hmmbatchsgd, seqs, masks, OracleEngine(), maxit=3, seq_minibatch=3)
        np.random.seed(SEED)
        hmm.infer()
        runs.append(hmm)
    for n in ("var_tran", "var_init", "elbo_vec", "var_x"):
        assert np.array_equal(getattr(runs[0], n), getattr(runs[1], n)), n


def test_none_is_the_behaviour_without_the_keyword():
    seqs, masks = class_data(LENGTHS)
    a = build_model(hmmbatchsgd, seqs, masks, OracleEngine())
    b = build_model(hmmbatchsgd, seqs, masks, OracleEngine(), seq_minibatch=None)
    np.random.seed(SEED)
    a.infer()
    state = np.random.get_state()
    np.random.seed(SEED)
    b.infer()
    assert np.array_equal(state[1], np.random.get_state()[1])          # (no draw from the global stream)
    assert b.batchfactor == 1.
    for n in ("var_tran", "var_init", "elbo_vec", "pred_logprob_mean", "pred_logprob_std", "var_x", "lalpha",
              "lbeta", "lliks", "mod_init", "mod_tran"):
        assert np.array_equal(getattr(a, n), getattr(b, n), equal_nan=True), n
    for x, y in zip(_factors(a.var_emit), _factors(b.var_emit)):
        assert np.array_equal(x, y)
    # ... and on a bare array
    c = build_model(hmmbatchsgd, seqs[2], masks[2], OracleEngine(), maxit=2)
    d = build_model(hmmbatchsgd, seqs[2], masks[2], OracleEngine(), maxit=2, seq_minibatch=None)
    c.infer()
    d.infer()
    assert np.array_equal(c.var_tran, d.var_tran) and np.array_equal(c.elbo_vec, d.elbo_vec)


@pytest.mark.parametrize("what", ["zero", "too_many", "bare_array", "one_element_list", "fraction"])
def test_constructor_errors(what):
    seqs, masks = class_data(LENGTHS)
    obs, mask, m = seqs, masks, 2
    if what == "zero":
        m = 0
    elif what == "too_many":
        m = len(LENGTHS) + 1
    elif what == "bare_array":
        obs, mask = seqs[2], masks[2]
    elif what == "one_element_list":
        obs, mask = [seqs[2]], [masks[2]]
    else:
        m = 1.5
    with pytest.raises(RuntimeError, match="seq_minibatch"):
        build_model(hmmbatchsgd, obs, mask, OracleEngine(), seq_minibatch=m)
    # the bounds themselves are allowed
    if what in ("zero", "too_many"):
        for ok in (1, len(LENGTHS)):
            assert build_model(hmmbatchsgd, seqs, masks, OracleEngine(), seq_minibatch=ok).seq_minibatch == ok


def test_an_override_is_refused():
    seqs, masks = class_data(LENGTHS)

    class Own(hmmbatchsgd.VBHMM):
        def global_update(self, *a):
            return hmmbatchsgd.VBHMM.global_update(self, *a)

    import types
    with pytest.raises(RuntimeError, match="several sequences"):
        build_model(types.SimpleNamespace(VBHMM=Own), seqs, masks, OracleEngine(), maxit=1, seq_minibatch=2).infer()
    with pytest.raises(RuntimeError, match="several sequences"):
        build_model(hmmbatchsgd, seqs, masks, OracleEngine(), maxit=1, seq_minibatch=2).infer(fused=False)


@pytest.mark.parametrize("flags", [0, 1, 2])
def test_the_gpu_tests_niw_reference_is_the_oracle_engine_per_sequence(flags):
    """test_gpu_seq_minibatch.py takes its NIW reference from the C oracle's cached per-sequence posteriors and the
    oracle engine's packing arithmetic (``niw_sequence_results``): here it is held to ``OracleEngine.estep([off_s],
    len_s, flags)`` itself, sequence by sequence.  Two fp64 implementations of the same sums over at most 2311 rows:
    round-off of n eps = 2.6e-13 relative at the worst, so rtol = 1e-12 (absolute: that times the largest entry)."""
    from seq_minibatch_helpers import niw_sequence_results, oracle_sequence_results
    from sequences_helpers import LENGTHS as L11, niw_problem
    K, D = 5, 3
    pb = niw_problem(K, D, L11, 900 + K)
    oe = OracleEngine()
    oe.set_obs(pb["obs"], pb["mask"])
    oe.set_globals(pb["mod_init"], pb["ltran"])
    oe.set_emission_niw(pb["mu"], pb["sigma"], pb["kappa"], pb["nu"])
    want = oracle_sequence_results(oe, L11, flags)
    got = niw_sequence_results(K, D, L11, 900 + K, flags)
    assert len(got) == len(want) == len(L11)
    for (gb, glb, gq), (wb, wlb, wq) in zip(got, want):
        np.testing.assert_allclose(gb, wb, rtol=1e-12, atol=1e-12 * np.abs(wb).max())
        np.testing.assert_allclose(glb, wlb, rtol=1e-12)
        np.testing.assert_allclose(gq, wq, rtol=1e-12, atol=1e-14)


def test_make_param_dict_has_the_optional_key():
    d = hmmbatchsgd.VBHMM.make_param_dict(1, 2, 3)
    assert d["seq_minibatch"] is None
    assert hmmbatchsgd.VBHMM.make_param_dict(1, 2, 3, seq_minibatch=8)["seq_minibatch"] == 8
