"""Decoding all declared sequences in one call (svihmm_viterbi_sequences / svihmm_ffbs_sequences, ``viterbi()`` /
``ffbs_windows()`` of the batch classes on a list): per-sequence drivers of the NumPy statements in
viterbi_helpers.py / ffbs_helpers.py over ``seq_off``, and ``DecodingOracle``, the oracle engine with the two
calls (and the window decoders the classes use on a plain array) in NumPy, so the class layer runs without a
GPU.  Host-side only; a reference never sees more than one sequence at a time."""
import numpy as np

from oracle import ref_c
from oracle import ref_numpy as R
from oracle.engine import OracleEngine

from tests.ffbs_helpers import backward_sample, check_paths, near_boundary_steps
from tests.viterbi_helpers import viterbi_numpy

USE_HOST_LLIKS = 4


def offsets(lengths):
    off = np.zeros(len(lengths) + 1, dtype=np.int64)
    np.cumsum(lengths, out=off[1:])
    return off


def viterbi_sequences_numpy(ll, seq_off, mod_init, ltran):
    """``ll[T, K]`` of the concatenated rows -> (z int32[T], score float64[N]), each sequence on its own rows."""
    seq_off = np.asarray(seq_off)
    z = np.empty(int(seq_off[-1]), dtype=np.int32)
    score = np.empty(len(seq_off) - 1)
    for s in range(len(seq_off) - 1):
        a, b = int(seq_off[s]), int(seq_off[s + 1])
        z[a:b], score[s] = viterbi_numpy(ll[a:b], mod_init, ltran)
    return z, score


def check_paths_sequences(z, la, logA, u, seq_off):
    """``check_paths`` per sequence: z, u [S, T] (or [T]), la [T, K].  Returns the number of excused steps."""
    seq_off = np.asarray(seq_off)
    z, u = np.asarray(z), np.asarray(u)
    assert z.shape == u.shape and z.shape[-1] == la.shape[0] == int(seq_off[-1]), (z.shape, u.shape, la.shape)
    n = 0
    for s in range(len(seq_off) - 1):
        a, b = int(seq_off[s]), int(seq_off[s + 1])
        n += check_paths(z[..., a:b], la[a:b], logA, u[..., a:b])
    return n


def backward_sample_sequences(la, logA, u, seq_off):
    """NumPy paths z int32[S, T] from la [T, K] and u [S, T], each sequence sampled back from its own last row:
    ``ffbs_helpers.draw`` step by step, the S draws of a step side by side (the same elementwise operations and
    the same running sums in state order)."""
    seq_off = np.asarray(seq_off)
    S, K = u.shape[0], la.shape[1]
    z = np.empty(u.shape, dtype=np.int32)
    logAT = np.ascontiguousarray(np.asarray(logA, dtype=np.float64).T)
    for s in range(len(seq_off) - 1):
        a, b = int(seq_off[s]), int(seq_off[s + 1])
        for t in range(b - 1, a - 1, -1):
            lp = np.broadcast_to(la[t], (S, K)) if t == b - 1 else la[t] + logAT[z[:, t + 1]]
            c = np.cumsum(np.exp(lp - lp.max(axis=1, keepdims=True)), axis=1)
            hit = (u[:, t] * c[:, -1])[:, None] <= c
            z[:, t] = np.where(hit.any(axis=1), hit.argmax(axis=1), K - 1)
    return z


def near_boundary_sequences(z, la, logA, u, seq_off):
    seq_off = np.asarray(seq_off)
    n = 0
    for s in range(len(seq_off) - 1):
        a, b = int(seq_off[s]), int(seq_off[s + 1])
        n += near_boundary_steps(z[..., a:b], la[a:b], logA, u[..., a:b])[0]
    return n


def philox_uniforms(seed, S, T):
    """The device's own uniforms of svihmm_ffbs_sequences: Philox row ``s * T + r``, stream 0."""
    w = R.philox4x32_10(seed, np.arange(S * T, dtype=np.uint64), 0)
    return R._u53(w[0], w[1]).reshape(S, T)


class DecodingOracle(OracleEngine):
    """OracleEngine + the decoders in NumPy: ``viterbi`` / ``ffbs_windows`` on windows, ``set_sequences`` and
    ``viterbi_sequences`` / ``ffbs_sequences`` on the declared sequences (the HipEngine's signatures)."""
    name = "decoding-oracle"

    def set_obs(self, obs, mask=None):
        OracleEngine.set_obs(self, obs, mask)
        self.seq_off = None

    def set_sequences(self, lengths):
        self.seq_off = None if lengths is None or len(lengths) == 0 else offsets(np.asarray(lengths).ravel())
        if self.seq_off is not None and int(self.seq_off[-1]) != self.T:
            raise RuntimeError("svihmm_set_sequences failed: seq_off[N] must equal T")

    def _filter(self, ll):
        return ref_c.forward(np.ascontiguousarray(ll), self.mod_init, self.ltran)

    @staticmethod
    def _uniforms(uniforms, seed, shape):
        if uniforms is not None:
            return np.asarray(uniforms, dtype=np.float64).reshape(shape)
        n = int(np.prod(shape))
        w = R.philox4x32_10(int(seed), np.arange(n, dtype=np.uint64), 0)
        return R._u53(w[0], w[1]).reshape(shape)

    def viterbi(self, starts, Lm, flags=0, want_z=True):
        self._pre_mutate()
        st = np.asarray(starts, dtype=np.int64).ravel()
        ll = self._lls(st, int(Lm), flags, len(st))
        out = [viterbi_numpy(w, self.mod_init, self.ltran) for w in ll]
        z = np.stack([o[0] for o in out]) if want_z else None
        return z, np.array([o[1] for o in out])

    def ffbs_windows(self, starts, Lm, logA, n_draws=1, uniforms=None, seed=0, flags=0, want_lalpha=False):
        self._pre_mutate()
        st = np.asarray(starts, dtype=np.int64).ravel()
        B, Lm, S = len(st), int(Lm), int(n_draws)
        ll = self._lls(st, Lm, flags, B)
        la = np.stack([self._filter(w) for w in ll])
        u = self._uniforms(uniforms, seed, (S, B, Lm))
        z = np.stack([[backward_sample(la[b], logA, u[s, b]) for b in range(B)] for s in range(S)])
        return z, (la if want_lalpha else None)

    def _all_ll(self, flags):
        if self.seq_off is None:
            raise RuntimeError("no sequences declared: call svihmm_set_sequences first")
        if flags & USE_HOST_LLIKS:
            if self._host_ll is None or self._host_ll.shape[:2] != (1, self.T):
                raise RuntimeError("SVIHMM_USE_HOST_LLIKS without uploaded lliks of shape [1, T, K] (svihmm_set_lliks)")
            return self._host_ll[0]
        return self.loglik([0], self.T, flags)[0]

    def viterbi_sequences(self, flags=0, want_z=True):
        self._pre_mutate()
        z, score = viterbi_sequences_numpy(self._all_ll(flags), self.seq_off, self.mod_init, self.ltran)
        return (z if want_z else None), score

    def ffbs_sequences(self, logA, n_draws=1, uniforms=None, seed=0, flags=0, want_lalpha=False):
        self._pre_mutate()
        ll, so, S = self._all_ll(flags), self.seq_off, int(n_draws)
        la = np.concatenate([self._filter(ll[int(a):int(b)]) for a, b in zip(so[:-1], so[1:])])
        u = self._uniforms(uniforms, seed, (S, self.T))
        z = backward_sample_sequences(la, logA, u, so)
        return z, (la if want_lalpha else None)
