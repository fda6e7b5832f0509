"""HipEngine: thin object wrapper over the C ABI (one handle = one GPU).

This is the E-step "operator" the host classes call; it mirrors the steps of the
reference's ``local_update`` / ``intermediate_pars`` (hmmsgd_metaobs.py:487-519,
857-928) but on whole minibatches of windows at once.  Device handles never live
in a pickled ``__dict__`` (the reference pickles whole VBHMM objects,
cluster/run_cluster_simple.py:32-37).
"""
import collections
import ctypes as C

import numpy as np

from . import _lib as L


class PackedStats(object):
    """View of the packed statistics buffer
    ``[A_raw K*K | xbar K*D | neff K | S K*D*D | lb]``."""

    def __init__(self, buf, K, D):
        self.buf, self.K, self.D = buf, K, D
        o = 0
        self.A_raw = buf[o:o + K * K].reshape(K, K); o += K * K
        self.xbar = buf[o:o + K * D].reshape(K, D); o += K * D
        self.neff = buf[o:o + K]; o += K
        self.S = buf[o:o + K * D * D].reshape(K, D, D); o += K * D * D
        self.lb = buf[o:o + 1]

    @staticmethod
    def size(K, D):
        return K * K + K * D + K + K * D * D + 1


class PackedDiagStats(object):
    """View of the packed statistics of a diagonal-Gaussian E-step
    ``[A_raw K*K | xbar K*D | neff K | xsq K*D | lb]`` (xsq[k, d] = sum_t q[t,k] x[t,d]^2)."""

    def __init__(self, buf, K, D):
        self.buf, self.K, self.D = buf, K, D
        o = 0
        self.A_raw = buf[o:o + K * K].reshape(K, K); o += K * K
        self.xbar = buf[o:o + K * D].reshape(K, D); o += K * D
        self.neff = buf[o:o + K]; o += K
        self.xsq = buf[o:o + K * D].reshape(K, D); o += K * D
        self.lb = buf[o:o + 1]

    @staticmethod
    def size(K, D):
        return K * K + 2 * K * D + K + 1


class PackedCatStats(object):
    """View of the packed statistics of a Categorical-emission E-step
    ``[A_raw K*K | counts K*V | lb]`` (counts[k, v] = sum of var_x[t, k] over unmasked rows
    with symbol v)."""

    def __init__(self, buf, K, V):
        self.buf, self.K, self.V = buf, K, V
        self.A_raw = buf[:K * K].reshape(K, K)
        self.counts = buf[K * K:K * K + K * V].reshape(K, V)
        self.lb = buf[K * K + K * V:K * K + K * V + 1]

    @staticmethod
    def size(K, V):
        return K * K + K * V + 1


class PackedMCatStats(object):
    """View of the packed statistics of a multi-column Categorical E-step
    ``[A_raw K*K | counts K*F | lb]``, ``F = sum(Vs)``: ``flat`` is the whole ``[K, F]`` block and
    ``col_counts[d]`` the ``[K, V_d]`` view of column d (``col_counts[d][k, v]`` = sum of var_x[t, k]
    over unmasked rows whose entry d is present with symbol v)."""

    def __init__(self, buf, K, Vs):
        Vs = tuple(int(v) for v in Vs)
        F = sum(Vs)
        self.buf, self.K, self.Vs, self.F = buf, K, Vs, F
        self.A_raw = buf[:K * K].reshape(K, K)
        self.flat = buf[K * K:K * K + K * F].reshape(K, F)
        off = np.concatenate(([0], np.cumsum(Vs))).astype(int)
        self.col_counts = [self.flat[:, off[d]:off[d + 1]] for d in range(len(Vs))]
        self.lb = buf[K * K + K * F:K * K + K * F + 1]

    @staticmethod
    def size(K, Vs):
        return K * K + K * int(sum(Vs)) + 1


class PackedPoissonStats(object):
    """View of the packed statistics of a Poisson E-step ``[A_raw K*K | stat K*2D | lb]``,
    ``stat[k] = [sx[k] D | n[k] D]``: ``sx[k, d]`` = sum of var_x[t, k] * count and ``n[k, d]`` = sum of
    var_x[t, k], both over the unmasked rows whose entry d is present; ``flat`` is the whole ``[K, 2D]`` block."""

    def __init__(self, buf, K, D):
        self.buf, self.K, self.D = buf, K, D
        self.A_raw = buf[:K * K].reshape(K, K)
        self.flat = buf[K * K:K * K + 2 * K * D].reshape(K, 2 * D)
        self.sx = self.flat[:, :D]
        self.n = self.flat[:, D:]
        self.lb = buf[K * K + 2 * K * D:K * K + 2 * K * D + 1]

    @staticmethod
    def size(K, D):
        return K * K + 2 * K * D + 1


class PackedGaussTrackStats(object):
    """View of the packed statistics of an E-step under ``set_emission_pgauss``
    ``[A_raw K*K | stat K*3D | lb]``, ``stat[k] = [sxx[k] D | sx[k] D | n[k] D]``: sums of var_x[t, k] r r,
    var_x[t, k] r and var_x[t, k] with ``r = x - origin[d]``, over the unmasked rows whose entry d is present;
    ``flat`` is the whole ``[K, 3D]`` block, ``origin`` what the statistics were taken about."""

    def __init__(self, buf, K, D, origin=None):
        self.buf, self.K, self.D = buf, K, D
        self.origin = np.zeros(D) if origin is None else origin
        self.A_raw = buf[:K * K].reshape(K, K)
        self.flat = buf[K * K:K * K + 3 * K * D].reshape(K, 3 * D)
        self.sxx = self.flat[:, :D]
        self.sx = self.flat[:, D:2 * D]
        self.n = self.flat[:, 2 * D:]
        self.lb = buf[K * K + 3 * K * D:K * K + 3 * K * D + 1]

    @staticmethod
    def size(K, D):
        return K * K + 3 * K * D + 1


def _split_niw(blk, K, D):
    o1, o2 = K * D, K * D + K * D * D
    return blk[:o1].reshape(K, D), blk[o1:o2].reshape(K, D, D), blk[o2:o2 + K], blk[o2 + K:]


def _split_mcat(blk, K, Vs):
    off = np.concatenate(([0], np.cumsum(Vs))).astype(int)
    flat = blk.reshape(K, sum(Vs))
    return [np.ascontiguousarray(flat[:, off[d]:off[d + 1]]) for d in range(len(Vs))]


# One row per emission family (the names of hmmbase.FAMILIES): the view of its packed statistics and that view's
# ``size(K, shape)``; ``fields``: the view's attributes that hold its constructor's arguments after ``K``; ``block`` /
# ``split``: length of the resident SVI loop's factor block and its parts as ``svi_read_factors`` returns them, both of
# ``(K, shape)`` (None: the family has no resident loop).  ``shape`` is D, V or the tuple Vs, as the family counts.
FamilyStats = collections.namedtuple("FamilyStats", "stats size fields block split")
FAMILY_STATS = {
    "niw": FamilyStats(PackedStats, PackedStats.size, ("D",), lambda K, D: K * D + K * D * D + 2 * K, _split_niw),
    "diag": FamilyStats(PackedDiagStats, PackedDiagStats.size, ("D",), lambda K, D: 4 * K * D,
                        lambda blk, K, D: tuple(blk.reshape(4, K, D))),
    "cat": FamilyStats(PackedCatStats, PackedCatStats.size, ("V",), lambda K, V: K * V,
                       lambda blk, K, V: blk.reshape(K, V)),
    "mcat": FamilyStats(PackedMCatStats, PackedMCatStats.size, ("Vs",), lambda K, Vs: K * sum(Vs), _split_mcat),
    "poisson": FamilyStats(PackedPoissonStats, PackedPoissonStats.size, ("D",), lambda K, D: 2 * K * D,
                           lambda blk, K, D: tuple(blk.reshape(2, K, D))),
    "pgauss": FamilyStats(PackedGaussTrackStats, PackedGaussTrackStats.size, ("D", "origin"), None, None),
}


def rewrap_packed(st, buf):
    """A view of ``st``'s type and shape over another buffer (sums / multiples of packed statistics)."""
    fields = next((f.fields for f in FAMILY_STATS.values() if isinstance(st, f.stats)),
                  ("V",) if hasattr(st, "counts") else ("D",))      # (another engine's view: told by its attributes)
    return type(st)(buf, st.K, *[getattr(st, a) for a in fields])


class HipEngine(object):
    """E-step engine on one MI355X.  Raises RuntimeError when the HIP library or
    a GPU is unavailable (no fallback)."""

    name = "hip"

    def __init__(self, device=0, dtype="f64"):
        self._lib = L.load()
        h = C.c_void_p()
        L.check(self._lib.svihmm_create(int(device), C.byref(h)), "svihmm_create")
        self._h = h
        if dtype not in ("f64", "f32", np.float64, np.float32):
            raise RuntimeError("dtype must be 'f64' or 'f32'")
        if dtype in ("f32", np.float32):
            self.set_precision("f32")
        self.device = int(device)
        self.T = self.D = self.K = 0
        # the emission family in force: (name in FAMILY_STATS, what its statistics view takes after K); () for the two
        # Gaussian families, whose view takes the resident rows' D as it is when the statistics are wrapped
        self.family = ("niw", ())
        self._svi = None      # the resident SVI loop begun through this object: (family name, K, shape)
        self._comm = False
        self.seq_off = None   # offsets declared with set_sequences (every upload of rows removes them)

    # -- lifecycle ------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.svihmm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __getstate__(self):
        raise RuntimeError("HipEngine holds device memory and cannot be pickled; "
                           "VBHMM objects drop it in __getstate__")

    def sync(self):
        L.check(self._lib.svihmm_sync(self._h), "svihmm_sync")

    def set_precision(self, dtype):
        """'f64' (default) or 'f32': fp32 storage of the scaled messages + fp32 statistics GEMM on
        the E-step fast path (see include/svihmm.h); inputs and outputs stay float64."""
        mode = {"f64": L.F64, "f32": L.F32}[dtype]
        L.check(self._lib.svihmm_set_precision(self._h, mode), "svihmm_set_precision")

    def precision(self):
        """(mode, whether the last E-step batch ran in the fp32 format)."""
        m, u = C.c_int32(), C.c_int32()
        L.check(self._lib.svihmm_get_precision(self._h, C.byref(m), C.byref(u)), "svihmm_get_precision")
        return ("f32" if m.value == L.F32 else "f64"), bool(u.value)

    def on_next_mutation(self, callback):
        """Register a one-shot callback that runs before the next call that uploads parameters
        or overwrites the E-step intermediates (``lliks / lalpha / lbeta / var_x`` rows in HBM):
        a host object that fetches those rows lazily resolves them while they are still valid."""
        self._on_mutate = callback

    def _pre_mutate(self):
        cb, self._on_mutate = getattr(self, "_on_mutate", None), None
        if cb is not None:
            cb()

    # -- inputs ----------------------------------------------------------------------
    def set_obs(self, obs, mask=None):
        self._pre_mutate()
        obs = np.asarray(obs, dtype=np.float64)
        if obs.ndim == 1:
            obs = obs[:, None]
        obs = np.ascontiguousarray(obs)
        T, D = obs.shape
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
            if m.shape != (T,):
                raise RuntimeError("mask must have shape (T,)")
        L.check(self._lib.svihmm_set_obs(self._h, L.dptr(obs), T, D, L.u8ptr(m)), "svihmm_set_obs")
        self.T, self.D = T, D
        self.seq_off = None
        self._obs_owner = None        # whoever uploaded claims the resident copy afterwards

    def generate(self, tran, means, chols, T, seed=0):
        """Generate a synthetic sequence directly in HBM (reference ``gen_synthetic.generate_data``
        semantics; counter-based randomness, see ``include/svihmm.h``): it becomes the resident
        observation copy.  ``chols`` are lower Cholesky factors of the emission covariances."""
        self._pre_mutate()
        tran = L.as_f64(tran)
        K = tran.shape[0]
        cdf = np.cumsum(tran, axis=1)
        cdf = np.ascontiguousarray(cdf / cdf[:, -1:])
        means = L.as_f64(means)
        D = means.shape[1]
        chols = L.as_f64(chols, (K, D, D))
        L.check(self._lib.svihmm_generate(self._h, int(T), K, D, L.dptr(cdf), L.dptr(means), L.dptr(chols),
                                          int(seed) & 0xFFFFFFFFFFFFFFFF), "svihmm_generate")
        self.T, self.D = int(T), D
        self.seq_off = None
        self._obs_owner = None

    def read_generated(self, want_obs=True, want_sts=True):
        sts = np.empty(self.T, dtype=np.int32) if want_sts else None
        obs = np.empty((self.T, self.D)) if want_obs else None
        L.check(self._lib.svihmm_read_generated(
            self._h, None if sts is None else sts.ctypes.data_as(C.c_void_p), L.dptr(obs)),
            "svihmm_read_generated")
        return obs, sts

    def shift_obs(self, shift):
        """Move the centre the handle keeps the resident observations at by ``shift`` (a
        conditioning hint; results of every call stay in the caller's coordinates)."""
        self._pre_mutate()
        c = np.ascontiguousarray(shift, dtype=np.float64)
        if c.shape != (self.D,):
            raise RuntimeError("shift must have shape (D,)")
        L.check(self._lib.svihmm_shift_obs(self._h, L.dptr(c)), "svihmm_shift_obs")

    def get_shift(self):
        """The centre ``c`` of the resident copy (``obs_dev = obs - c``)."""
        c = np.empty(self.D)
        L.check(self._lib.svihmm_get_shift(self._h, L.dptr(c)), "svihmm_get_shift")
        return c

    def set_obs_blocks(self, blocks, T, D, mask=None):
        """Upload a sequence that arrives in row blocks (``gen_synthetic.read_data_mmap``,
        reference ``gen_synthetic.py:188-191``): ``blocks`` yields ``[n_i, D]`` arrays in
        order; rows beyond the last block keep whatever the allocation held."""
        self._pre_mutate()
        T, D = int(T), int(D)
        m = None
        if mask is not None:
            m = np.ascontiguousarray(np.asarray(mask).astype(np.uint8))
            if m.shape != (T,):
                raise RuntimeError("mask must have shape (T,)")
        L.check(self._lib.svihmm_alloc_obs(self._h, T, D, int(m is not None)), "svihmm_alloc_obs")
        self.T, self.D = T, D
        self.seq_off = None
        self._obs_owner = None
        row = 0
        for blk in blocks:
            blk = np.ascontiguousarray(np.asarray(blk, dtype=np.float64).reshape(-1, D))
            n = blk.shape[0]
            if n == 0:
                continue
            mp = None if m is None else m[row:row + n].ctypes.data_as(C.c_void_p)
            L.check(self._lib.svihmm_set_obs_rows(self._h, row, n, L.dptr(blk), mp), "svihmm_set_obs_rows")
            row += n
        return row

    def set_globals(self, mod_init, ltran):
        self._pre_mutate()
        ltran = L.as_f64(ltran)
        K = ltran.shape[0]
        mod_init = L.as_f64(mod_init, (K,))
        if ltran.shape != (K, K):
            raise RuntimeError("ltran must be square")
        L.check(self._lib.svihmm_set_globals(self._h, K, L.dptr(mod_init), L.dptr(ltran)),
                "svihmm_set_globals")
        self.K = K

    def set_emission_niw(self, mu, sigma, kappa, nu, check=True):
        """Upload the K NIW mean-field factors; the quadratic-form parameters are built on
        the device.  ``check=True`` waits for the factorisation so that a sigma that is
        not positive definite raises here; ``check=False`` returns immediately (the error
        then surfaces at the next synchronising call -- used in hot loops)."""
        self._pre_mutate()
        mu = L.as_f64(mu)
        K, D = mu.shape
        sigma = L.as_f64(sigma, (K, D, D))
        kappa = L.as_f64(kappa, (K,))
        nu = L.as_f64(nu, (K,))
        L.check(self._lib.svihmm_set_emission_niw(self._h, K, D, L.dptr(mu), L.dptr(sigma),
                                                  L.dptr(kappa), L.dptr(nu)),
                "svihmm_set_emission_niw")
        self.family = ("niw", ())
        if check:
            L.check(self._lib.svihmm_sync(self._h), "svihmm_set_emission_niw")

    def set_emission_diag(self, mu, nus, alphas, betas, check=True):
        """Upload K diagonal-covariance Gaussian factors (normal-inverse-gamma mean field per
        dimension, all arrays [K, D]); see ``svihmm_set_emission_diag``.  Statistics then come
        back as ``PackedDiagStats``."""
        self._pre_mutate()
        mu = L.as_f64(mu)
        K, D = mu.shape
        nus, alphas, betas = (L.as_f64(a, (K, D)) for a in (nus, alphas, betas))
        L.check(self._lib.svihmm_set_emission_diag(self._h, K, D, L.dptr(mu), L.dptr(nus), L.dptr(alphas),
                                                   L.dptr(betas)), "svihmm_set_emission_diag")
        self.family = ("diag", ())
        if check:
            L.check(self._lib.svihmm_sync(self._h), "svihmm_set_emission_diag")

    def set_emission_prior(self, mu0, sigma0):
        mu0 = L.as_f64(mu0)
        K, D = mu0.shape
        sigma0 = L.as_f64(sigma0, (K, D, D))
        L.check(self._lib.svihmm_set_emission_prior(self._h, K, D, L.dptr(mu0), L.dptr(sigma0)),
                "svihmm_set_emission_prior")

    def niw_vlb_terms(self, mu, sigma, kappa, nu):
        """(log det sigma_mf, tr(sigma_mf^-1 sigma_0), (mu_mf-mu_0)' sigma_mf^-1 (mu_mf-mu_0)), each
        [K], for the given NIW mean-field parameters (prior from set_emission_prior); does not
        disturb the E-step's parameter set."""
        mu = L.as_f64(mu)
        K, D = mu.shape
        sigma = L.as_f64(sigma, (K, D, D)); kappa = L.as_f64(kappa, (K,)); nu = L.as_f64(nu, (K,))
        out = np.empty((3, K))
        L.check(self._lib.svihmm_niw_vlb_terms(self._h, K, D, L.dptr(mu), L.dptr(sigma), L.dptr(kappa),
                                               L.dptr(nu), L.dptr(out)), "svihmm_niw_vlb_terms")
        return out[0], out[1], out[2]

    def set_lliks(self, lliks):
        self._pre_mutate()
        lliks = L.as_f64(lliks)
        B, Lm, K = lliks.shape
        L.check(self._lib.svihmm_set_lliks(self._h, L.dptr(lliks), B, Lm), "svihmm_set_lliks")
        self._host_ll_windows = B

    # -- compute -----------------------------------------------------------------------
    @staticmethod
    def _starts(starts):
        return np.ascontiguousarray(np.asarray(starts, dtype=np.int64).ravel())

    def loglik(self, starts, Lm, flags=0):
        self._pre_mutate()
        st = self._starts(starts)
        out = np.empty((len(st), Lm, self.K))
        L.check(self._lib.svihmm_loglik(self._h, L.i64ptr(st), len(st), int(Lm), int(flags),
                                        L.dptr(out)), "svihmm_loglik")
        return out

    def forward_backward(self, starts, Lm, flags=0, want=("lalpha", "lbeta", "var_x", "local_lb"),
                         B=None):
        self._pre_mutate()
        st = None if starts is None else self._starts(starts)
        B = len(st) if st is not None else int(B)
        self._rows = B * int(Lm)
        self._held = None if st is None else ("windows", st, int(Lm))
        res = {}
        bufs = {}
        for name in ("lalpha", "lbeta", "var_x"):
            bufs[name] = np.empty((B, Lm, self.K)) if name in want else None
        bufs["local_lb"] = np.empty(B) if "local_lb" in want else None
        L.check(self._lib.svihmm_forward_backward(
            self._h, L.i64ptr(st), B, int(Lm), int(flags), L.dptr(bufs["lalpha"]),
            L.dptr(bufs["lbeta"]), L.dptr(bufs["var_x"]), L.dptr(bufs["local_lb"])),
            "svihmm_forward_backward")
        for k, v in bufs.items():
            if v is not None:
                res[k] = v
        return res

    def estep(self, starts, Lm, flags=L.TRANS_WRAP, read=True, inner=None):
        """Whole-minibatch E-step -> PackedStats (or None with read=False: the
        statistics stay in HBM for allreduce()).  ``inner=(off, length)`` restricts
        the statistics to that segment of every window (buffered meta-observations)."""
        self._pre_mutate()
        st = self._starts(starts)
        out = np.empty(self._packed_len()) if read else None
        off, ln = (0, int(Lm)) if inner is None else (int(inner[0]), int(inner[1]))
        self._rows = len(st) * int(Lm)
        self._held = ("windows", st, int(Lm))
        L.check(self._lib.svihmm_estep_minibatch_ex(self._h, L.i64ptr(st), len(st), int(Lm),
                                                    off, ln, int(flags), L.dptr(out)),
                "svihmm_estep_minibatch")
        return self._wrap_packed(out) if read else None

    def suffstats(self, starts, Lm, var_x, flags=L.TRANS_WRAP, read=True):
        """Expected sufficient statistics of posteriors the caller supplies (no E-step):
        ``var_x[b, t]`` is the posterior of observation row ``starts[b] + t``, used as given.
        ``TRANS_WRAP``: the metaobs transition form (reference hmmsgd_metaobs.py:876-878),
        without it the batch form (hmmbatchcd.py:182-184).  Returns the view ``estep`` returns
        (``lb`` = 0), or None with read=False (statistics stay in HBM).  The intermediates of the
        last E-step are left as they were."""
        self._pre_mutate()
        st = self._starts(starts)
        Lm = int(Lm)
        if len(st) < 1 or Lm < 1:
            raise ValueError("suffstats: need at least one window of positive length")
        q = np.asarray(var_x, dtype=np.float64)
        if q.shape != (len(st), Lm, self.K):
            raise ValueError("suffstats: var_x has shape %s, expected %s"
                             % (q.shape, (len(st), Lm, self.K)))
        q = np.ascontiguousarray(q)
        out = np.empty(self._packed_len()) if read else None
        L.check(self._lib.svihmm_suffstats(self._h, L.i64ptr(st), len(st), Lm, int(flags), L.dptr(q),
                                           L.dptr(out)), "svihmm_suffstats")
        return self._wrap_packed(out) if read else None

    def set_sequences(self, lengths):
        """Declare the resident rows as consecutive independent sequences of the given lengths
        (``svihmm_set_sequences``; their sum must be ``T``).  ``None`` / ``()`` removes the declaration,
        as every upload of new rows does.  While it is in force, windows that hold rows of two
        sequences are rejected by every call that takes windows."""
        n = 0 if lengths is None else len(lengths)
        if n == 0:
            L.check(self._lib.svihmm_set_sequences(self._h, None, 0), "svihmm_set_sequences")
            self.seq_off = None
            return
        off = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(np.asarray(lengths, dtype=np.int64).ravel(), out=off[1:])
        self.set_sequence_offsets(off)

    def set_sequence_offsets(self, seq_off):
        """``set_sequences`` from the ``N + 1`` offsets themselves (``seq_off[0] = 0 .. seq_off[N] = T``)."""
        off = np.ascontiguousarray(np.asarray(seq_off, dtype=np.int64).ravel())
        if len(off) < 2:
            raise RuntimeError("set_sequence_offsets: need at least two offsets")
        L.check(self._lib.svihmm_set_sequences(self._h, L.i64ptr(off), len(off) - 1), "svihmm_set_sequences")
        self.seq_off = off

    def set_labels(self, labels):
        """Known states of the resident rows (``svihmm_set_labels``): an int-valued array of length ``T``,
        ``-1`` where the row is free, the state index where it is known.  ``None`` removes the labels, as every
        upload of new rows does.  While they are in force every E-step and decoder on the device sees
        ``-inf`` lliks at a labelled row's other states; the resident SVI loops, ``grow_windows`` and
        ``pred_logprob`` refuse."""
        self._pre_mutate()
        if labels is None:
            L.check(self._lib.svihmm_set_labels(self._h, None), "svihmm_set_labels")
            return
        a = np.asarray(labels)
        if a.ndim != 1 or a.shape[0] != getattr(self, "T", 0):
            raise RuntimeError("set_labels: labels must have shape (T,) = (%d,), got %s"
                               % (getattr(self, "T", 0), a.shape))
        if not (np.issubdtype(a.dtype, np.integer) or np.all(a == np.rint(a))):
            raise RuntimeError("set_labels: labels must be int-valued")
        if a.size and (a.min() < -(2 ** 31) or a.max() >= 2 ** 31):
            raise RuntimeError("set_labels: labels must fit int32")
        a = np.ascontiguousarray(a.astype(np.int32))
        L.check(self._lib.svihmm_set_labels(self._h, a.ctypes.data_as(C.POINTER(C.c_int32))), "svihmm_set_labels")

    def set_state_sets(self, allowed, K=None):
        """Allowed-state sets of the resident rows (``svihmm_set_state_sets``): a bool array ``[T, K]``, True where
        state ``k`` is allowed at row ``t`` (a row of all True is free), or the packed ``uint64 [T, W]`` of
        ``util.pack_state_sets`` together with ``K=``.  ``None`` removes the sets, as every upload of new rows does.
        Sets and labels are alternatives: setting one kind removes the other.  While sets are in force every E-step
        and decoder on the device sees ``-inf`` lliks at the states a row does not allow; the resident SVI loops,
        ``grow_windows`` and ``pred_logprob`` refuse.  The library refuses a row that allows no state, a padding bit
        at or beyond ``K`` and ``K`` outside ``[1, 256]``, whatever was in force staying in force."""
        from .util import pack_state_sets
        self._pre_mutate()
        if allowed is None:
            L.check(self._lib.svihmm_set_state_sets(self._h, None, 0), "svihmm_set_state_sets")
            return
        a = np.asarray(allowed)
        T = getattr(self, "T", 0)
        if a.dtype == np.uint64:
            if K is None:
                raise RuntimeError("set_state_sets: packed uint64 sets need K=")
            K = int(K)
            if a.ndim != 2 or a.shape[1] != (K + 63) // 64:
                raise RuntimeError("set_state_sets: packed sets for K = %d must have shape (T, %d), got %s"
                                   % (K, (K + 63) // 64, a.shape))
        elif a.dtype == np.bool_:
            if a.ndim != 2 or a.shape[1] < 1:
                raise RuntimeError("set_state_sets: allowed must have shape (T, K), got %s" % (a.shape,))
            if K is not None and int(K) != a.shape[1]:
                raise RuntimeError("set_state_sets: K = %d, allowed has %d columns" % (int(K), a.shape[1]))
            K = a.shape[1]
            if 1 <= K <= 256:                   # (outside it the library refuses before it reads the array)
                a = pack_state_sets(a)
            else:
                a = np.zeros((a.shape[0], (K + 63) // 64), dtype=np.uint64)
        else:
            raise RuntimeError("set_state_sets: allowed must be a bool [T, K] array or packed uint64 [T, W] with "
                               "K=, got dtype %s" % a.dtype)
        if T and a.shape[0] != T:               # (no rows resident: the library says so)
            raise RuntimeError("set_state_sets: allowed must have T = %d rows, got %d" % (T, a.shape[0]))
        a = np.ascontiguousarray(a)
        L.check(self._lib.svihmm_set_state_sets(self._h, a.ctypes.data_as(C.POINTER(C.c_uint64)), K),
                "svihmm_set_state_sets")

    def estep_sequences(self, flags=0, read=True):
        """Whole E-step of all declared sequences in one device call (``svihmm_estep_sequences``):
        ``(stats, seq_lb[N], q0[K])`` -- ``stats`` as ``estep`` wraps them (None with read=False: they
        stay in HBM for ``allreduce_packed``), ``A_raw`` in the batch form summed over the sequences
        (``TRANS_WRAP``: plus each sequence's own wrap pair), ``lb = seq_lb.sum()``, ``q0`` the sum of
        the sequences' first posterior rows.  Afterwards ``var_x`` of all T rows is readable
        (``read_rows("var_x", ..)``, ``read_intermediate("var_x", 1, T)``, ``state_argmax``)."""
        self._pre_mutate()
        off = getattr(self, "seq_off", None)
        n = 0 if off is None else len(off) - 1      # (none declared: the library says so)
        out = np.empty(self._packed_len()) if read else None
        seq_lb = np.empty(max(n, 1))
        q0 = np.empty(max(self.K, 1))
        L.check(self._lib.svihmm_estep_sequences(self._h, int(flags), L.dptr(out), L.dptr(seq_lb), L.dptr(q0)),
                "svihmm_estep_sequences")
        self._rows = self.T
        self._held = ("sequences",)
        return (self._wrap_packed(out) if read else None), seq_lb[:n], q0[:self.K]

    def estep_sequence_subset(self, idx, flags=0, read=True):
        """E-step of a minibatch of whole sequences in one device call (``svihmm_estep_sequence_subset``):
        ``idx`` lists declared sequences (any integer sequence, any order; a repeated entry counts once per
        occurrence).  Returns ``(stats, seq_lb[M], q0[K])`` as ``estep_sequences`` does, restricted to the
        listed sequences, ``seq_lb`` in the order of ``idx``.  The cost follows the listed rows ``R``.
        Afterwards ``var_x`` of those ``R`` rows, in the order of ``idx``, is readable
        (``read_rows("var_x", 0, R)``, ``state_argmax``)."""
        self._pre_mutate()
        ix = np.ascontiguousarray(np.asarray(idx).ravel(), dtype=np.int32)
        if len(ix) < 1:
            raise RuntimeError("estep_sequence_subset: idx is empty (at least one sequence must be listed)")
        if not np.array_equal(ix, np.asarray(idx).ravel()):
            raise RuntimeError("estep_sequence_subset: idx must hold integers that fit 32 bits")
        out = np.empty(self._packed_len()) if read else None
        seq_lb = np.empty(len(ix))
        q0 = np.empty(max(self.K, 1))
        L.check(self._lib.svihmm_estep_sequence_subset(self._h, ix.ctypes.data_as(C.POINTER(C.c_int32)), len(ix),
                                                       int(flags), L.dptr(out), L.dptr(seq_lb), L.dptr(q0)),
                "svihmm_estep_sequence_subset")
        off = self.seq_off
        self._rows = int((off[ix + 1] - off[ix]).sum())
        self._held = ("subset", ix)
        return (self._wrap_packed(out) if read else None), seq_lb, q0[:self.K]

    def _stats_args(self):
        name, args = self.family
        return FAMILY_STATS[name], (self.K,) + (args or (self.D,))

    def _packed_len(self):
        fam, args = self._stats_args()
        return fam.size(*args[:2])

    def _wrap_packed(self, buf):
        fam, args = self._stats_args()
        return fam.stats(buf, *args)

    def set_emission_cat(self, logp):
        """Categorical emissions: ``logp[k, v] = E_q log theta_k[v]`` (obs = symbol indices)."""
        self._pre_mutate()
        logp = L.as_f64(logp)
        K, V = logp.shape
        L.check(self._lib.svihmm_set_emission_cat(self._h, K, V, L.dptr(logp)), "svihmm_set_emission_cat")
        self.family = ("cat", (V,))

    def set_emission_mcat(self, tables):
        """Multi-column Categorical emissions (``svihmm_set_emission_mcat``): ``tables`` is a list of D
        arrays, ``tables[d][k, v] = E_q log theta_{k,d}[v]``; obs is ``[T, D]`` symbol indices.
        Statistics then come back as ``PackedMCatStats``."""
        self._pre_mutate()
        tabs = [L.as_f64(t) for t in tables]
        if len(tabs) < 1 or any(t.ndim != 2 or t.shape[0] != tabs[0].shape[0] for t in tabs):
            raise RuntimeError("set_emission_mcat: tables must be a non-empty list of [K, V_d] arrays")
        K = tabs[0].shape[0]
        Vs = np.ascontiguousarray([t.shape[1] for t in tabs], dtype=np.int32)
        logp = np.ascontiguousarray(np.concatenate(tabs, axis=1))
        L.check(self._lib.svihmm_set_emission_mcat(self._h, K, len(tabs), Vs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                   L.dptr(logp)), "svihmm_set_emission_mcat")
        self.family = ("mcat", (tuple(int(v) for v in Vs),))

    def set_emission_poisson(self, elog, erate, max_count):
        """Poisson count emissions (``svihmm_set_emission_poisson``): ``elog[k, d] = psi(a) - log(b)`` and
        ``erate[k, d] = a / b`` of the Gamma factors; obs is ``[T, D]`` counts, an entry present when
        ``0 <= x < max_count + 1``.  The ``gammaln(c + 1)`` table is built once per ``max_count``.
        Statistics then come back as ``PackedPoissonStats``."""
        self._pre_mutate()
        elog, erate = L.as_f64(elog), L.as_f64(erate)
        if elog.ndim != 2 or erate.shape != elog.shape:
            raise RuntimeError("set_emission_poisson: elog and erate must be [K, D] arrays of one shape")
        C_ = int(max_count)
        if not 0 <= C_ <= L.POISSON_MAX_COUNT:
            raise RuntimeError("set_emission_poisson: max_count = %d outside [0, %d]" % (C_, L.POISSON_MAX_COUNT))
        if getattr(self, "_logfact_C", None) != C_:
            from scipy.special import gammaln
            self._logfact = np.ascontiguousarray(gammaln(np.arange(C_ + 1, dtype=np.float64) + 1.0))
            self._logfact_C = C_
        K, D = elog.shape
        L.check(self._lib.svihmm_set_emission_poisson(self._h, K, D, L.dptr(elog), L.dptr(erate),
                                                      L.dptr(self._logfact), C_), "svihmm_set_emission_poisson")
        self.family = ("poisson", (D,))

    def set_emission_pgauss(self, mu, hprec, cst, origin=None):
        """Gaussian tracks with missing entries (``svihmm_set_emission_pgauss``): ``mu[k, d]``,
        ``hprec[k, d] = -0.5 alphas / betas`` and ``cst[k, d] = -0.5 / nus - 0.5 (log betas - psi(alphas)) -
        0.5 log 2 pi`` of the normal-inverse-gamma factors; obs is ``[T, D]``, an entry present when
        ``-1e150 < x < 1e150``.  ``origin[d]`` (default zeros) is what the statistics are taken about; they then
        come back as ``PackedGaussTrackStats``."""
        self._pre_mutate()
        mu, hprec, cst = L.as_f64(mu), L.as_f64(hprec), L.as_f64(cst)
        if mu.ndim != 2 or hprec.shape != mu.shape or cst.shape != mu.shape:
            raise RuntimeError("set_emission_pgauss: mu, hprec and cst must be [K, D] arrays of one shape")
        K, D = mu.shape
        origin = np.zeros(D) if origin is None else np.array(L.as_f64(origin)).ravel()
        if origin.shape != (D,):
            raise RuntimeError("set_emission_pgauss: origin must have one entry per column")
        L.check(self._lib.svihmm_set_emission_pgauss(self._h, K, D, L.dptr(mu), L.dptr(hprec), L.dptr(cst),
                                                     L.dptr(origin)), "svihmm_set_emission_pgauss")
        self.family = ("pgauss", (D, origin))

    def pred_logprob(self, starts, Lm, flags=L.MASK_AS_NAN):
        """Mean predictive log-probability of the masked rows of the windows and their number
        (reference pred_logprob / pred_logprob_full); ``(None, 0)`` when nothing is masked."""
        self._pre_mutate()
        st = self._starts(starts)
        self._rows = len(st) * int(Lm)
        out = np.empty(2)
        L.check(self._lib.svihmm_pred_logprob(self._h, L.i64ptr(st), len(st), int(Lm), int(flags),
                                              L.dptr(out)), "svihmm_pred_logprob")
        n = int(out[1])
        return (float(out[0]) if n > 0 else None), n

    def heldout_rows(self, want_lp=False):
        """Held-out log-probability of the masked rows of the posterior batch the last E-step-type call left
        (``svihmm_heldout_rows``; ``forward_backward``, ``estep``, ``estep_sequences``, ``estep_sequence_subset``),
        every emission family, without another E-step: ``(mean or None, count)``, with ``want_lp`` also
        ``lp[nrows]`` in batch-row order (NaN for the rows that are not masked).  The E-step is expected to have
        run with ``MASK_AS_NAN``."""
        out = np.empty(2)
        lp = np.empty(max(int(getattr(self, "_rows", 0)), 1)) if want_lp else None
        L.check(self._lib.svihmm_heldout_rows(self._h, L.dptr(out), L.dptr(lp)), "svihmm_heldout_rows")
        n = int(out[1])
        res = ((float(out[0]) if n > 0 else None), n)
        return res + (lp[:int(self._rows)],) if want_lp else res

    def _batch_rows_of(self, rows):
        """Resident row numbers -> (batch rows, index of the entry each came from) under the last E-step's map."""
        held = getattr(self, "_held", None)
        if held is None:
            raise RuntimeError("heldout_entries: no E-step batch of resident rows is known to this engine "
                               "(forward_backward with starts, estep, estep_sequences, estep_sequence_subset)")
        if held[0] == "sequences":
            return rows, np.arange(len(rows), dtype=np.int64)

        def expand(lo, hi, what):
            # entry e owns positions lo[e] .. hi[e] - 1 of a sorted table: (e, position) of every pair
            cnt = hi - lo
            if len(cnt) and cnt.min() < 1:
                bad = int(np.flatnonzero(cnt < 1)[0])
                raise ValueError("heldout_entries: resident row %d (entry %d) lies in no %s of the batch held"
                                 % (rows[bad], bad, what))
            e = np.repeat(np.arange(len(lo), dtype=np.int64), cnt)
            first = np.cumsum(cnt) - cnt
            return e, np.arange(int(cnt.sum()), dtype=np.int64) - np.repeat(first, cnt) + np.repeat(lo, cnt)

        if held[0] == "windows":
            # every occurrence: window b holds resident row r at batch row b * Lm + (r - st[b]); the windows whose
            # start lies in (r - Lm, r], found in the sorted starts, listed per entry in ascending b
            st, Lm = held[1], held[2]
            order = np.argsort(st, kind="stable")
            ss = st[order]
            e, p = expand(np.searchsorted(ss, rows - Lm, side="right"), np.searchsorted(ss, rows, side="right"), "window")
            b = order[p]
            o = np.lexsort((b, e))
            e, b = e[o], b[o]
            return b * Lm + (rows[e] - st[b]), e
        # a subset: the declared sequence of every row, then its positions in idx (ascending), in the gathered order
        ix, off = held[1].astype(np.int64), self.seq_off
        s = np.searchsorted(off, rows, side="right") - 1
        s[(rows < 0) | (rows >= off[-1])] = -1
        order = np.argsort(ix, kind="stable")
        si = ix[order]
        e, p = expand(np.searchsorted(si, s, side="left"), np.searchsorted(si, s, side="right"), "listed sequence")
        m = order[p]
        dst = np.cumsum(off[ix + 1] - off[ix]) - (off[ix + 1] - off[ix])
        return dst[m] + (rows[e] - off[ix[m]]), e

    def heldout_entries(self, rows, cols, vals, resident=True, want_lp=False):
        """Entry-wise held-out log-probability (``svihmm_heldout_entries``; the multi-column Categorical, Poisson and
        Gaussian-tracks families): entry ``e`` scores value ``vals[e]`` of column ``cols[e]`` against the posterior row
        ``rows[e]`` of the batch the last E-step-type call left.  ``resident=True``: ``rows`` are resident row
        numbers, mapped to batch rows from the last call -- after a window batch to every occurrence in the
        windows (a row in no window raises ``ValueError``), after ``estep_sequences`` unchanged, after
        ``estep_sequence_subset`` to its positions in the gathered order; ``resident=False``: batch rows as they
        are.  Returns ``(mean or None, count)``; with ``want_lp`` also ``lp``, one value per entry passed to the
        library (NaN for entries whose value is not present under the family's rule) and, when ``resident``
        mapped them, ``src`` -- the index into ``rows`` each came from."""
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).ravel())
        c = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).ravel())
        v = np.ascontiguousarray(np.asarray(vals, dtype=np.float64).ravel())
        if not (len(r) == len(c) == len(v)):
            raise ValueError("heldout_entries: rows, cols and vals must have one length")
        src = None
        if resident:
            r, src = self._batch_rows_of(r)
            r = np.ascontiguousarray(r, dtype=np.int64)
            c, v = np.ascontiguousarray(c[src]), np.ascontiguousarray(v[src])
        n = len(r)
        out = np.empty(2)
        lp = np.empty(max(n, 1)) if want_lp else None
        L.check(self._lib.svihmm_heldout_entries(self._h, n, L.i64ptr(r) if n else None,
                                                 c.ctypes.data_as(C.POINTER(C.c_int32)) if n else None,
                                                 L.dptr(v) if n else None, L.dptr(out), L.dptr(lp)),
                "svihmm_heldout_entries")
        cnt = int(out[1])
        res = ((float(out[0]) if cnt > 0 else None), cnt)
        if not want_lp:
            return res
        return res + (lp[:n],) + ((src,) if resident else ())

    def _batch_row_exists(self, g):
        """Whether the library hands out row ``g`` of ``var_x`` (``svihmm_read_rows``; a row at or past the batch's
        ``lastB * lastLm`` rows is refused by a host-side check there, nothing runs)."""
        return self._lib.svihmm_read_rows(self._h, 3, int(g), 1, L.dptr(np.empty(max(self.K, 1)))) == 0

    def posterior_expect(self, table):
        """Posterior expectation of a per-state table over the posterior batch the last E-step-type call left
        (``svihmm_posterior_expect``; ``forward_backward``, ``estep``, ``estep_sequences``, ``estep_sequence_subset``):
        ``out[g, f] = sum_k var_x[g, k] table[k, f]`` for every batch row ``g``, ``[nrows, F]``, on the device without
        another E-step and without reading ``var_x`` back.  ``table`` is ``[K, F]`` float64 (``[K]`` counts as
        ``F = 1``), any finite values: no emission family is involved."""
        t = L.as_state_table(table, self.K, "posterior_expect")
        n = int(getattr(self, "_rows", 0))
        # the library writes lastB * lastLm rows: no call before it is known that they fit the buffer
        if self._batch_row_exists(n):
            raise RuntimeError("posterior_expect: the posterior batch held has more than the %d rows this engine "
                               "counted at its last E-step-type call" % n)
        out = np.empty((max(n, 1), t.shape[1]))
        L.check(self._lib.svihmm_posterior_expect(self._h, t.shape[1], L.dptr(t), L.dptr(out)),
                "svihmm_posterior_expect")
        if n > 0 and not self._batch_row_exists(n - 1):
            raise RuntimeError("posterior_expect: the posterior batch held has fewer than the %d rows this engine "
                               "counted at its last E-step-type call" % n)
        return out[:n]

    def posterior_expect_entries(self, table, rows, cols):
        """``out[e] = sum_k var_x[rows[e], k] table[k, cols[e]]`` for a sparse list of (batch row, table column) pairs
        (``svihmm_posterior_expect_entries``), ``[n]``: ``k`` ascending, every product and sum rounded on its own, so
        a NumPy loop restates it bit for bit.  ``rows`` are batch rows (the rows ``read_rows("var_x")`` numbers);
        duplicates are allowed, an empty list launches nothing."""
        t = L.as_state_table(table, self.K, "posterior_expect_entries")
        r = np.ascontiguousarray(np.asarray(rows, dtype=np.int64).ravel())
        c = np.ascontiguousarray(np.asarray(cols, dtype=np.int32).ravel())
        if len(r) != len(c):
            raise ValueError("posterior_expect_entries: rows and cols must have one length")
        n = len(r)
        out = np.empty(max(n, 1))
        L.check(self._lib.svihmm_posterior_expect_entries(
            self._h, t.shape[1], L.dptr(t), n, L.i64ptr(r) if n else None,
            c.ctypes.data_as(C.POINTER(C.c_int32)) if n else None, L.dptr(out)), "svihmm_posterior_expect_entries")
        return out[:n]

    def state_argmax(self, true_sts=None, want_z=True):
        """``np.argmax(var_x, axis=1)`` over the rows of the last E-step (window-major) and, with
        labels, the count matrix ``DM[pred, true]`` of ``util.munkres_match`` (reference
        ``hmmbase.py:346-355``, ``util.py:236-277``) -- decoded on the device, so only the
        int32 labels cross the bus.  Returns ``(z or None, DM or None)``."""
        n = getattr(self, "_rows", 0)
        if n <= 0:
            raise RuntimeError("state_argmax: no E-step has run on this engine")
        z = np.empty(n, dtype=np.int32) if want_z else None
        ts = conf = None
        if true_sts is not None:
            ts = np.ascontiguousarray(np.asarray(true_sts).ravel(), dtype=np.int32)
            if ts.size != n:
                raise ValueError("true_sts has %d labels for %d decoded rows" % (ts.size, n))
            conf = np.zeros((self.K, self.K), dtype=np.int64)
        vp = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        L.check(self._lib.svihmm_state_argmax(self._h, vp(ts), vp(z), vp(conf)), "svihmm_state_argmax")
        return z, conf

    def viterbi(self, starts, Lm, flags=0, want_z=True):
        """Viterbi / MAP state path of every window under the globals and the emission family
        currently set (``svihmm_viterbi``): ``(z int32[B, Lm], score float64[B])`` with
        ``score[b] = max_z log p(z, x_window)`` in the expectations' log domain.  The lliks are those
        ``loglik(starts, Lm, flags)`` returns; with ``USE_HOST_LLIKS`` the batch uploaded by
        ``set_lliks`` is decoded (``starts`` then only gives the number of windows).  Given the same
        lliks the result is bit-identical to the NumPy recursion stated in ``include/svihmm.h``.
        ``want_z=False`` skips the backtrack and returns ``(None, score)``."""
        self._pre_mutate()
        st = self._starts(starts)
        Lm = int(Lm)
        z = np.empty((len(st), max(Lm, 0)), dtype=np.int32) if want_z else None
        score = np.empty(len(st))
        L.check(self._lib.svihmm_viterbi(self._h, L.i64ptr(st), len(st), Lm, int(flags),
                                         None if z is None else z.ctypes.data_as(C.c_void_p),
                                         L.dptr(score)), "svihmm_viterbi")
        return z, score

    def viterbi_sequences(self, flags=0, want_z=True):
        """MAP state path of every declared sequence (``set_sequences``) in one device call
        (``svihmm_viterbi_sequences``): ``(z int32[T] or None, score float64[N])``; row ``r`` of ``z`` is the
        state of resident row ``r``, so sequence ``s`` is ``z[seq_off[s]:seq_off[s + 1]]``.  Each sequence is
        decoded as ``viterbi([seq_off[s]], len_s, flags)`` decodes it (the chain starts from ``mod_init``),
        bit for bit given the same lliks.  With ``USE_HOST_LLIKS`` the ``[1, T, K]`` batch uploaded by
        ``set_lliks`` holds the lliks of the concatenated rows.  Afterwards ``read_rows("lliks", ..)`` covers
        all T rows."""
        self._pre_mutate()
        off = getattr(self, "seq_off", None)
        n = 0 if off is None else len(off) - 1      # (none declared: the library says so)
        T = max(int(self.T or 0), 0)
        z = np.empty(max(T, 1), dtype=np.int32) if want_z else None
        score = np.empty(max(n, 1))
        L.check(self._lib.svihmm_viterbi_sequences(self._h, int(flags),
                                                   None if z is None else z.ctypes.data_as(C.c_void_p),
                                                   L.dptr(score)), "svihmm_viterbi_sequences")
        self._rows = T
        return (None if z is None else z[:T]), score[:n]

    def ffbs_sequences(self, logA, n_draws=1, uniforms=None, seed=0, flags=0, want_lalpha=False):
        """``n_draws`` FFBS state paths of every declared sequence from ONE forward filter
        (``svihmm_ffbs_sequences``): ``(z int32[S, T], lalpha float64[T, K] or None)``.  ``uniforms`` [S, T]
        holds the uniform of (draw, resident row); without them the device draws its own (Philox4x32-10
        keyed by ``seed``, counter row ``draw * T + row``).  Filter, draw rule and ``logA`` as in
        ``ffbs_windows``; every sequence starts from ``mod_init`` and is sampled back from its own last row."""
        self._pre_mutate()
        S = int(n_draws)
        T = max(int(self.T or 0), 0)
        logA = L.as_f64(logA, (self.K, self.K))
        u = None
        if uniforms is not None:
            u = L.as_f64(uniforms, (max(S, 0), T))
        z = np.empty((max(S, 0), max(T, 1)), dtype=np.int32)
        la = np.empty((max(T, 1), self.K)) if want_lalpha else None
        L.check(self._lib.svihmm_ffbs_sequences(self._h, int(flags), L.dptr(logA), S, L.dptr(u),
                                                int(seed) & 0xFFFFFFFFFFFFFFFF, z.ctypes.data_as(C.c_void_p),
                                                L.dptr(la)), "svihmm_ffbs_sequences")
        self._rows = T
        return z[:, :T], (None if la is None else la[:T])

    def grow_windows(self, centers, half0, probe_off=0, increment=1, cutoff=1000, epsilon=1e-5, rule=0,
                     flags=0, method="auto", trace_cap=0):
        """Adaptive window length / buffer growth on the device (``svihmm_grow_windows``; reference
        ``select_L`` with ``half0 = minHalfL, probe_off = 0``, ``select_buffer`` with ``half0 = probe_off =
        halfL``): for every centre the half-width at which the posterior of its probe rows ``c - probe_off``,
        ``c + probe_off`` stops moving, by the rule stated in ``include/svihmm.h`` (``rule`` 0: last
        residual below ``epsilon``, 1: running average).  ``method``: "auto", "literal" or "products".
        Returns ``(half int32[n], steps int32[n], trace float64[n, trace_cap, 2] or None)``; trace rows
        past a centre's steps are NaN."""
        self._pre_mutate()
        c = np.ascontiguousarray(np.asarray(centers, dtype=np.int64).ravel())
        n, cap = len(c), int(trace_cap)
        half = np.empty(n, dtype=np.int32)
        steps = np.empty(n, dtype=np.int32)
        trace = np.empty((n, cap, 2)) if cap > 0 else None
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        L.check(self._lib.svihmm_grow_windows(self._h, L.i64ptr(c), n, int(half0), int(probe_off), int(increment),
                                              int(cutoff), float(epsilon), int(rule), int(flags),
                                              L.GROW_METHOD[method], vp(half), vp(steps), L.dptr(trace), cap),
                "svihmm_grow_windows")
        return half, steps, trace

    def read_packed(self):
        out = np.empty(self._packed_len())
        L.check(self._lib.svihmm_read_packed(self._h, L.dptr(out)), "svihmm_read_packed")
        return self._wrap_packed(out)

    def read_intermediate(self, what, B, Lm):
        idx = {"lliks": 0, "lalpha": 1, "lbeta": 2, "var_x": 3}[what]
        out = np.empty((B, Lm, self.K))
        L.check(self._lib.svihmm_read_intermediate(self._h, idx, L.dptr(out)),
                "svihmm_read_intermediate")
        return out

    def read_rows(self, what, row0, nrows):
        idx = {"lliks": 0, "lalpha": 1, "lbeta": 2, "var_x": 3}[what]
        out = np.empty((int(nrows), self.K))
        L.check(self._lib.svihmm_read_rows(self._h, idx, int(row0), int(nrows), L.dptr(out)),
                "svihmm_read_rows")
        return out

    def ffbs(self, logA, uniforms, flags=0, want_lalpha=True):
        self._pre_mutate()
        logA = L.as_f64(logA, (self.K, self.K))
        u = L.as_f64(uniforms, (self.T,))
        z = np.empty(self.T, dtype=np.int64)
        la = np.empty((self.T, self.K)) if want_lalpha else None
        L.check(self._lib.svihmm_ffbs(self._h, L.dptr(logA), L.dptr(u), int(flags),
                                      L.i64ptr(z), L.dptr(la)), "svihmm_ffbs")
        return z, la

    def ffbs_sample(self, lalpha, logA, uniforms):
        """Backward sampling only from the supplied forward messages (the ``lalpha_init``
        branch of the reference's FFBS, hmm_fast.pyx:80-95)."""
        self._pre_mutate()
        lalpha = L.as_f64(lalpha)
        T, K = lalpha.shape
        logA = L.as_f64(logA, (K, K))
        u = L.as_f64(uniforms, (T,))
        z = np.empty(T, dtype=np.int64)
        L.check(self._lib.svihmm_ffbs_sample(self._h, T, K, L.dptr(lalpha), L.dptr(logA), L.dptr(u),
                                             L.i64ptr(z)), "svihmm_ffbs_sample")
        return z

    def ffbs_windows(self, starts, Lm, logA, n_draws=1, uniforms=None, seed=0, flags=0, want_lalpha=False):
        """``n_draws`` state paths of every window from ONE forward filter (``svihmm_ffbs_windows``):
        ``(z int32[S, B, Lm], lalpha float64[B, Lm, K] or None)``.  The filter uses the globals and
        the emission family currently set (with ``USE_HOST_LLIKS`` the batch uploaded by
        ``set_lliks``; ``starts`` then only gives the number of windows and may be None); the draws
        use ``logA[k, z_next]`` like ``ffbs``.  ``uniforms`` [S, B, Lm] are consumed one per state;
        without them the device draws its own (Philox4x32-10 keyed by ``seed``, nothing uploaded).
        The draw rule is stated in ``include/svihmm.h``."""
        self._pre_mutate()
        if starts is None:
            if not int(flags) & L.USE_HOST_LLIKS:
                raise RuntimeError("ffbs_windows: starts=None needs USE_HOST_LLIKS (the windows of set_lliks)")
            st, B = None, int(getattr(self, "_host_ll_windows", 0))
        else:
            st = self._starts(starts)
            B = len(st)
        Lm, S = int(Lm), int(n_draws)
        logA = L.as_f64(logA, (self.K, self.K))
        u = None
        if uniforms is not None:
            u = L.as_f64(uniforms, (max(S, 0), B, max(Lm, 0)))
        z = np.empty((max(S, 0), B, max(Lm, 0)), dtype=np.int32)
        la = np.empty((B, max(Lm, 0), self.K)) if want_lalpha else None
        self._rows = B * max(Lm, 0)
        L.check(self._lib.svihmm_ffbs_windows(self._h, L.i64ptr(st), B, Lm, int(flags), L.dptr(logA), S,
                                              L.dptr(u), int(seed) & 0xFFFFFFFFFFFFFFFF,
                                              z.ctypes.data_as(C.c_void_p), L.dptr(la)), "svihmm_ffbs_windows")
        return z, la

    # -- SVI loop with the variational state resident in HBM ---------------------------------
    def svi_begin(self, prior_tran, var_tran, prior, factors, prior_logpart, maxit, zsign=1.0):
        """Upload the state of ``hmmsgd_metaobs.VBHMM.infer``: transition prior / factor [K,K],
        NIW ``prior`` and current ``factors`` as (mu [K,D], sigma [K,D,D], kappa [K], nu [K]).
        Afterwards ``svi_iteration`` runs whole iterations (stationary init, psi-expectations,
        E-step, natural-gradient step, ELBO) on the device without anything coming back."""
        self._pre_mutate()
        var_tran = L.as_f64(var_tran)
        K = var_tran.shape[0]
        prior_tran = L.as_f64(prior_tran, (K, K))
        mu0 = L.as_f64(prior[0]); D = mu0.shape[1]
        arrs = [mu0, L.as_f64(prior[1], (K, D, D)), L.as_f64(prior[2], (K,)), L.as_f64(prior[3], (K,)),
                L.as_f64(prior_logpart, (K,)), L.as_f64(factors[0], (K, D)), L.as_f64(factors[1], (K, D, D)),
                L.as_f64(factors[2], (K,)), L.as_f64(factors[3], (K,))]
        L.check(self._lib.svihmm_svi_begin(self._h, K, D, L.dptr(prior_tran), L.dptr(var_tran),
                                           *([L.dptr(a) for a in arrs] + [int(maxit), float(zsign)])),
                "svihmm_svi_begin")
        self.K, self.family, self._svi = K, ("niw", ()), ("niw", K, D)

    def svi_begin_diag(self, prior_tran, var_tran, prior, factors, maxit):
        """The same loop for ``DiagonalGaussian`` emitters: ``prior`` / ``factors`` as
        (mu, nus, alphas, betas), each [K, D]."""
        self._pre_mutate()
        var_tran = L.as_f64(var_tran)
        K = var_tran.shape[0]
        prior_tran = L.as_f64(prior_tran, (K, K))
        D = np.asarray(prior[0]).shape[1]
        pb = np.ascontiguousarray(np.stack([L.as_f64(a, (K, D)) for a in prior]))
        fb = np.ascontiguousarray(np.stack([L.as_f64(a, (K, D)) for a in factors]))
        L.check(self._lib.svihmm_svi_begin_diag(self._h, K, D, L.dptr(prior_tran), L.dptr(var_tran), L.dptr(pb),
                                                L.dptr(fb), int(maxit)), "svihmm_svi_begin_diag")
        self.K, self.family, self._svi = K, ("diag", ()), ("diag", K, D)

    def svi_begin_cat(self, prior_tran, var_tran, alpha0, alpha, maxit):
        """The same loop for ``Categorical`` emitters over one symbol column: Dirichlet prior and
        factors [K, V]."""
        self._pre_mutate()
        var_tran = L.as_f64(var_tran)
        K = var_tran.shape[0]
        prior_tran = L.as_f64(prior_tran, (K, K))
        alpha0 = L.as_f64(alpha0); V = alpha0.shape[1]
        alpha = L.as_f64(alpha, (K, V))
        L.check(self._lib.svihmm_svi_begin_cat(self._h, K, V, L.dptr(prior_tran), L.dptr(var_tran), L.dptr(alpha0),
                                               L.dptr(alpha), int(maxit)), "svihmm_svi_begin_cat")
        self.K, self.family, self._svi = K, ("cat", (V,)), ("cat", K, V)

    def svi_begin_mcat(self, prior_tran, var_tran, alpha0_cols, alpha_cols, maxit):
        """The same loop for ``ProductCategorical`` emitters over D symbol columns: Dirichlet priors and
        factors as lists of D arrays ``[K, V_d]`` (``svihmm_svi_begin_mcat``)."""
        self._pre_mutate()
        var_tran = L.as_f64(var_tran)
        K = var_tran.shape[0]
        prior_tran = L.as_f64(prior_tran, (K, K))
        a0 = [L.as_f64(a) for a in alpha0_cols]
        if len(a0) < 1 or any(a.ndim != 2 or a.shape[0] != K for a in a0):
            raise RuntimeError("svi_begin_mcat: alpha0_cols must be a non-empty list of [K, V_d] arrays")
        if len(alpha_cols) != len(a0):
            raise RuntimeError("svi_begin_mcat: alpha_cols must have one array per column of alpha0_cols")
        al = [L.as_f64(a, p.shape) for a, p in zip(alpha_cols, a0)]
        Vs = np.ascontiguousarray([a.shape[1] for a in a0], dtype=np.int32)
        p0 = np.ascontiguousarray(np.concatenate(a0, axis=1))
        p1 = np.ascontiguousarray(np.concatenate(al, axis=1))
        L.check(self._lib.svihmm_svi_begin_mcat(self._h, K, len(a0), Vs.ctypes.data_as(C.POINTER(C.c_int32)),
                                                L.dptr(prior_tran), L.dptr(var_tran), L.dptr(p0), L.dptr(p1),
                                                int(maxit)), "svihmm_svi_begin_mcat")
        Vs = tuple(int(v) for v in Vs)
        self.K, self.family, self._svi = K, ("mcat", (Vs,)), ("mcat", K, Vs)

    def svi_begin_poisson(self, prior_tran, var_tran, prior, factors, max_count, maxit):
        """The same loop for ``ProductPoisson`` emitters over D count columns: Gamma ``prior = (a0, b0)`` and
        ``factors = (a, b)`` (shape, rate), each ``[K, D]``; an entry is present when
        ``0 <= x < max_count + 1`` (``svihmm_svi_begin_poisson``)."""
        from .distributions import _logfact_table
        self._pre_mutate()
        var_tran = L.as_f64(var_tran)
        K = var_tran.shape[0]
        prior_tran = L.as_f64(prior_tran, (K, K))
        a0 = L.as_f64(prior[0])
        if a0.ndim != 2 or a0.shape[0] != K:
            raise RuntimeError("svi_begin_poisson: the Gamma parameters must be [K, D] arrays")
        D = a0.shape[1]
        C_ = int(max_count)
        if not 0 <= C_ <= L.POISSON_MAX_COUNT:
            raise RuntimeError("svi_begin_poisson: max_count = %d outside [0, %d]" % (C_, L.POISSON_MAX_COUNT))
        pb = np.ascontiguousarray(np.stack([a0, L.as_f64(prior[1], (K, D))]))
        fb = np.ascontiguousarray(np.stack([L.as_f64(a, (K, D)) for a in factors]))
        logfact = np.ascontiguousarray(_logfact_table(C_), dtype=np.float64)
        L.check(self._lib.svihmm_svi_begin_poisson(self._h, K, D, L.dptr(prior_tran), L.dptr(var_tran), L.dptr(pb),
                                                   L.dptr(fb), L.dptr(logfact), C_, int(maxit)),
                "svihmm_svi_begin_poisson")
        self.K, self.family, self._svi = K, ("poisson", (D,)), ("poisson", K, D)

    def svi_read_factors(self):
        """(var_tran, var_init, factors) with ``factors`` in the loop's family layout: NIW
        (mu, sigma, kappa, nu), diagonal (mu, nus, alphas, betas), Categorical alpha [K, V],
        multi-column Categorical the list of D arrays alpha_d [K, V_d], Poisson (a, b), each [K, D]."""
        name, K, W = self._svi
        fam = FAMILY_STATS[name]
        vt, vi, blk = np.empty((K, K)), np.empty(K), np.empty(fam.block(K, W))
        L.check(self._lib.svihmm_svi_read_factors(self._h, L.dptr(vt), L.dptr(vi), L.dptr(blk)),
                "svihmm_svi_read_factors")
        return vt, vi, fam.split(blk, K, W)

    def svi_iteration(self, it, starts, nwin_total, Lm, flags, rho, bfactA, bfactE, inner=None):
        """Enqueue iteration ``it`` on the windows ``starts`` (asynchronous)."""
        self._pre_mutate()
        st = self._starts(starts)
        off, ln = (0, int(Lm)) if inner is None else (int(inner[0]), int(inner[1]))
        self._rows = len(st) * int(Lm)
        self._held = ("windows", st, int(Lm))
        L.check(self._lib.svihmm_svi_iteration(self._h, int(it), L.i64ptr(st), len(st), int(nwin_total),
                                               int(Lm), off, ln, int(flags), float(rho), float(bfactA),
                                               float(bfactE)), "svihmm_svi_iteration")

    def svi_sequences(self, prior_init, var_init):
        """After any ``svi_begin*``: the loop steps on minibatches of whole declared sequences
        (``svihmm_svi_sequences``); ``prior_init`` / ``var_init`` [K], the learned initial-state factor, join the
        resident state."""
        self._pre_mutate()
        K = self._svi[1] if self._svi else np.asarray(var_init).shape[0]   # (no loop begun through this object: the library says so)
        p, v = L.as_f64(prior_init, (K,)), L.as_f64(var_init, (K,))
        L.check(self._lib.svihmm_svi_sequences(self._h, L.dptr(p), L.dptr(v)), "svihmm_svi_sequences")

    def svi_iteration_sequences(self, it, idx, flags, rho, bfact):
        """Enqueue iteration ``it`` on the declared sequences listed in ``idx`` (asynchronous; ``bfact = N / M``)."""
        self._pre_mutate()
        ix = np.ascontiguousarray(np.asarray(idx).ravel(), dtype=np.int32)
        if not np.array_equal(ix, np.asarray(idx).ravel()):
            raise RuntimeError("svi_iteration_sequences: idx must hold integers that fit 32 bits")
        L.check(self._lib.svihmm_svi_iteration_sequences(
            self._h, int(it), ix.ctypes.data_as(C.POINTER(C.c_int32)) if len(ix) else None, len(ix), int(flags),
            float(rho), float(bfact)), "svihmm_svi_iteration_sequences")
        off = getattr(self, "seq_off", None)
        if off is not None and len(ix):
            self._rows = int((off[ix + 1] - off[ix]).sum())
            self._held = ("subset", ix)

    def svi_set_adagrad(self, ada_G):
        """AdaGrad accumulator of the transition factor joins the resident state (reference
        hmmsgd_metaobs.py:1036-1040); ``None`` switches back to the plain rho step."""
        if ada_G is None:
            L.check(self._lib.svihmm_svi_set_adagrad(self._h, None), "svihmm_svi_set_adagrad")
            return
        g = L.as_f64(ada_G, (self.K, self.K))
        L.check(self._lib.svihmm_svi_set_adagrad(self._h, L.dptr(g)), "svihmm_svi_set_adagrad")

    def svi_read_adagrad(self):
        out = np.empty((self.K, self.K))
        L.check(self._lib.svihmm_svi_read_adagrad(self._h, L.dptr(out)), "svihmm_svi_read_adagrad")
        return out

    def svi_read_elbo(self, n):
        """(elbo_vec[:n], device milliseconds of each iteration); waits for the device."""
        e = np.empty(int(n)); ms = np.empty(int(n))
        L.check(self._lib.svihmm_svi_read_elbo(self._h, int(n), L.dptr(e), L.dptr(ms)), "svihmm_svi_read_elbo")
        return e, ms

    def svi_recoveries(self):
        """How often the current loop left its device-side counters for stream events mid-way (svihmm_debug.h)."""
        n = C.c_int32()
        L.check(self._lib.svihmm_svi_recoveries(self._h, C.byref(n)), "svihmm_svi_recoveries")
        return int(n.value)

    def svi_read_state(self):
        """Current (var_tran, var_init, mu, sigma, kappa, nu); waits for the device."""
        _, K, D = self._svi
        if isinstance(D, tuple):                # (multi-column Categorical: the library refuses, NIW layout)
            D = len(D)
        out = [np.empty((K, K)), np.empty(K), np.empty((K, D)), np.empty((K, D, D)), np.empty(K), np.empty(K)]
        L.check(self._lib.svihmm_svi_read_state(self._h, *[L.dptr(a) for a in out]), "svihmm_svi_read_state")
        return tuple(out)

    def read_globals(self):
        """(mod_init [K], ltran [K,K]) as the recursions currently hold them."""
        mi, lt = np.empty(self.K), np.empty((self.K, self.K))
        L.check(self._lib.svihmm_read_globals(self._h, L.dptr(mi), L.dptr(lt)), "svihmm_read_globals")
        return mi, lt

    # -- multi-GPU ------------------------------------------------------------------------
    def comm_unique_id(self):
        buf = C.create_string_buffer(128)
        L.check(self._lib.svihmm_comm_unique_id(buf), "svihmm_comm_unique_id")
        return buf.raw

    def comm_init(self, uid, rank, nranks):
        L.check(self._lib.svihmm_comm_init(self._h, uid, int(rank), int(nranks)),
                "svihmm_comm_init")
        self._comm = True

    def comm_count(self):
        """Number of ranks RCCL itself reports for the communicator (0 without one)."""
        n = C.c_int32()
        L.check(self._lib.svihmm_comm_count(self._h, C.byref(n)), "svihmm_comm_count")
        return n.value

    def allreduce_packed(self):
        L.check(self._lib.svihmm_allreduce_packed(self._h), "svihmm_allreduce_packed")

    def export_packed(self):
        """This handle's statistics as the all-reduce would put them on the wire (caller coordinates)."""
        out = np.empty(self._packed_len())
        L.check(self._lib.svihmm_export_packed(self._h, L.dptr(out)), "svihmm_export_packed")
        return out

    def import_packed(self, buf):
        """The reduced vector of a host-side exchange back into the handle (see export_packed)."""
        buf = L.as_f64(buf, (self._packed_len(),))
        L.check(self._lib.svihmm_import_packed(self._h, L.dptr(buf)), "svihmm_import_packed")

    def allreduce_host(self, arr, op="sum"):
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float64).ravel())
        L.check(self._lib.svihmm_allreduce_host(self._h, L.dptr(a), a.size,
                                                1 if op == "max" else 0),
                "svihmm_allreduce_host")
        return a.reshape(np.shape(arr))

    # -- measurement ------------------------------------------------------------------------
    def profile(self, on=True, only=None):
        """HIP events around the handle's launches; ``only``: names of the kernel slots to bracket
        (``svihmm_kernel_name``), the others run without events."""
        v = 1 if on else 0
        if on and only is not None:
            names = [self._lib.svihmm_kernel_name(i).decode() for i in range(L.NKERN)]
            v = L.PROF_SLOTS
            for n in only:
                v |= 1 << names.index(n)
        L.check(self._lib.svihmm_profile_enable(self._h, v), "profile_enable")

    def profile_reset(self):
        L.check(self._lib.svihmm_profile_reset(self._h), "profile_reset")

    def profile_read(self):
        ms = np.zeros(L.NKERN)
        cnt = np.zeros(L.NKERN, dtype=np.int64)
        L.check(self._lib.svihmm_profile_read(self._h, L.dptr(ms), L.i64ptr(cnt)), "profile_read")
        names = [self._lib.svihmm_kernel_name(i).decode() for i in range(L.NKERN)]
        return {n: (float(m), int(c)) for n, m, c in zip(names, ms, cnt) if c > 0}

    def last_kernel(self, slot_name):
        """Name of the kernel function the slot's last launch dispatched ("" when not recorded)."""
        names = [self._lib.svihmm_kernel_name(i).decode() for i in range(L.NKERN)]
        return self._lib.svihmm_last_kernel_name(self._h, names.index(slot_name)).decode()

    def set_variant(self, which, value):
        """``which``: a slot name of ``_lib.VARIANT`` or its index; include/svihmm_debug.h lists every slot's codes."""
        idx = L.VARIANT[which] if isinstance(which, str) else which
        L.check(self._lib.svihmm_set_variant(self._h, idx, int(value)), "set_variant")

    def selftest_mfma(self, A, B):
        A = L.as_f64(A, (16, 4)); B = L.as_f64(B, (4, 16))
        out = np.empty((16, 16))
        L.check(self._lib.svihmm_selftest_mfma(self._h, L.dptr(A), L.dptr(B), L.dptr(out)),
                "selftest_mfma")
        return out


def device_count():
    n = C.c_int()
    lib = L.load()
    rc = lib.svihmm_device_count(C.byref(n))
    return n.value if rc == 0 else 0
