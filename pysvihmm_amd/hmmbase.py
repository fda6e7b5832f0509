"""VariationalHMMBase -- same class surface as the reference ``hmmbase.py``.

The E-step methods (``local_update``, ``forward_msgs``, ``backward_msgs``,
``full_local_update``, ``ffbs_fast``) run on the MI355X through the C ABI
(``pysvihmm_amd.engine.HipEngine``); everything cheap and O(K^2 + K D^2) stays
host-side NumPy with the reference's formulas: psi-expectations
(reference hmmbase.py:214-216, SciPy digamma), ELBO (hmmbase.py:145-199), metrics
(hmmbase.py:346-406).

State flows through instance attributes exactly like the reference (``obs, mask,
var_init, var_tran, var_emit, lliks, lalpha, lbeta, var_x, mod_init, mod_tran``).
The engine handle is never pickled (``__getstate__``).

``engine=`` lets a caller supply the engine object (tests inject the oracle to
exercise the host logic without a GPU).  The default is the HIP engine; there is
no CPU fallback: constructing it without the built library / a GPU raises.
"""
from __future__ import division

import abc
import collections
from copy import deepcopy

import numpy as np
import numpy.linalg as npl
import scipy.spatial.distance as dist
from numpy import newaxis as npa
from scipy.special import digamma, gammaln

from . import util
from . import _lib as L
from .distributions import (Categorical, DiagonalGaussian, Gaussian, ProductCategorical, ProductGaussian, ProductPoisson,
                            niw_prior_logpart, vlb_logz_sign)
from .engine import rewrap_packed

# This is for taking logs of things so we don't get -inf (reference hmmbase.py:30)
eps = 1e-9
DBL_EPSILON = float(np.finfo(np.float64).eps)


def is_niw_gaussian(e):
    """Device fast path is keyed on the concrete emission family, mirroring the
    reference's ``type(self.var_emit[0]) is Gaussian`` dispatch
    (hmmsgd_metaobs.py:887,1050): ``Gaussian`` itself, subclasses that keep its
    ``expected_log_likelihood`` (an override must be honoured, so such objects take the generic
    plugin route: host ``expected_log_likelihood`` -> uploaded ``lliks``), or any class that opts in
    with ``svihmm_niw_fastpath = True``."""
    t = type(e)
    if getattr(t, "svihmm_niw_fastpath", False):
        return True
    return isinstance(e, Gaussian) and t.expected_log_likelihood is Gaussian.expected_log_likelihood


def is_diag_gaussian(e):
    """Diagonal-covariance family (``distributions.DiagonalGaussian`` and subclasses that keep
    its ``expected_log_likelihood``): the device runs it on 2 D + 1 features per row."""
    t = type(e)
    return (isinstance(e, DiagonalGaussian)
            and t.expected_log_likelihood is DiagonalGaussian.expected_log_likelihood)


def concat_sequences(obs, mask=None):
    """``obs`` as a list / tuple of ``[T_s, D]`` arrays (several independent sequences) ->
    ``(rows [sum T_s, D], mask or None, seq_off int64[N + 1])``; ``mask`` may be a matching list, one
    concatenated array or None.  Anything else passes through with ``seq_off = None``.  A one-element
    list gives that element itself (the model then behaves exactly as with the bare array)."""
    if not isinstance(obs, (list, tuple)):
        return obs, mask, None
    if len(obs) == 0:
        raise RuntimeError("obs is an empty list of sequences")
    seqs = [np.asarray(o) for o in obs]
    if any(o.ndim != seqs[0].ndim or o.ndim not in (1, 2) or o.shape[0] < 1 for o in seqs) or \
            any(o.shape[1:] != seqs[0].shape[1:] for o in seqs):
        raise RuntimeError("every sequence must be a non-empty [T_s, D] array of one common D")
    seq_off = np.zeros(len(seqs) + 1, dtype=np.int64)
    np.cumsum([o.shape[0] for o in seqs], out=seq_off[1:])
    if isinstance(mask, (list, tuple)):
        if len(mask) != len(seqs) or any(np.shape(m) != (o.shape[0],) for m, o in zip(mask, seqs)):
            raise RuntimeError("mask must list one [T_s] array per sequence")
        mask = mask[0] if len(seqs) == 1 else np.concatenate([np.asarray(m).astype('bool') for m in mask])
    elif mask is not None and np.shape(mask) != (int(seq_off[-1]),):
        raise RuntimeError("a concatenated mask must have one entry per row of all sequences")
    rows = obs[0] if len(seqs) == 1 else np.concatenate(seqs, axis=0)
    return rows, mask, seq_off


def dirichlet_elbo(prior, var):
    """sum over rows of E_q[log Dir(.|prior_r)] + H[Dir(.|var_r)] for row-wise Dirichlet factors
    (the ``*_energy + *_entropy`` terms of reference hmmbase.py:150-181 and
    hmmsgd_metaobs.py:277-292, with their ``eps`` placement inside gammaln / digamma)."""
    prior = np.asarray(prior, dtype=np.float64)
    var = np.asarray(var, dtype=np.float64)
    elog = digamma(var + eps) - digamma(var.sum(axis=1) + eps)[:, npa]      # E_q log theta
    lognorm = lambda a: gammaln(a.sum(axis=1) + eps) - gammaln(a + eps).sum(axis=1)
    energy = lognorm(prior) + ((prior - 1.) * elog).sum(axis=1)
    entropy = -(lognorm(var) + ((var - 1.) * elog).sum(axis=1))
    return float(energy.sum() + entropy.sum())


# ---- the emission families the device evaluates itself: one ordered table ------------------------------------------
# A record per family, in the order the predicates are asked (``VariationalHMMBase._family``):
#   name        the family's name, also its key in ``engine.FAMILY_STATS``
#   pred        name of the model's predicate method (subclasses override these, so they are looked up by name)
#   push        push(model, engine): upload the emitters' factors / tables through the engine's ``set_emission_*``
#   emitter     the class whose ``get_vlb`` the resident SVI loop's ELBO kernels restate (None: no resident loop)
#   svi_method  name of the engine's ``svi_begin*`` (None: no resident loop)
#   svi_args    svi_args(model, maxit): that call's arguments after (prior_tran, var_tran)
#   svi_pull    svi_pull(model): the loop's resident state -> the object's attributes (reference attribute names)
#   heldout     "rows": only whole rows can be held out; "entries": single entries too (heldout_entries_logprob)
#   by_type     by_type(model): the emitters are the family's as far as their types say (no engine is touched)
Family = collections.namedtuple("Family", "name pred push emitter svi_method svi_args svi_pull heldout by_type")


def _stack(ve, *names):
    return tuple(np.array([getattr(g, n) for g in ve], dtype=np.float64) for n in names)


def _all_exactly(cls):
    return lambda m: len(m.var_emit) > 0 and all(type(e) is cls for e in m.var_emit)


def _push_cat(m, eng):
    # Categorical: E log theta table (pybasicbayes Categorical.expected_log_likelihood), looked up on the device
    eng.set_emission_cat(np.stack([digamma(e.alpha_mf) - digamma(np.sum(e.alpha_mf)) for e in m.var_emit]))


def _push_mcat(m, eng):
    # D symbol columns: one E log theta table [K, V_d] per column, looked up and added on the device
    per_state = [e.expected_log_tables() for e in m.var_emit]
    eng.set_emission_mcat([np.stack([t[d] for t in per_state]) for d in range(len(per_state[0]))])


def _push_poisson(m, eng):
    # D count columns: (E log lambda, E lambda) per state and column, multiplied and added on the device
    tabs = [e.expected_tables() for e in m.var_emit]
    eng.set_emission_poisson(np.stack([t[0] for t in tabs]), np.stack([t[1] for t in tabs]), m.var_emit[0].max_count)


def _push_pgauss(m, eng):
    # D real-valued columns with missing entries: (mu, hprec, cst) per state and column; the squared residual of
    # each present entry is formed on the device
    tabs = [e.expected_tables() for e in m.var_emit]
    eng.set_emission_pgauss(*[np.stack([t[i] for t in tabs]) for i in range(3)], origin=m._pgauss_origin())


def _svi_args_niw(m, maxit):
    prior = m._prior_arrays()
    return prior, m._emission_arrays(), niw_prior_logpart(prior[1], prior[3]), maxit, vlb_logz_sign()


def _svi_args_mcat(m, maxit):
    ve = m.var_emit
    stack = lambda name: [np.array([getattr(g, name)[d] for g in ve], dtype=np.float64) for d in range(ve[0].D)]
    return stack("alphav_0"), stack("alpha_mf"), maxit


def _svi_pull_niw(m):
    vt, vi, mu, sg, ka, nu = m.engine.svi_read_state()
    m.var_tran, m.var_init = vt, vi
    D = m.D
    for k, G in enumerate(m.var_emit):
        G.mu_mf = mu[k]; G.sigma_mf = sg[k]
        G.kappa_mf = ka[k]; G.nu_mf = nu[k]
        G.mu = G.mu_mf
        G.sigma = G.sigma_mf / (G.nu_mf - D - 1)


def _svi_pull_factors(set_emitter):
    def pull(m):
        m.var_tran, m.var_init, fac = m.engine.svi_read_factors()
        for k, G in enumerate(m.var_emit):
            set_emitter(G, k, fac)
    return pull


def _set_cat(G, k, fac):
    G._alpha_mf = fac[k].copy()
    G.weights = G._alpha_mf / G._alpha_mf.sum()


_svi_pull_mf = _svi_pull_factors(lambda G, k, fac: G._set_mf(*[a[k].copy() for a in fac]))

FAMILIES = (
    Family("niw", "_niw_fastpath", lambda m, eng: eng.set_emission_niw(*m._emission_arrays()), Gaussian,
           "svi_begin", _svi_args_niw, _svi_pull_niw, "rows", lambda m: m._niw_fastpath()),
    # diagonal family: the K x D normal-inverse-gamma factors; lliks on 2 D + 1 features
    Family("diag", "_diag_fastpath", lambda m, eng: eng.set_emission_diag(*m._diag_arrays()), DiagonalGaussian,
           "svi_begin_diag",
           lambda m, maxit: (_stack(m.var_emit, "mu_0", "nus_0", "alphas_0", "betas_0"), m._diag_arrays(), maxit),
           _svi_pull_mf, "rows", lambda m: len(m.var_emit) > 0 and all(is_diag_gaussian(e) for e in m.var_emit)),
    Family("cat", "_cat_fastpath", _push_cat, Categorical, "svi_begin_cat",
           lambda m, maxit: _stack(m.var_emit, "alphav_0", "alpha_mf") + (maxit,),
           _svi_pull_factors(_set_cat), "rows", lambda m: m._cat_fastpath()),
    Family("mcat", "_mcat_fastpath", _push_mcat, ProductCategorical, "svi_begin_mcat", _svi_args_mcat,
           _svi_pull_factors(lambda G, k, fac: G._set_alpha([c[k] for c in fac])), "entries",
           _all_exactly(ProductCategorical)),
    Family("poisson", "_poisson_fastpath", _push_poisson, ProductPoisson, "svi_begin_poisson",
           lambda m, maxit: (_stack(m.var_emit, "alpha_0", "beta_0"), _stack(m.var_emit, "alpha_mf", "beta_mf"),
                             m.var_emit[0].max_count, maxit),
           _svi_pull_mf, "entries", _all_exactly(ProductPoisson)),
    Family("pgauss", "_pgauss_fastpath", _push_pgauss, None, None, None, None, "entries",
           _all_exactly(ProductGaussian)),
)
FAMILY = {f.name: f for f in FAMILIES}


class VariationalHMMBase(object, metaclass=abc.ABCMeta):
    """Abstract base class for finite variational HMMs."""

    # Interface
    @abc.abstractmethod
    def global_update(self):
        pass

    @abc.abstractmethod
    def infer(self):
        """ Perform inference. """
        pass

    @staticmethod
    def make_param_dict(prior_init, prior_tran, prior_emit, mask=None):
        return {'prior_init': prior_init, 'prior_tran': prior_tran,
                'prior_emit': prior_emit, 'mask': mask}

    def set_mask(self, mask):
        if mask is None:
            self.mask = np.zeros(self.obs.shape[0], dtype='bool')
        else:
            self.mask = np.asarray(mask).astype('bool')
        self._obs_dirty = True

    def set_labels(self, labels):
        """Partially labelled rows: ``labels[t] = -1`` leaves row ``t`` free, ``labels[t] = k`` says the row is
        known to be in state ``k``.  One int-valued array over the rows, or -- when ``obs`` was a list -- a list with
        one array per sequence.  ``None`` removes the labels.  Every E-step and decoder of the model then sees
        ``lliks[t, j] = -inf`` for ``j != labels[t]`` at the labelled rows (``local_update``, the batch ``infer()``
        loops, ``viterbi()``, ``ffbs_windows()``, ``heldout_logprob()``): on the device where the engine has
        ``set_labels``, else through host lliks clamped here.  A label whose state is impossible under the initial
        and transition factors leaves that chain's results unspecified (``-inf`` / NaN)."""
        if labels is None:
            self.labels = None
            self._obs_dirty = True
            return
        so = self.__dict__.get("seq_off")
        if isinstance(labels, (list, tuple)) and len(labels) and np.ndim(labels[0]) >= 1:
            lens = [len(a) for a in labels]
            want = [int(n) for n in np.diff(so)] if so is not None else [self.obs.shape[0]]
            if lens != want:
                raise ValueError("set_labels: the list's lengths %s do not match the sequences' %s" % (lens, want))
            labels = np.concatenate([np.asarray(a).ravel() for a in labels])
        a = np.asarray(labels)
        if a.ndim != 1 or a.shape[0] != self.obs.shape[0]:
            raise ValueError("set_labels: labels must have shape (%d,), got %s" % (self.obs.shape[0], a.shape))
        if not np.issubdtype(a.dtype, np.integer):
            if not (np.issubdtype(a.dtype, np.floating) and np.all(a == np.rint(a))):
                raise ValueError("set_labels: labels must be int-valued")
        a = a.astype(np.int64)
        if a.size and a.min() < -1:
            t = int(np.flatnonzero(a < -1)[0])
            raise ValueError("set_labels: labels[%d] = %d (-1 means free, a state index means known)" % (t, a[t]))
        if a.size and a.max() >= self.K:
            t = int(np.argmax(a))
            raise ValueError("set_labels: labels[%d] = %d, the model has K = %d states" % (t, a[t], self.K))
        self.labels = a.astype(np.int32)
        self.state_sets = None                  # (labels and allowed-state sets are alternatives)
        self._obs_dirty = True

    def set_state_sets(self, allowed):
        """Allowed-state sets per row, the weaker statement than a label: ``allowed[t, k]`` is True where row ``t``
        may be in state ``k``; a row of all True is free.  One bool array ``[T, K]`` over the rows, or -- when ``obs``
        was a list -- a list with one bool array ``[T_s, K]`` per sequence.  ``None`` removes the sets.  Sets replace
        labels, as ``set_labels`` replaces sets.  Every E-step and decoder of the model then sees
        ``lliks[t, k] = -inf`` wherever ``allowed[t, k]`` is False, in the places ``set_labels`` lists: on the device
        where the engine has ``set_state_sets``, else through host lliks clamped here.  A set none of whose states is
        possible under the initial and transition factors leaves that chain's results unspecified."""
        if allowed is None:
            self.state_sets = None
            self._obs_dirty = True
            return
        so = self.__dict__.get("seq_off")
        T = self.obs.shape[0]
        if isinstance(allowed, (list, tuple)) and len(allowed) and np.ndim(allowed[0]) >= 2:
            lens = [len(a) for a in allowed]
            want = [int(n) for n in np.diff(so)] if so is not None else [T]
            if lens != want:
                raise ValueError("set_state_sets: the list's lengths %s do not match the sequences' %s" % (lens, want))
            widths = sorted(set(np.shape(a)[1] for a in allowed))
            if widths != [self.K]:
                raise ValueError("set_state_sets: the arrays have %s columns, the model has K = %d states"
                                 % (widths, self.K))
            allowed = np.concatenate([np.asarray(a) for a in allowed])
        a = np.asarray(allowed)
        if a.ndim != 2 or a.shape[0] != T:
            raise ValueError("set_state_sets: allowed must have shape (%d, %d), got %s" % (T, self.K, a.shape))
        if a.shape[1] != self.K:
            raise ValueError("set_state_sets: allowed has %d columns, the model has K = %d states"
                             % (a.shape[1], self.K))
        if a.dtype != np.bool_:
            raise ValueError("set_state_sets: allowed must be a bool array, got dtype %s" % a.dtype)
        empty = np.flatnonzero(~a.any(axis=1))
        if empty.size:
            raise ValueError("set_state_sets: row %d allows no state (a free row is all True)" % int(empty[0]))
        self.state_sets = np.ascontiguousarray(a)
        self.labels = None                      # (sets and labels are alternatives)
        self._obs_dirty = True

    def _clamp_lliks(self, ll, windows, Lm):
        """The labels' clamp of host lliks ``ll`` [B, Lm, K] of the windows ``windows`` (in place): at a labelled
        row every state but the label gets ``-inf``, the label's entry keeps its bits.  Allowed-state sets
        (``set_state_sets``): ``-inf`` wherever the row does not allow the state."""
        sets = self.__dict__.get("state_sets")
        if sets is not None:
            for b, s in enumerate(windows):
                ll[b][~sets[s:s + Lm]] = -np.inf
            return ll
        lab = self.__dict__.get("labels")
        if lab is None:
            return ll
        for b, s in enumerate(windows):
            l = lab[s:s + Lm]
            rows = np.flatnonzero(l >= 0)
            keep = ll[b, rows, l[rows]].copy()
            ll[b, rows, :] = -np.inf
            ll[b, rows, l[rows]] = keep
        return ll

    def _labels_on_host(self):
        """Labels or allowed-state sets are set and the engine does not take them: lliks are evaluated and clamped
        on the host."""
        if self.__dict__.get("state_sets") is not None:
            return not hasattr(self.engine, "set_state_sets")
        return self.__dict__.get("labels") is not None and not hasattr(self.engine, "set_labels")

    def __init__(self, obs, prior_init, prior_tran, prior_emit, mask=None,
                 init_init=None, init_tran=None, verbose=False, sts=None,
                 engine=None, device=0, dtype="f64"):
        self.verbose = verbose
        self.sts = sts

        # Save the hyperparameters
        self.prior_init = deepcopy(np.asarray(prior_init)).astype('float64')
        self.prior_tran = deepcopy(np.asarray(prior_tran)).astype('float64')
        self.prior_emit = deepcopy(prior_emit)

        # Initialize global variational distributions.
        if init_init is None:
            self.var_init = self.prior_init / np.sum(self.prior_init)
        else:
            self.var_init = np.array(init_init, dtype='float64')
        if init_tran is None:
            self.var_tran = self.prior_tran / np.sum(self.prior_tran, axis=1)[:, np.newaxis]
        else:
            self.var_tran = np.array(init_tran, dtype='float64')

        # copy: mean and covariance of the prior objects are the (random) initial values
        self.var_emit = deepcopy(prior_emit)

        # several sequences (a list of [T_s, D] arrays): rows concatenated, offsets beside them
        obs, mask, self.seq_off = concat_sequences(obs, mask)
        self.obs = obs
        self.K = self.prior_tran.shape[0]
        if obs.ndim == 1:
            self.T = obs.shape[0]
            self.D = 1
        elif obs.ndim == 2:
            self.T, self.D = obs.shape
        else:
            raise RuntimeError("obs must have 1 or 2 dimensions")
        self.labels = None
        self.state_sets = None
        self.set_mask(mask)

        self.elbo = -np.inf
        self._engine = engine
        self._device = device
        self._dtype = dtype       # "f64" (the reference's type) or "f32" (engine precision mode)
        self._obs_dirty = True
        self._lZ = None

    # -- engine plumbing -----------------------------------------------------------
    @property
    def engine(self):
        if self._engine is None:
            from .engine import HipEngine
            self._engine = HipEngine(self._device, dtype=getattr(self, "_dtype", "f64"))  # raises without library/GPU
            self._obs_dirty = True
        return self._engine

    def __getstate__(self):
        pend = self.__dict__.get("_pending_rows")
        if pend is not None:      # resolve device-resident attributes before the handle goes
            for name in list(pend[2]):
                getattr(self, name)
        d = dict(self.__dict__)
        d.pop('_pending_rows', None)
        d.pop('_prior_stack', None)
        d.pop('_host_lliks', None)
        d.pop('_obs_print', None)
        d.pop('_seq_var_x', None)
        d['_engine'] = None       # device handles are not picklable
        d['_obs_dirty'] = True
        return d

    def __setstate__(self, d):
        self.__dict__.update(d)

    def set_data(self, obs, mask=None):
        obs, mask, self.seq_off = concat_sequences(obs, mask)
        self.obs = obs
        if self._multi():
            self.T = int(self.seq_off[-1])      # (several sequences state their own row count)
        if mask is None:
            self.mask = np.zeros(self.obs.shape[0], dtype='bool')
        else:
            self.mask = mask
        lab = self.__dict__.get("labels")
        if lab is not None and len(lab) != self.obs.shape[0]:
            self.labels = None                  # (labels described the previous rows)
        sets = self.__dict__.get("state_sets")
        if sets is not None and len(sets) != self.obs.shape[0]:
            self.state_sets = None
        self._obs_dirty = True

    def _upload_obs(self, force=False):
        """obs/mask -> HBM (once; again after set_data / in-place edits flagged by
        ``_obs_dirty``, or when another model has used the same engine since: the resident copy
        belongs to whoever uploaded last -- the engines clear ``_obs_owner`` on every upload).
        Coordinates are the engine's business: the resident copy is kept centred inside the
        handle, means and statistics cross the C ABI in the coordinates of ``self.obs``
        (include/svihmm.h, svihmm_set_obs)."""
        eng = self.engine
        if force or self._obs_dirty or getattr(eng, "_obs_owner", None) != id(self):
            if self._pgauss_fastpath():
                # the family goes in force before the rows do: an upload under it is not centred, so the device reads
                # the caller's bits -- and a 1e308-style sentinel, finite to the Gaussian families' centring, cannot
                # drag a centre that the way back would then have to undo in rounded arithmetic
                self._push_emission()
            eng.set_obs(self.obs, self.mask)
            if self._multi() and hasattr(eng, "set_sequences"):
                # (from here on the engine rejects windows that hold rows of two sequences)
                eng.set_sequences(np.diff(self.seq_off))
            if self.__dict__.get("labels") is not None and hasattr(eng, "set_labels"):
                # (the upload above removed whatever labels the handle held)
                eng.set_labels(self.labels)
            if self.__dict__.get("state_sets") is not None and hasattr(eng, "set_state_sets"):
                eng.set_state_sets(self.state_sets)
            eng._obs_owner = id(self)
            self._obs_dirty = False
            self._obs_print = self._obs_fingerprint()

    def _obs_fingerprint(self):
        """Identity + content probe of ``self.obs`` / ``self.mask``: buffer address, shape,
        strides and the bytes of a strided sample (every 509th element, the first and last 4096)
        and of the whole mask.  Only consulted when the caller opted in with
        ``assume_obs_unchanged = True`` (an attribute of the model): by default every ``infer()``
        uploads ``self.obs`` again, like the reference reads it afresh on every call -- a checksum
        of the whole buffer (0.26 s for 256 MB) costs 50 x the upload it would save (4.5 ms)."""
        import zlib
        o = np.asarray(self.obs)
        flat = o.reshape(-1) if o.flags.c_contiguous else None
        if flat is None:
            return None                   # (unusual layout: no probe, always upload)
        sample = np.concatenate((flat[:4096], flat[::509], flat[-4096:]))
        m = np.ascontiguousarray(self.mask)
        return (o.__array_interface__["data"][0], o.shape, o.strides, hash(sample.tobytes()),
                m.shape, zlib.crc32(m.view(np.uint8)))

    def _obs_unchanged(self):
        if not getattr(self, "assume_obs_unchanged", False):
            return False                  # default: upload again (in-place edits of any size count)
        fp = self.__dict__.get("_obs_print")
        return fp is not None and fp == self._obs_fingerprint()

    # -- several sequences ----------------------------------------------------------
    def _multi(self):
        """More than one sequence (``obs`` was a list of at least two): total statistics are the
        sums over the sequences, nothing crosses a join."""
        so = self.__dict__.get("seq_off")
        return so is not None and len(so) > 2

    def _require_fused_sequences(self, fused):
        if self._multi() and not fused:
            raise RuntimeError("several sequences: infer(fused=False) and local_update / global_update "
                               "overrides are not supported (the literal global_update would walk "
                               "across the joins)")

    def _sequences_estep(self):
        """E-step of all sequences under the current variational parameters: ``(stats, lb, q0)`` with
        the statistics summed over the sequences (batch transition form), ``lb = sum_s local_lb[s]``
        and ``q0 = sum_s var_x[first row of s]``.  One ``estep_sequences`` call where the engine has
        it, else one ``estep([off], len)`` per sequence with the sums formed here."""
        if not self._device_family() and not self._labels_on_host():
            raise RuntimeError("several sequences need an emission family the device evaluates "
                               "(NIW / diagonal Gaussian, Categorical, multi-column Categorical, Poisson or "
                               "Gaussian tracks on an engine with set_emission_mcat / _poisson / _pgauss): host "
                               "lliks are not supported")
        self._psi_expectations()
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission()
        self._seq_flags = flags
        eng = self.engine
        self._seq_var_x = None
        if hasattr(eng, "estep_sequences") and not flags & L.USE_HOST_LLIKS:
            st, seq_lb, q0 = eng.estep_sequences(flags=flags)
            return st, float(st.lb[0]), q0
        so = self.seq_off
        total, lb, q0 = None, 0., np.zeros(self.K)
        var_x = np.empty((self.T, self.K))
        for s in range(len(so) - 1):
            off, ln = int(so[s]), int(so[s + 1] - so[s])
            if flags & L.USE_HOST_LLIKS:        # (labels clamped on the host: the sequence's slice of the [1, T, K] batch)
                eng.set_lliks(self._host_lliks[:, off:off + ln])
            st = eng.estep([off], ln, flags=flags)
            total = st.buf.copy() if total is None else total + st.buf
            lb += float(st.lb[0])
            var_x[off:off + ln] = eng.read_intermediate("var_x", 1, ln)[0]
            q0 += var_x[off]
        self._seq_var_x = var_x
        st = rewrap_packed(st, total)
        st.lb[0] = lb
        return st, lb, q0

    def _sequence_subset_estep(self, idx):
        """E-step of the sequences listed in ``idx`` only (a minibatch of whole sequences; an entry that
        occurs twice counts twice): ``(stats, lb, q0)`` as ``_sequences_estep`` returns them, summed over the
        listed sequences.  One ``estep_sequence_subset`` call where the engine has it, else one
        ``estep([off], len)`` per listed sequence with the sums formed here.  No per-row attribute is set."""
        if not self._device_family() and not self._labels_on_host():
            raise RuntimeError("several sequences need an emission family the device evaluates "
                               "(NIW / diagonal Gaussian, Categorical, multi-column Categorical, Poisson or "
                               "Gaussian tracks on an engine with set_emission_mcat / _poisson / _pgauss): host "
                               "lliks are not supported")
        self._psi_expectations()
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission()
        self._seq_flags = flags
        eng = self.engine
        self._seq_var_x = None
        if hasattr(eng, "estep_sequence_subset") and not flags & L.USE_HOST_LLIKS:
            st, seq_lb, q0 = eng.estep_sequence_subset(idx, flags=flags)
            return st, float(st.lb[0]), q0
        so = self.seq_off
        total, lb, q0 = None, 0., np.zeros(self.K)
        for s in idx:
            off, ln = int(so[s]), int(so[s + 1] - so[s])
            if flags & L.USE_HOST_LLIKS:        # (labels clamped on the host: the sequence's slice of the [1, T, K] batch)
                eng.set_lliks(self._host_lliks[:, off:off + ln])
            st = eng.estep([off], ln, flags=flags)
            total = st.buf.copy() if total is None else total + st.buf
            lb += float(st.lb[0])
            q0 += eng.read_rows("var_x", 0, 1)[0]
        st = rewrap_packed(st, total)
        st.lb[0] = lb
        return st, lb, q0

    def _read_var_x(self):
        """``var_x`` [T, K] of the last fused E-step."""
        if self._multi() and self.__dict__.get("_seq_var_x") is not None:
            return self._seq_var_x
        return self.engine.read_intermediate("var_x", 1, self.T)[0]

    def _psi_expectations(self):
        """reference hmmbase.py:214-216."""
        self.mod_init = digamma(self.var_init + eps) - digamma(np.sum(self.var_init) + eps)
        tran_sum = np.sum(self.var_tran, axis=1)
        self.mod_tran = digamma(self.var_tran + eps) - digamma(tran_sum[:, npa] + eps)

    def _emission_arrays(self):
        ve = self.var_emit
        return (np.array([g.mu_mf for g in ve], dtype=np.float64),
                np.array([g.sigma_mf for g in ve], dtype=np.float64),
                np.array([float(g.kappa_mf) for g in ve]),
                np.array([float(g.nu_mf) for g in ve]))

    def _niw_fastpath(self):
        # (observations wider than the NIW kernels take go the generic route: lliks from the
        #  emitters' expected_log_likelihood on the host, recursions on the device)
        d = self.obs.shape[1] if self.obs.ndim == 2 else 1
        return d <= L.NIW_MAX_D and all(is_niw_gaussian(e) for e in self.var_emit)

    def _diag_fastpath(self):
        d = self.obs.shape[1] if self.obs.ndim == 2 else 1
        return (d <= L.DIAG_MAX_D and hasattr(self.engine, "set_emission_diag")
                and all(is_diag_gaussian(e) for e in self.var_emit))

    def _diag_arrays(self):
        ve = self.var_emit
        return tuple(np.array([getattr(g, n) for g in ve], dtype=np.float64)
                     for n in ("mf_mu", "mf_nus", "mf_alphas", "mf_betas"))

    def _cat_fastpath(self):
        """Categorical emissions over one integer-valued observation column (the device keeps
        the E log theta table and counts symbols; reference hmmsgd_metaobs.py:907-926)."""
        from .distributions import Categorical
        ve = self.var_emit
        return (all(type(e) is Categorical for e in ve)
                and len({e.num_parameters() for e in ve}) == 1
                and (self.obs.ndim == 1 or self.obs.shape[1] == 1))

    def _mcat_fastpath(self):
        """Multi-column Categorical emissions (``ProductCategorical``: D symbol columns, independent
        given the state) on an engine that has the family: the device keeps the D E log theta
        tables and counts symbols per column.  Other engines keep the host-lliks route."""
        from .distributions import ProductCategorical
        ve = self.var_emit
        if not all(type(e) is ProductCategorical for e in ve) or len(ve) < 1:
            return False
        V = ve[0].V
        return (all(e.V == V for e in ve)
                and self.obs.ndim == 2 and self.obs.shape[1] == len(V)
                and len(V) <= L.MCAT_MAX_D and sum(V) <= L.MCAT_MAX_F
                and hasattr(self.engine, "set_emission_mcat"))

    def _poisson_fastpath(self):
        """Poisson count emissions (``ProductPoisson``: D count columns, independent given the state) on
        an engine that has the family: the device keeps the (E log lambda, E lambda) tables and sums
        counts per column.  Other engines keep the host-lliks route."""
        from .distributions import ProductPoisson
        ve = self.var_emit
        if not all(type(e) is ProductPoisson for e in ve) or len(ve) < 1:
            return False
        D, C = ve[0].D, ve[0].max_count
        return (all(e.D == D and e.max_count == C for e in ve)
                and self.obs.ndim == 2 and self.obs.shape[1] == D
                and D <= L.POISSON_MAX_D and C <= L.POISSON_MAX_COUNT
                and hasattr(self.engine, "set_emission_poisson"))

    def _pgauss_fastpath(self):
        """Gaussian tracks with missing entries (``ProductGaussian``: D real-valued columns, independent
        given the state, single entries may be absent) on an engine that has the family: the device keeps
        the (mu, hprec, cst) tables and sums (r r, r, 1) per column about an origin.  Other engines keep the
        host-lliks route."""
        from .distributions import ProductGaussian
        ve = self.var_emit
        if not all(type(e) is ProductGaussian for e in ve) or len(ve) < 1:
            return False
        D = len(ve[0].mf_mu)
        return (all(len(e.mf_mu) == D for e in ve)
                and self.obs.ndim == 2 and self.obs.shape[1] == D and D <= L.PGAUSS_MAX_D
                and hasattr(self.engine, "set_emission_pgauss"))

    def _pgauss_origin(self):
        """Each column's mean over the present entries of the data, formed once per ``obs`` array: what the
        device takes the family's statistics about."""
        if getattr(self, "_pg_origin_obs", None) is not self.obs:
            self._pg_origin = self.var_emit[0].data_origin(self.obs)
            self._pg_origin_obs = self.obs
        return self._pg_origin

    def _family(self, among=FAMILIES):
        """The first record of ``among`` (hmmbase.FAMILIES, in its order) whose predicate holds for this model, or None:
        the predicates after it are not asked.  Labels on an engine that does not take them: None, so that no
        device family evaluates unclamped lliks (the host-lliks route clamps them)."""
        if self._labels_on_host():
            return None
        return next((f for f in among if getattr(self, f.pred)()), None)

    def _device_family(self):
        """Whether the device evaluates the emitters' family itself (no host lliks)."""
        return self._family() is not None

    # -- the device-resident SVI loop: what its class surfaces share -------------------------
    # (hmmsgd_metaobs.VBHMM on windows of one chain, hmmbatchsgd.VBHMM(seq_minibatch=M) on whole sequences)
    def _svi_family(self):
        """Emission family the device-resident loop runs for this model (None: host loop)."""
        f = self._family([f for f in FAMILIES if f.svi_method])
        return f and f.name

    def _svi_plain_vlb(self, fam):
        """The emitters' ``get_vlb`` is the family's own (the loop's ELBO kernels restate it)."""
        return all(type(e).get_vlb is FAMILY[fam].emitter.get_vlb for e in self.var_emit)

    def _svi_begin(self, fam, maxit):
        """Upload the transition factor and the family's prior / factors: the engine's ``svi_begin*``."""
        f = FAMILY[fam]
        getattr(self.engine, f.svi_method)(self.prior_tran, self.var_tran, *f.svi_args(self, maxit))

    def _svi_pull_state(self):
        """Device state -> the object's attributes (reference attribute names)."""
        fam = self._svi_family()
        if getattr(self, "adagrad", False):
            self.ada_G = self.engine.svi_read_adagrad()
        FAMILY[fam].svi_pull(self)

    def _prior_arrays(self):
        """Stacked NIW prior hyperparameters (mu_0 [K,D], sigma_0 [K,D,D], kappa_0 [K], nu_0 [K]).
        The priors of a model do not change after construction (the reference never writes
        them either), so they are stacked once per emitter array."""
        ve = self.var_emit
        key = (id(ve), len(ve))
        c = self.__dict__.get("_prior_stack")
        if c is None or c[0] != key:
            c = (key, np.array([g.mu_0 for g in ve]), np.array([g.sigma_0 for g in ve]),
                 np.array([float(g.kappa_0) for g in ve]), np.array([float(g.nu_0) for g in ve]))
            self._prior_stack = c
        return c[1:]

    def _emit_vlb(self):
        """sum_k var_emit[k].get_vlb() (reference hmmbase.py:183-185), batched for NIW
        Gaussians."""
        ve = self.var_emit
        if self._niw_fastpath() and all(type(e).get_vlb is Gaussian.get_vlb for e in ve):
            from .distributions import niw_vlb_batch
            mu, sg, ka, nu = self._emission_arrays()
            mu0, sg0, ka0, nu0 = self._prior_arrays()
            terms = None
            eng = self.engine
            if hasattr(eng, "niw_vlb_terms"):
                # log det / trace / quadratic form of sigma_mf from the device (it factorises
                # sigma_mf for the E-step anyway): the host-side batched solve of K D x D systems
                # costs more than the device E-step of a 64-window minibatch
                key = (id(self), id(ve), mu0.shape)      # the engine's prior copy belongs to one model
                if getattr(eng, "_prior_owner", None) != key:
                    eng.set_emission_prior(mu0, sg0)
                    eng._prior_owner = key
                terms = eng.niw_vlb_terms(mu, sg, ka, nu)
            return float(np.sum(niw_vlb_batch(
                mu, sg, ka, nu, mu0, sg0, ka0, nu0, terms=terms)))
        tot = 0.
        for k in range(self.K):
            tot += ve[k].get_vlb()
        return tot

    def _push_globals(self):
        self.engine.set_globals(self.mod_init, self.mod_tran)

    def _push_emission(self, windows=None, Lm=None, nan_mask=False):
        """Make the emission log-likelihoods available on the device.

        NIW Gaussians: upload the K mean-field factors, lliks are evaluated by the
        emission kernel.  Any other plugin object: evaluate
        ``expected_log_likelihood`` on the host (reference hmmbase.py:219-220) and
        upload ``lliks``.  Returns the flag word for the engine calls."""
        f = self._family()
        if f is not None:
            f.push(self, self.engine)
            return L.MASK_AS_NAN if nan_mask else 0
        obs = self.obs if self.obs.ndim == 2 else self.obs[:, None]
        if windows is None:
            windows, Lm = [0], self.T
        ll = np.empty((len(windows), Lm, self.K))
        for b, s in enumerate(windows):
            x = obs[s:s + Lm]
            if nan_mask:
                x = x.copy()
                x[self.mask[s:s + Lm]] = np.nan
            for k, odist in enumerate(self.var_emit):
                ll[b, :, k] = np.nan_to_num(odist.expected_log_likelihood(x))
        self._clamp_lliks(ll, windows, Lm)
        self.engine.set_lliks(ll)
        self._host_lliks = ll
        return L.USE_HOST_LLIKS

    # -- ELBO ------------------------------------------------------------------------
    def lower_bound(self):
        """ Variational lower bound (reference hmmbase.py:145-199)."""
        # E_q[log p] - E_q[log q] of the Dirichlet factors (initial distribution, transition rows)
        pi_term = dirichlet_elbo(self.prior_init[None, :], self.var_init[None, :])
        A_term = dirichlet_elbo(self.prior_tran, self.var_tran)

        emit_vlb = self._emit_vlb()

        # "log Z" = sum over ALL t of LSE_k lalpha[t,k] (quirk Q4, hmmbase.py:194);
        # reduced on the device with the posterior kernel when available
        if self._lZ is not None:
            lZ = self._lZ
        else:
            lZ = np.sum(np.logaddexp.reduce(self.lalpha, axis=1))

        return pi_term + A_term + emit_vlb + lZ

    # -- E-step ------------------------------------------------------------------------
    def local_update(self, obs=None, mask=None):
        """Batch local update (reference hmmbase.py:201-229) on the device.
        Afterwards ``lliks, lalpha, lbeta, var_x, mod_init, mod_tran`` hold host
        arrays of shape [T,K] / [K] / [K,K]."""
        if obs is not None or mask is not None:
            self.set_data(self.obs if obs is None else obs,
                          self.mask if mask is None else mask)
        if self._multi():
            # every sequence from mod_init, nothing across a join: one device call, then the rows
            _, self._lZ, _ = self._sequences_estep()
            self._fetch_local()
            return
        self._psi_expectations()
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission()
        if (type(self).forward_msgs is not VariationalHMMBase.forward_msgs
                or type(self).backward_msgs is not VariationalHMMBase.backward_msgs):
            # a subclass replaced the message passes ("Override this for specialized behavior",
            # reference hmmbase.py:279,304): follow the reference's sequence literally
            self._local_update_literal([0], self.T, flags)
            return
        r = self.engine.forward_backward([0], self.T, flags=flags)
        self.lalpha = r["lalpha"][0]
        self.lbeta = r["lbeta"][0]
        self.var_x = r["var_x"][0]
        self._lZ = float(r["local_lb"][0])
        self.lliks = self.engine.read_intermediate("lliks", 1, self.T)[0]

    def _local_update_literal(self, starts, Lm, flags, metaobs=None):
        """lliks from the engine (or the uploaded host lliks), then ``self.forward_msgs()`` /
        ``self.backward_msgs()`` as overridable hooks, posterior on the host
        (reference hmmbase.py:219-229)."""
        if flags & L.USE_HOST_LLIKS:
            self.lliks = self._host_lliks[0]
        else:
            self.lliks = self.engine.loglik(starts, Lm, flags=flags)[0]
        if metaobs is None:
            self.forward_msgs()
            self.backward_msgs()
        else:
            self.forward_msgs(metaobs)
            self.backward_msgs(metaobs)
        v = self.lalpha + self.lbeta
        v = v - np.max(v, axis=1)[:, npa]
        v = np.exp(v)
        self.var_x = v / np.sum(v, axis=1)[:, npa]
        self._lZ = None

    def forward_msgs(self, obs=None, mask=None):
        """lalpha from ``self.lliks, self.mod_init, self.mod_tran``
        (reference hmmbase.py:266-295)."""
        self.engine.set_globals(self.mod_init, self.mod_tran)
        self.engine.set_lliks(np.ascontiguousarray(self.lliks)[None])
        r = self.engine.forward_backward(None, self.lliks.shape[0], flags=L.USE_HOST_LLIKS,
                                         want=("lalpha", "local_lb"), B=1)
        self.lalpha = r["lalpha"][0]
        self._lZ = float(r["local_lb"][0])

    def backward_msgs(self, obs=None, mask=None):
        """lbeta (reference hmmbase.py:297-320)."""
        self.engine.set_globals(self.mod_init, self.mod_tran)
        self.engine.set_lliks(np.ascontiguousarray(self.lliks)[None])
        r = self.engine.forward_backward(None, self.lliks.shape[0], flags=L.USE_HOST_LLIKS,
                                         want=("lbeta",), B=1)
        self.lbeta = r["lbeta"][0]

    def _batch_estep_stats(self):
        """Whole-chain E-step + expected sufficient statistics on the device, batch
        transition form (hmmbatchcd.py:182-184): used by the batch infer() loops so
        that only O(K^2 + K D^2) numbers cross PCIe per iteration."""
        if self._multi():
            st, self._lZ, self._q0 = self._sequences_estep()
            return st
        self._psi_expectations()
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission()
        st = self.engine.estep([0], self.T, flags=flags)  # no TRANS_WRAP: t=1..T-1
        self._lZ = float(st.lb[0])
        self._q0 = self.engine.read_rows("var_x", 0, 1)[0]
        return st

    def _batch_stats_route(self, literal_global_update, families=("niw", "diag", "cat", "mcat", "poisson", "pgauss")):
        """Whether the host loop of a batch class (a ``local_update`` override, or
        ``infer(fused=False)``) may take the statistics of ``self.var_x`` on the device instead of
        the literal ``global_update``: only where that method is the class's own and the engine and
        the emission family have device statistics."""
        if "global_update" in self.__dict__ or type(self).global_update is not literal_global_update:
            return False
        if not hasattr(self.engine, "suffstats"):
            return False
        return self._family([FAMILY[f] for f in families]) is not None

    def _batch_suffstats(self):
        """Statistics of the host posteriors ``self.var_x`` (whatever ``local_update`` left there)
        over the whole chain on the device, batch transition form (hmmbatchcd.py:182-184): what
        ``_batch_estep_stats`` returns, for the same ``_global_update_from_stats``."""
        self._upload_obs()
        self._push_globals()
        self._push_emission()
        q = np.asarray(self.var_x, dtype=np.float64)
        self._q0 = q[0].copy()
        return self.engine.suffstats([0], self.T, q[None], flags=0)

    def _fetch_local(self):
        """Pull the per-time-step arrays of the last device E-step to the host
        attributes (documented reference attributes)."""
        T = self.T
        if self._multi():
            # var_x from the concatenated read-back, the messages sequence by sequence (the engine
            # still holds the globals and emission factors of the last E-step)
            eng, so = self.engine, self.seq_off
            self.var_x = self._read_var_x()
            self.lliks, self.lalpha, self.lbeta = (np.empty((T, self.K)) for _ in range(3))
            for s in range(len(so) - 1):
                off, ln = int(so[s]), int(so[s + 1] - so[s])
                if self._seq_flags & L.USE_HOST_LLIKS:
                    eng.set_lliks(self._host_lliks[:, off:off + ln])
                r = eng.forward_backward([off], ln, flags=self._seq_flags, want=("lalpha", "lbeta"))
                self.lalpha[off:off + ln] = r["lalpha"][0]
                self.lbeta[off:off + ln] = r["lbeta"][0]
                self.lliks[off:off + ln] = eng.read_intermediate("lliks", 1, ln)[0]
            return
        self.lliks = self.engine.read_intermediate("lliks", 1, T)[0]
        self.lalpha = self.engine.read_intermediate("lalpha", 1, T)[0]
        self.lbeta = self.engine.read_intermediate("lbeta", 1, T)[0]
        self.var_x = self.engine.read_intermediate("var_x", 1, T)[0]

    def pred_logprob(self):
        """Mean predictive log-probability of the masked data
        (reference hmmbase.py:322-340)."""
        K = self.K
        obs = self.obs
        mask = self.mask
        nmiss = np.sum(mask)
        if nmiss == 0:
            return None
        logprob = np.zeros((nmiss, K))
        for k, odist in enumerate(self.var_emit):
            logprob[:, k] = (np.log(self.var_x[mask, k] + eps)
                             + odist.expected_log_likelihood(obs[mask, :]))
        return np.mean(np.logaddexp.reduce(logprob, axis=1))

    def full_local_update(self):
        self.local_update()
        return self.var_x

    def _full_estep_device(self):
        """Whole-chain E-step whose per-row results stay in HBM (for hamming_dist(None, ...))."""
        if self._multi():
            self._sequences_estep()
            return
        self._psi_expectations()
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission()
        self.engine.forward_backward([0], self.T, flags=flags, want=())

    # -- held-out scores on the device ----------------------------------------------------
    def _heldout_family(self):
        """Emission family of the emitters as far as their types say (no engine is touched):
        "niw", "diag", "cat", "mcat", "poisson", "pgauss" or None."""
        return next((f.name for f in FAMILIES if f.by_type(self)), None)

    def _heldout_estep(self, what):
        """The full E-step the held-out scores are taken against: the class's own ``_full_estep_device``
        (the E-step of its ``full_local_update``: the whole chain, or every sequence from ``mod_init`` in
        one device call; per-row results stay in HBM).  What that call writes on the way -- the
        psi-expectations and the sequence bookkeeping -- is put back: no attribute of the model changes."""
        if not self._device_family():
            raise NotImplementedError("%s: the emitters are of a family this engine does not evaluate on the "
                                      "device (the held-out kernels score against device lliks)" % what)
        if not hasattr(self.engine, "heldout_rows"):
            raise NotImplementedError("%s: this engine has no held-out kernels (heldout_rows / heldout_entries); "
                                      "pred_logprob is the host route" % what)
        names = ("mod_init", "mod_tran", "_seq_flags", "_seq_var_x", "_lZ")
        none = object()
        keep = {n: self.__dict__.get(n, none) for n in names}
        try:
            self._full_estep_device()
        finally:
            for n, v in keep.items():
                if v is none:
                    self.__dict__.pop(n, None)
                else:
                    self.__dict__[n] = v
        return self.engine

    def heldout_logprob(self):
        """Mean predictive log-probability of the masked rows, the value ``pred_logprob_full`` defines
        (``mean_t LSE_k(log(var_x[t, k] + 1e-9) + E_q log p(x_t | k))`` over the masked rows ``t``, ``var_x``
        from the class's ``full_local_update`` E-step: ``hmmsgd_metaobs`` treats the masked rows as missing
        there, the batch classes follow the reference's batch ``local_update``, which does not look at the
        mask), computed on the device for every device family
        (NIW, diagonal Gaussian, Categorical, ``ProductCategorical``, ``ProductPoisson``, ``ProductGaussian``) and
        for a list
        ``obs`` (every sequence from ``mod_init``, one device call): two doubles cross the bus instead of
        ``var_x[T, K]``.  ``None`` without masked rows.  No attribute of the model changes.  Emitters without
        a device family raise ``NotImplementedError``."""
        if self._heldout_family() is None:
            raise NotImplementedError("heldout_logprob: the emitters have no device family (NIW / diagonal "
                                      "Gaussian, Categorical, ProductCategorical, ProductPoisson, ProductGaussian): their lliks "
                                      "are evaluated on the host, use pred_logprob")
        if not np.any(self.mask):
            return None
        val, _ = self._heldout_estep("heldout_logprob").heldout_rows()
        return val

    def heldout_entries_logprob(self, rows, cols, vals, per_entry=False):
        """Entry-wise ("speckled") held-out score of a ``ProductCategorical`` / ``ProductPoisson`` /
        ``ProductGaussian`` model: the entries ``(rows[e], cols[e])`` of ``obs`` (rows numbered over the concatenation when ``obs`` was a
        list) were blanked -- set NaN, ``util.speckle_holdout`` -- before fitting; ``vals[e]`` is what stood
        there.  Full E-step on the blanked data (the one ``heldout_logprob`` runs), then
        ``lp_e = LSE_k(log(var_x[rows[e], k] + 1e-9) + E_q log p(vals[e] | k, column cols[e]))`` on the device:
        the mean over the entries whose value is present under the family's rule (``None`` if there is none),
        with ``per_entry`` ``(mean, lp[n])`` (NaN for the skipped ones).  ``ValueError`` unless every
        ``obs[rows, cols]`` is NaN; ``NotImplementedError`` for other emitters (a NaN entry of a ``Gaussian`` or
        ``DiagonalGaussian`` row blanks the whole row).  No attribute of the model changes."""
        f = FAMILY.get(self._heldout_family())
        if f is None or f.heldout != "entries":
            raise NotImplementedError("heldout_entries_logprob: entry-wise scores need ProductGaussian, "
                                      "ProductCategorical or ProductPoisson emitters (columns independent given the state); other "
                                      "families have no per-entry missingness")
        r = np.asarray(rows, dtype=np.int64).ravel()
        c = np.asarray(cols, dtype=np.int64).ravel()
        v = np.asarray(vals, dtype=np.float64).ravel()
        if not (len(r) == len(c) == len(v)):
            raise ValueError("heldout_entries_logprob: rows, cols and vals must have one length")
        obs = self.obs if self.obs.ndim == 2 else self.obs[:, None]
        if len(r) and (r.min() < 0 or r.max() >= obs.shape[0] or c.min() < 0 or c.max() >= obs.shape[1]):
            raise ValueError("heldout_entries_logprob: an entry lies outside obs %s" % (obs.shape,))
        seen = obs[r, c]
        if not np.all(np.isnan(seen)):
            e = int(np.flatnonzero(~np.isnan(seen))[0])
            raise ValueError("heldout_entries_logprob: obs[%d, %d] = %r is not blanked (entry %d): the posterior "
                             "would have seen the value it is scored on" % (r[e], c[e], float(seen[e]), e))
        eng = self._heldout_estep("heldout_entries_logprob")
        res = eng.heldout_entries(r, c, v, resident=True, want_lp=per_entry)
        if not per_entry:
            return res[0]
        return res[0], (res[2] if len(r) else np.empty(0))

    # -- posterior expectations of per-state tables ----------------------------------------
    def _expect_engine(self):
        """The engine, where ``posterior_expect`` can run on the device: it has the two calls and the posterior
        batch it holds is this model's whole-chain / all-sequences E-step (the batch ``var_x`` is read from after
        ``infer()`` of the batch classes and after ``full_local_update()``); else None.  No engine is created."""
        eng = self.__dict__.get("_engine")
        if eng is None or not callable(getattr(eng, "posterior_expect", None)) \
                or not callable(getattr(eng, "posterior_expect_entries", None)):
            return None
        if getattr(eng, "_obs_owner", None) != id(self):
            return None
        held, T = getattr(eng, "_held", None), self.obs.shape[0]
        if held is None or int(getattr(eng, "_rows", 0)) != T:
            return None
        whole = held[0] == "sequences" or (held[0] == "windows" and len(held[1]) == 1 and int(held[1][0]) == 0
                                           and int(held[2]) == T)
        return eng if whole else None

    def _expect_route(self, device_call, prepare):
        """``(device result or None, var_x for the host route or None for self.var_x)``.  ``prepare``: the caller needs
        posteriors of all rows (``_expect_prepare``).  A call the engine refuses because it holds no posterior batch
        any more -- a decoder, ``loglik`` or a new upload ran since the E-step, which the engine's own note of the
        batch does not record -- clears that note and, with ``prepare``, prepares again: a class whose ``var_x`` does
        not cover the rows then averages a fresh whole-chain E-step, never a stale or shorter ``self.var_x``."""
        var_x = self._expect_prepare() if prepare else None
        eng = self._expect_engine()
        if eng is None:
            return None, var_x
        try:
            return device_call(eng), None
        except RuntimeError as e:
            if "no posterior batch held" not in str(e):
                raise
        eng._held = None
        if prepare:
            var_x = self._expect_prepare()
            eng = self._expect_engine()
            if eng is not None:
                return device_call(eng), None
        return None, var_x

    def _posterior_expect(self, t, prepare=False):
        out, var_x = self._expect_route(lambda eng: eng.posterior_expect(t), prepare)
        if out is None:
            out = np.asarray(self.var_x if var_x is None else var_x, dtype=np.float64) @ t
        so = self.__dict__.get("seq_off")
        if so is not None and out.shape[0] == int(so[-1]):
            return [out[int(so[s]):int(so[s + 1])] for s in range(len(so) - 1)]
        return out

    def _posterior_expect_entries(self, t, rows, cols, prepare=False):
        r = np.asarray(rows, dtype=np.int64).ravel()
        c = np.asarray(cols, dtype=np.int64).ravel()
        if len(r) != len(c):
            raise ValueError("posterior_expect_entries: rows and cols must have one length")
        out, var_x = self._expect_route(lambda eng: eng.posterior_expect_entries(t, r, c), prepare)
        if out is not None:
            return out
        q = np.asarray(self.var_x if var_x is None else var_x, dtype=np.float64)
        if len(r) and (r.min() < 0 or r.max() >= q.shape[0] or c.min() < 0 or c.max() >= t.shape[1]):
            raise ValueError("posterior_expect_entries: an entry lies outside [0, %d) x [0, %d)"
                             % (q.shape[0], t.shape[1]))
        # the device's order: k ascending from 0.0, every product and every sum rounded on its own
        out = np.zeros(len(r))
        for k in range(self.K):
            out = out + q[r, k] * t[k, c]
        return out

    def posterior_expect(self, table):
        """Posterior expectation of a per-state table: ``out[t, f] = sum_k var_x[t, k] table[k, f]``, ``[rows, F]``.
        ``table`` is a ``[K, F]`` float64 array of any finite values (a ``[K]`` array counts as ``F = 1``).  On an
        engine that has ``posterior_expect`` and holds this model's whole-chain posterior batch -- after ``infer()``
        of the batch classes on one chain, after ``full_local_update()`` -- the product is formed on the device
        against the rows in HBM (``svihmm_posterior_expect``) and only ``[rows, F]`` crosses the bus; otherwise it is
        ``self.var_x @ table`` in NumPy.  When ``obs`` was a list the result is a list of per-sequence arrays.

        The device averages the batch the engine HOLDS.  After ``infer()`` and ``full_local_update()`` that is the
        batch ``var_x`` was read from, and both routes see the same bits.  A later whole-chain E-step that sets no
        attribute (``heldout_logprob()``, ``hamming_dist(None, ..)``) under changed parameters replaces the batch
        held and leaves ``self.var_x``: the device route then answers for the newer posteriors, the NumPy route for
        ``self.var_x``.  ``local_update()`` brings the two together again."""
        return self._posterior_expect(L.as_state_table(table, self.K, "posterior_expect"))

    def posterior_expect_entries(self, table, rows, cols):
        """``out[e] = sum_k var_x[rows[e], k] table[k, cols[e]]`` for a list of single (row, table column) pairs,
        ``[n]``; rows are numbered over the concatenation when ``obs`` was a list, as ``heldout_entries_logprob``
        numbers them.  Device or NumPy as ``posterior_expect`` chooses; both add ``k`` ascending with every product
        and sum rounded on its own, so they agree bit for bit."""
        return self._posterior_expect_entries(L.as_state_table(table, self.K, "posterior_expect_entries"), rows, cols)

    def _expect_family_table(self, who):
        """``(family name, table [K, F])`` of the per-state means ``reconstruct()`` averages, by the emitters' types."""
        fam = self._heldout_family()
        ve = self.var_emit
        if fam is None and len(ve) and all(is_niw_gaussian(e) for e in ve):
            fam = "niw"                     # (rows wider than the device's NIW kernels take: the table is the same)
        if fam == "niw":
            tab = [np.ravel(e.mu_mf) for e in ve]
        elif fam in ("diag", "pgauss"):
            tab = [np.ravel(e.mf_mu) for e in ve]
        elif fam == "poisson":
            tab = [np.ravel(e.alpha_mf) / np.ravel(e.beta_mf) for e in ve]
        elif fam == "cat":
            tab = [np.ravel(e.alpha_mf) / np.sum(e.alpha_mf) for e in ve]
        elif fam == "mcat":
            tab = [np.concatenate([np.ravel(a) / np.sum(a) for a in e.alpha_mf]) for e in ve]
        else:
            raise NotImplementedError("%s: emitters of type %s have no table of per-state means known here; build "
                                      "the [K, F] table yourself and call posterior_expect(table)"
                                      % (who, type(ve[0]).__name__ if len(ve) else None))
        return fam, np.array(tab, dtype=np.float64)

    def _expect_prepare(self):
        """Posteriors of all the model's rows: ``var_x`` to average where the device does not hold them (None:
        ``self.var_x``).  The batch classes have them after ``infer()``; ``hmmsgd_metaobs.VBHMM`` overrides this."""
        return None

    def reconstruct(self):
        """Posterior mean of every observation column, the smoothed / denoised signal
        ``xhat[t, d] = sum_k var_x[t, k] mean[k, d]`` through ``posterior_expect``: the table is ``mu_mf``
        (``Gaussian``), ``mf_mu`` (``DiagonalGaussian`` / ``ProductGaussian``), ``alpha_mf / beta_mf`` (the expected
        rates of ``ProductPoisson``) or, for ``Categorical`` / ``ProductCategorical``, the predictive symbol
        probabilities ``alpha / alpha.sum()`` of the columns side by side (``[T, sum V_d]``, the columns' blocks in
        ascending ``d``).  Needs posteriors for all the model's rows: after ``infer()`` of the batch classes that
        holds; ``hmmsgd_metaobs.VBHMM``, whose last batch is a minibatch of windows, runs ``full_local_update()``
        first when the batch held does not cover the T rows.  Other emitters raise ``NotImplementedError``."""
        _, t = self._expect_family_table("reconstruct")
        return self._posterior_expect(t, prepare=True)

    def impute(self):
        """A copy of the data in which every absent entry is replaced by its posterior mean
        (``posterior_expect_entries`` on the family's table of means); present entries come back bit-identical.
        Absent: NaN for ``Gaussian`` / ``DiagonalGaussian``, not ``_present()`` for ``ProductGaussian`` and
        ``ProductPoisson``.  Masked rows are not special: their present entries stay, their absent ones are filled.
        A list ``obs`` comes back as a list.  The symbol families raise ``NotImplementedError``: a mean symbol is
        not a symbol, ``reconstruct()`` gives the predictive probabilities.  Needs what ``reconstruct()`` needs."""
        fam, t = self._expect_family_table("impute")
        if fam in ("cat", "mcat"):
            raise NotImplementedError("impute: symbol columns have no mean to fill in; reconstruct() returns the "
                                      "predictive symbol probabilities of every row")
        x = np.asarray(self.obs)
        x2 = x.reshape(x.shape[0], -1)
        if fam in ("pgauss", "poisson"):
            absent = ~self.var_emit[0]._present(x2)[1]
        else:
            absent = np.isnan(np.asarray(x2, dtype=np.float64))
        rows, cols = np.nonzero(absent)
        out = np.array(x2, dtype=x2.dtype if np.issubdtype(x2.dtype, np.floating) else np.float64)
        out[rows, cols] = self._posterior_expect_entries(t, rows, cols, prepare=True)
        out = out.reshape(x.shape)
        so = self.__dict__.get("seq_off")
        if so is not None:
            return [out[int(so[s]):int(so[s + 1])] for s in range(len(so) - 1)]
        return out

    # -- Viterbi / MAP path -------------------------------------------------------------
    def viterbi(self, metaobs=None):
        """Most probable state sequence of the whole chain (or of one meta-observation
        ``metaobs``: rows ``i1 .. i2``) under the current variational parameters, decoded on the
        device: ``(z int32[Lm], score)``.  Same psi-expectations and missing-data convention as
        ``full_local_update`` (masked rows contribute ``lliks = 0``); emission plugins without a
        device family are evaluated on the host and uploaded (``set_lliks``).  No attribute of the
        model changes.  ``argmax(var_x, axis=1)`` remains the decode of ``hamming_dist``; for the
        same metric on the MAP path: ``util.munkres_match(true_sts, z, K)``.

        Several sequences (``obs`` was a list) and ``metaobs=None``: every sequence is decoded on its
        own, from ``mod_init`` at its first row, all in ONE device call (``viterbi_sequences``):
        ``(list of z_s int32[T_s], score float64[N])``."""
        if metaobs is None and self._multi():
            return self._viterbi_sequences()
        loff, uoff = (0, self.T - 1) if metaobs is None else (metaobs.i1, metaobs.i2)
        Lm = uoff - loff + 1
        mod_init = digamma(self.var_init + eps) - digamma(np.sum(self.var_init) + eps)
        tran_sum = np.sum(self.var_tran, axis=1)
        mod_tran = digamma(self.var_tran + eps) - digamma(tran_sum[:, npa] + eps)
        self._upload_obs()
        self.engine.set_globals(mod_init, mod_tran)
        flags = self._push_emission(windows=[loff], Lm=Lm, nan_mask=True)
        z, score = self.engine.viterbi([loff], Lm, flags=flags)
        return z[0], float(score[0])

    def _split_sequences(self, a):
        """Views of the last axis of ``a`` (resident rows) per sequence."""
        so = self.seq_off
        return [a[..., int(so[s]):int(so[s + 1])] for s in range(len(so) - 1)]

    def _viterbi_sequences(self):
        mod_init = digamma(self.var_init + eps) - digamma(np.sum(self.var_init) + eps)
        tran_sum = np.sum(self.var_tran, axis=1)
        mod_tran = digamma(self.var_tran + eps) - digamma(tran_sum[:, npa] + eps)
        self._upload_obs()
        eng = self.engine
        eng.set_globals(mod_init, mod_tran)
        # (a plugin without a device family: its lliks of the concatenated rows as one [1, T, K] batch)
        flags = self._push_emission(windows=[0], Lm=self.T, nan_mask=True)
        if hasattr(eng, "viterbi_sequences"):
            z, score = eng.viterbi_sequences(flags=flags)
            return [np.array(v) for v in self._split_sequences(z)], np.array(score, dtype=np.float64)
        zs, score = [], np.empty(len(self.seq_off) - 1)
        for s, (off, end) in enumerate(zip(self.seq_off[:-1], self.seq_off[1:])):
            off, ln = int(off), int(end - off)
            if flags & L.USE_HOST_LLIKS:
                eng.set_lliks(self._host_lliks[:, off:off + ln])
            z, sc = eng.viterbi([off], ln, flags=flags)
            zs.append(z[0])
            score[s] = sc[0]
        return zs, score

    # -- FFBS (reference hmm_fast.pyx:43-124, bound at hmmbase.py:409-411) ---------------
    def ffbs_fast(self, var_init, lalpha_init=None, uniforms=None):
        """Forward-filter backward-sample.  Returns ``(z int64[T], lalpha[T,K])``.

        Follows the Cython variant: ``DBL_EPSILON`` instead of 1e-9 and transitions
        ``log(var_tran + DBL_EPSILON)`` (un-normalised; quirk Q6).  ``uniforms`` (one
        per time step) replaces libc ``rand()``, which cannot be reproduced on a
        device; default draws them from ``np.random``."""
        var_init = np.asarray(var_init, dtype=np.float64)
        A = self.var_tran
        mod_init = digamma(var_init + DBL_EPSILON) - digamma(np.sum(var_init) + DBL_EPSILON)
        logA = np.log(A + DBL_EPSILON)
        if uniforms is None:
            uniforms = np.random.random_sample(self.T)
        if lalpha_init is not None:
            # backward sampling only, from the supplied messages (hmm_fast.pyx:80-95: neither
            # the likelihoods nor the filter run; lalpha_init itself is returned)
            lalpha_init = np.asarray(lalpha_init, dtype=np.float64)
            if lalpha_init.shape != (self.T, self.K):
                raise RuntimeError("lalpha_init must have shape (T, K)")
            return self.engine.ffbs_sample(lalpha_init, logA, uniforms), lalpha_init
        self._upload_obs()
        self.engine.set_globals(mod_init, logA)
        flags = self._push_emission()
        z, lalpha = self.engine.ffbs(logA, uniforms, flags=flags)
        return z, lalpha

    def ffbs_windows(self, metaobs=None, n_draws=1, var_init=None, uniforms=None, seed=None):
        """``n_draws`` FFBS state paths of one meta-observation, of a list of equal-length ones, or
        (``metaobs=None``) of the whole chain, all from ONE forward filter on the device:
        ``z int32[n_draws, B, Lm]``.  Conventions of ``ffbs_fast`` (quirk Q6): ``var_init`` (default
        ``self.var_init``) through digamma with ``DBL_EPSILON``, ``log(var_tran + DBL_EPSILON)`` as
        the filter's transition and the sampler's; emission plugins without a device family are
        evaluated on the host (``set_lliks``), as in ``viterbi()``.  ``uniforms`` [n_draws, B, Lm]
        replace the device's counter-based generator, whose ``seed`` otherwise comes from
        ``np.random`` (so ``np.random.seed`` makes the draws reproducible).  No attribute of the
        model changes.

        Several sequences (``obs`` was a list) and ``metaobs=None``: ``n_draws`` paths of every
        sequence, each filtered from ``mod_init`` at its own first row, all from ONE device call
        (``ffbs_sequences``): a list of ``int32[n_draws, T_s]`` arrays.  ``uniforms`` is then
        ``[n_draws, T]`` over the concatenated rows."""
        if metaobs is None and self._multi():
            return self._ffbs_sequences(n_draws, var_init, uniforms, seed)
        if metaobs is None:
            wins = [(0, self.T - 1)]
        elif isinstance(metaobs, (list, tuple)):
            wins = [(m.i1, m.i2) for m in metaobs]
        else:
            wins = [(metaobs.i1, metaobs.i2)]
        if not wins:
            raise RuntimeError("ffbs_windows: no meta-observation given")
        Lm = wins[0][1] - wins[0][0] + 1
        if any(u - l + 1 != Lm for l, u in wins):
            raise RuntimeError("ffbs_windows: the meta-observations must have equal lengths")
        starts = [l for l, _ in wins]
        var_init = np.asarray(self.var_init if var_init is None else var_init, dtype=np.float64)
        mod_init = digamma(var_init + DBL_EPSILON) - digamma(np.sum(var_init) + DBL_EPSILON)
        logA = np.log(self.var_tran + DBL_EPSILON)
        if uniforms is None and seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
        self._upload_obs()
        self.engine.set_globals(mod_init, logA)
        flags = self._push_emission(windows=starts, Lm=Lm)
        z, _ = self.engine.ffbs_windows(starts, Lm, logA, n_draws=n_draws, uniforms=uniforms,
                                        seed=0 if seed is None else seed, flags=flags)
        return z

    def _ffbs_sequences(self, n_draws, var_init, uniforms, seed):
        var_init = np.asarray(self.var_init if var_init is None else var_init, dtype=np.float64)
        mod_init = digamma(var_init + DBL_EPSILON) - digamma(np.sum(var_init) + DBL_EPSILON)
        logA = np.log(self.var_tran + DBL_EPSILON)
        if uniforms is None and seed is None:
            seed = int(np.random.randint(0, 2 ** 31 - 1)) * 2 ** 31 + int(np.random.randint(0, 2 ** 31 - 1))
        self._upload_obs()
        eng = self.engine
        eng.set_globals(mod_init, logA)
        flags = self._push_emission(windows=[0], Lm=self.T)
        seed = 0 if seed is None else seed
        if hasattr(eng, "ffbs_sequences"):
            z, _ = eng.ffbs_sequences(logA, n_draws=n_draws, uniforms=uniforms, seed=seed, flags=flags)
            return [np.array(v) for v in self._split_sequences(z)]
        if uniforms is None:
            raise RuntimeError("ffbs_windows on several sequences: this engine has no ffbs_sequences; "
                               "pass uniforms [n_draws, T] to sample sequence by sequence")
        u = np.asarray(uniforms, dtype=np.float64).reshape(int(n_draws), self.T)
        out = []
        for off, end in zip(self.seq_off[:-1], self.seq_off[1:]):
            off, ln = int(off), int(end - off)
            if flags & L.USE_HOST_LLIKS:
                eng.set_lliks(self._host_lliks[:, off:off + ln])
            z, _ = eng.ffbs_windows([off], ln, logA, n_draws=n_draws, uniforms=u[:, None, off:off + ln], flags=flags)
            out.append(z[:, 0])
        return out

    # -- metrics (host) ----------------------------------------------------------------
    def hamming_dist(self, full_var_x, true_sts):
        """Hamming distance after the best label permutation (reference hmmbase.py:346-365).
        ``full_var_x=None``: the whole-chain E-step, the arg-max and the K x K count matrix
        run on the device and only the labels cross the bus (T = 1e6, K = 64: 4 MB instead
        of the 512 MB of var_x); the distance follows from the counts."""
        if full_var_x is None and self._multi() and not hasattr(self.engine, "estep_sequences"):
            full_var_x = self.full_local_update()      # (no device call that decodes all sequences)
        if full_var_x is None:
            true_sts = np.asarray(true_sts).ravel()
            self._full_estep_device()
            _, DM = self.engine.state_argmax(true_sts, want_z=False)
            best_match = util.match_from_counts(DM)
            hit = DM[np.arange(self.K), best_match].sum()
            return 1.0 - hit / float(true_sts.size), best_match
        state_sq = np.argmax(full_var_x, axis=1).astype(int)
        best_match = util.munkres_match(true_sts, state_sq, self.K)
        return dist.hamming(true_sts, best_match[state_sq]), best_match

    def KL_L2_gaussian(self, emit_true, permutation):
        """Evaluation metric (reference hmmbase.py:364-390): for every learned state ``k2`` paired
        with the true state ``k = permutation[k2]``, KL(N(learned) || N(true)) summed, and the
        summed L2 distance of the means."""
        kl_total = 0.
        l2_total = 0.
        for k2 in range(len(permutation)):
            tru, fit = emit_true[permutation[k2]], self.var_emit[k2]
            d = np.asarray(tru.mu) - np.asarray(fit.mu)
            l2_total += npl.norm(d)
            St, Sf = np.asarray(tru.sigma), np.asarray(fit.sigma)
            kl_total += .5 * (np.trace(npl.solve(St, Sf)) + d.dot(npl.solve(St, d)) - d.shape[0]
                              - (npl.slogdet(Sf)[1] - npl.slogdet(St)[1]))
        return kl_total, l2_total

    def A_dist(self, A_true, perm):
        A = self.var_tran / np.sum(self.var_tran, axis=1)[:, np.newaxis]
        A_true = A_true[np.ix_(perm, perm)]
        return npl.norm(A_true - A)
