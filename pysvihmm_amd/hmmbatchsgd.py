"""Batch natural-gradient VB -- class surface of reference ``hmmbatchsgd.py``.
Full-data E-step on the MI355X each iteration, Robbins-Monro natural-gradient
M-step on the host (hmmbatchsgd.py:202-259).  With ``seq_minibatch=M`` on a list of sequences: stochastic
variational inference over whole sequences -- the E-step of M sampled sequences per iteration, their
statistics scaled by ``batchfactor = N / M`` (the factor hmmbatchsgd.py:120-123 names and never sets)."""
from __future__ import division

import sys
import time

import numpy as np

from .hmmbase import FAMILY, VariationalHMMBase, is_niw_gaussian, is_diag_gaussian
from .distributions import ProductCategorical, ProductPoisson, ProductGaussian
from .engine import rewrap_packed
from . import util
from . import _lib as L

eps = 1e-9
tau0 = 1.
kappa0 = 0.7


class VBHMM(VariationalHMMBase):
    """Same constructor as reference hmmbatchsgd.py:64-66.

    ``seq_minibatch`` (default None: every iteration is a pass over all rows, as in the reference).  An integer
    ``M`` needs ``obs`` to be a list of ``N >= 2`` sequences and ``1 <= M <= N`` (``RuntimeError`` otherwise).
    Each iteration of ``infer()`` then draws ``idx = np.sort(np.random.choice(N, size=M, replace=False))`` from the
    global ``np.random`` stream, sets ``batchfactor = N / M``, runs the E-step of the drawn sequences only (one
    ``estep_sequence_subset`` device call) and takes the natural-gradient step on their statistics times
    ``batchfactor``: ``var_init`` is blended like the other factors, ``elbo_vec[it]`` is the usual noisy
    estimate (``batchfactor`` times the minibatch's local bound), ``pred_logprob_mean / _std`` stay NaN per
    iteration.  After the last iteration one E-step over all sequences under the final parameters fills
    ``var_x, lalpha, lbeta, lliks`` (all ``T`` rows) and ``hamming``.

    ``infer(device_loop=None)``: with ``seq_minibatch`` set, the iterations run in the engine's resident SVI loop
    (``svi_begin*``, ``svi_sequences``, one ``svi_iteration_sequences`` call per iteration: the variational state
    stays in HBM, the same draws come from the global stream, ``elbo_vec`` and ``iter_time`` -- device seconds --
    from ``svi_read_elbo``) where ``_svi_sequences_refusal()`` finds nothing against it (an engine with the loop, one
    of its emission families with the family's own ``get_vlb``, no piece of the host route overridden or wrapped,
    ``prior_tran >= 1``, pseudo-counts in the loop's range); otherwise the host route above.  ``device_loop=False`` keeps the host route, ``device_loop=True`` raises ``RuntimeError`` with the
    reason where the loop cannot be taken."""

    @staticmethod
    def make_param_dict(prior_init, prior_tran, prior_emit, tau=tau0,
                        kappa=kappa0, mask=None, seq_minibatch=None):
        """``seq_minibatch``: optional, default None (see the class)."""
        return {'prior_init': prior_init, 'prior_tran': prior_tran,
                'prior_emit': prior_emit, 'mask': mask, 'tau': tau,
                'kappa': kappa, 'seq_minibatch': seq_minibatch}

    def __init__(self, obs, prior_init, prior_tran, prior_emit, tau=tau0,
                 kappa=kappa0, mask=None, init_init=None, init_tran=None,
                 epsilon=1e-8, maxit=100, verbose=False, sts=None, engine=None, device=0, dtype="f64",
                 seq_minibatch=None):
        super(VBHMM, self).__init__(obs, prior_init, prior_tran, prior_emit,
                                    mask=mask, init_init=init_init,
                                    init_tran=init_tran, verbose=verbose,
                                    sts=sts, engine=engine, device=device, dtype=dtype)
        self.batch = self.obs
        self.elbo = -np.inf
        self.tau = tau
        self.kappa = kappa
        self.lrate = tau ** (-kappa)
        self.epsilon = epsilon
        self.maxit = maxit
        self.batchfactor = 1.
        self.seq_minibatch = None
        if seq_minibatch is not None:
            n = len(self.seq_off) - 1 if self._multi() else 0
            if n < 2:
                raise RuntimeError("seq_minibatch needs obs to be a list of at least two sequences")
            if int(seq_minibatch) != seq_minibatch or not 1 <= int(seq_minibatch) <= n:
                raise RuntimeError("seq_minibatch = %r must be an integer in [1, N = %d]" % (seq_minibatch, n))
            self.seq_minibatch = int(seq_minibatch)

        self.var_x = np.ones((self.T, self.K))
        self.var_x /= np.sum(self.var_x, axis=1)[:, np.newaxis]

        self.lalpha = np.empty((self.T, self.K))
        self.lbeta = np.empty((self.T, self.K))
        self.lliks = np.empty((self.T, self.K))
        self.mod_init = np.zeros(self.K)
        self.mod_tran = np.zeros((self.K, self.K))

    # pieces of the host route a subclass (or a wrapper set on the instance) may replace, and the engine calls it makes:
    # where one is replaced the host route, which goes through them, is used (hmmsgd_metaobs.VBHMM._LOOP_HOOKS)
    _SEQ_LOOP_HOOKS = ("local_update", "global_update", "lower_bound", "_seq_minibatch_stats", "_sequence_subset_estep",
                       "_global_update_from_stats", "_natgrad_emissions", "_psi_expectations", "_emit_vlb",
                       "_push_globals", "_push_emission")
    _SEQ_ENGINE_CALLS = ("estep_sequence_subset", "set_globals", "set_emission_niw", "set_emission_diag",
                         "set_emission_cat", "set_emission_mcat", "set_emission_poisson", "set_emission_pgauss")

    def _svi_sequences_refusal(self):
        """Why ``infer`` cannot run in the engine's resident loop on sequence minibatches (None: it can)."""
        if self.seq_minibatch is None:
            return "seq_minibatch is not set"
        if self.__dict__.get("labels") is not None:
            return ("labels are set (set_labels): the resident loop does not take them; the host route steps "
                    "on estep_sequence_subset, which honours them")
        if self.__dict__.get("state_sets") is not None:
            return ("allowed-state sets are set (set_state_sets): the resident loop does not take them; the host "
                    "route steps on estep_sequence_subset, which honours them")
        eng = self.engine
        if not (hasattr(eng, "svi_sequences") and hasattr(eng, "svi_iteration_sequences")):
            return "the engine has no svi_sequences / svi_iteration_sequences"
        if self._pgauss_fastpath():
            return ("the resident loop does not take ProductGaussian emitters (svihmm_set_emission_pgauss has no "
                    "svi_begin of its own): the sequence minibatches step on the host route")
        fam = self._svi_family()
        if fam is None or not hasattr(eng, FAMILY[fam].svi_method):
            return "the emitters are none of the resident loop's families on this engine"
        if not self._svi_plain_vlb(fam):
            return "an emitter overrides get_vlb"
        for name in self._SEQ_LOOP_HOOKS:
            if name in self.__dict__ or getattr(type(self), name) is not getattr(VBHMM, name):
                return "%s is overridden" % name
        for name in self._SEQ_ENGINE_CALLS:
            if name in getattr(eng, "__dict__", {}):
                return "the engine's %s is replaced on the instance" % name
        if np.min(self.prior_tran) < 1.0:
            return "prior_tran has entries below 1"
        for name in ("var_tran", "var_init", "prior_init"):
            if not np.min(getattr(self, name)) >= L.SVI_MIN_PSEUDOCOUNT:
                return "%s has entries below SVI_MIN_PSEUDOCOUNT = %g" % (name, L.SVI_MIN_PSEUDOCOUNT)
        return None

    def _infer_device_sequences(self):
        """The iterations of ``infer`` in the engine's resident loop: upload once, one call per iteration with the
        host route's draw, then ``elbo_vec`` / ``iter_time`` and the state back on the object."""
        eng = self.engine
        maxit, n, m = self.maxit, len(self.seq_off) - 1, self.seq_minibatch
        self._upload_obs()
        self._svi_begin(self._svi_family(), maxit)
        eng.svi_sequences(self.prior_init, self.var_init)
        self.batchfactor = bf = n / m
        self._seq_var_x = None
        for it in range(maxit):
            self.lrate = (it + self.tau) ** (-self.kappa)
            idx = np.sort(np.random.choice(n, size=m, replace=False))
            eng.svi_iteration_sequences(it, idx, 0, self.lrate, bf)
        elbo, ms = eng.svi_read_elbo(maxit)
        self._svi_pull_state()
        self.elbo_vec = elbo
        self.iter_time = ms * 1e-3
        self.elbo = elbo[-1]
        if self.verbose:
            for it in range(maxit):
                print("iter: %d, ELBO: %.2f" % (it, elbo[it]))
            sys.stdout.flush()

    def infer(self, fused=True, device_loop=None):
        """reference hmmbatchsgd.py:143-200 (no early stop, ``if False:`` :180).  ``device_loop``: see the class."""
        if type(self).local_update is not VariationalHMMBase.local_update \
                or type(self).global_update is not VBHMM.global_update:
            fused = False
        why = self._svi_sequences_refusal() if device_loop is not False else "device_loop=False"
        if device_loop is True and why is not None:
            raise RuntimeError("infer(device_loop=True): %s" % why)
        self._require_fused_sequences(fused)
        mb = self.seq_minibatch       # (a list of sequences: the line above has refused everything but the fused path)
        route = not fused and self._batch_stats_route(VBHMM.global_update, ("niw", "diag"))
        self.obs_full = self.obs.copy()
        self.obs[self.mask, :] = np.nan       # hmmbatchsgd.py:149 (NaN rows -> lliks 0)
        self._obs_dirty = True

        maxit = self.maxit
        self.elbo_vec = np.inf * np.ones(maxit)
        self.pred_logprob_mean = np.nan * np.ones(maxit)
        self.pred_logprob_std = np.nan * np.ones(maxit)
        self.iter_time = np.nan * np.ones(maxit)

        if why is None:
            self._infer_device_sequences()
        for it in range(maxit if why is not None else 0):
            start_time = time.time()
            self.lrate = (it + self.tau) ** (-self.kappa)
            if mb is not None:
                st = self._seq_minibatch_stats()
                self._global_update_from_stats(st)
            elif fused:
                st = self._batch_estep_stats()
                self._global_update_from_stats(st)
            elif route:
                # a local_update override: its posteriors' statistics on the device, then the same
                # update the fused path applies
                self.local_update()
                self._global_update_from_stats(self._batch_suffstats())
            else:
                self.local_update()
                self.global_update()
            self.iter_time[it] = time.time() - start_time

            lb = self.lower_bound()
            if self.verbose:
                print("iter: %d, ELBO: %.2f" % (it, lb))
                sys.stdout.flush()

            self.elbo = lb
            self.elbo_vec[it] = lb
            if mb is None and np.any(self.mask):    # (a minibatch leaves posteriors of M sequences only: NaN)
                if fused:
                    self.var_x = self._read_var_x()
                tmp = self.pred_logprob()
                if tmp is not None:
                    self.pred_logprob_mean[it] = np.mean(tmp)
                    self.pred_logprob_std[it] = np.std(tmp)

        lbidx = np.where(np.logical_not(np.isinf(self.elbo_vec)))[0]
        self.elbo_vec = self.elbo_vec[lbidx]
        self.pred_logprob_mean = self.pred_logprob_mean[lbidx]
        self.pred_logprob_std = self.pred_logprob_std[lbidx]
        self.iter_time = self.iter_time[lbidx]

        if mb is not None:
            # the per-row attributes cover all T rows: one E-step over every sequence under the final parameters
            _, self._lZ, _ = self._sequences_estep()
        if fused:
            self._fetch_local()
        if self.sts is not None:
            self.hamming, self.perm = self.hamming_dist(self.var_x, self.sts)

        self.obs = self.obs_full
        self._obs_dirty = True

    def _natgrad_emissions(self, lrate, stats_for_k):
        for k in range(self.K):
            G = self.var_emit[k]
            if type(G) is ProductCategorical:
                # Dirichlet factors: the natural parameters are alpha - 1, so the blend is the blend of alpha
                new = stats_for_k(G, k)
                G._set_alpha([(1. - lrate) * a + lrate * b for a, b in zip(G.alpha_mf, new)])
                continue
            if type(G) is ProductPoisson:
                # Gamma factors: the natural parameters are (a - 1, -b), so the blend is linear in (a, b)
                a, b = stats_for_k(G, k)
                G._set_mf((1. - lrate) * G.alpha_mf + lrate * a, (1. - lrate) * G.beta_mf + lrate * b)
                continue
            if is_diag_gaussian(G) or type(G) is ProductGaussian:
                # the same blend in the diagonal family's natural parameters (the reference's
                # NIW arithmetic, util.py:28-60, has no counterpart for it)
                new = stats_for_k(G, k)
                eta = ((1. - lrate) * G.to_natural(G.mf_mu, G.mf_nus, G.mf_alphas, G.mf_betas)
                       + lrate * G.to_natural(*new))
                G._set_mf(*G.from_natural(eta))
                continue
            mu_mf, sigma_mf, kappa_mf, nu_mf = stats_for_k(G, k)
            nats_t = util.NIW_mf_natural_pars(mu_mf, sigma_mf, kappa_mf, nu_mf)
            nats_old = util.NIW_mf_natural_pars(G.mu_mf, G.sigma_mf, G.kappa_mf, G.nu_mf)
            nats_new = (1. - lrate) * nats_old + lrate * nats_t
            util.NIW_mf_moment_pars(G, *nats_new)

    def _seq_minibatch_stats(self):
        """One iteration's minibatch of whole sequences: the draw, ``batchfactor = N / M``, the E-step of the
        drawn sequences and their statistics times ``batchfactor`` (every entry of the packed layout is a sum
        over rows, so the whole buffer scales); ``_lZ`` the scaled local bound, ``_q0`` the unscaled sum of
        first posterior rows (``_global_update_from_stats`` scales it)."""
        n = len(self.seq_off) - 1
        idx = np.sort(np.random.choice(n, size=self.seq_minibatch, replace=False))
        self.batchfactor = bf = n / self.seq_minibatch
        st, lb, self._q0 = self._sequence_subset_estep(idx)
        st = rewrap_packed(st, st.buf * bf)
        self._lZ = bf * lb
        return st

    def _global_update_from_stats(self, st):
        lrate = self.lrate
        if self.seq_minibatch is None:
            self.var_init = self.prior_init + self._q0
        else:      # a noisy estimate like the others: blended, not replaced
            self.var_init = (1. - lrate) * self.var_init + lrate * (self.prior_init + self.batchfactor * self._q0)
        nats_old = self.var_tran - 1.
        nats_t = (self.prior_tran + st.A_raw) - 1.
        self.var_tran = ((1. - lrate) * nats_old + lrate * nats_t) + 1.

        def from_stats(G, k):
            if hasattr(st, "col_counts"):
                return G._posterior_hypparams([c[k] for c in st.col_counts])
            if hasattr(st, "sxx"):
                return G._posterior_hypparams(st.n[k], st.sx[k], st.sxx[k], st.origin)
            if hasattr(st, "sx"):
                return G._posterior_hypparams(st.sx[k], st.n[k])
            if hasattr(st, "xsq"):
                return G._posterior_hypparams(st.neff[k], st.xbar[k], st.xsq[k])
            if not is_niw_gaussian(G):
                raise RuntimeError("fused batch update needs NIW Gaussian emissions")
            n = st.neff[k]
            if n > 0:
                xbar = st.xbar[k] / n
                return G._posterior_hypparams(n, xbar, st.S[k] - n * np.outer(xbar, xbar))
            return G._posterior_hypparams(n, None, None)
        self._natgrad_emissions(lrate, from_stats)

    def global_update(self, batch=None):
        """Literal host M-step (reference hmmbatchsgd.py:202-259)."""
        if batch is None:
            batch = self.obs
        lrate = self.lrate
        self.var_init = self.prior_init + self.var_x[0, :]
        nats_old = self.var_tran - 1.
        tran_mf = self.prior_tran.copy()
        for t in range(1, self.T):
            tran_mf += np.outer(self.var_x[t - 1, :], self.var_x[t, :])
        nats_t = tran_mf - 1.
        self.var_tran = ((1. - lrate) * nats_old + lrate * nats_t) + 1.
        inds = np.logical_not(self.mask)
        def from_rows(G, k):
            x, w = batch[inds, :], self.var_x[inds, k]
            if is_diag_gaussian(G) or type(G) in (ProductCategorical, ProductPoisson, ProductGaussian):
                return G._posterior_hypparams(*G._get_weighted_statistics(x, w))
            return util.NIW_meanfield(G, x, w)
        self._natgrad_emissions(lrate, from_rows)
