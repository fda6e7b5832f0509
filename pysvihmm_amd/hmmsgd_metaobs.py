"""SVI for HMMs with meta-observation minibatches -- class surface of the reference
``hmmsgd_metaobs.py`` (the working SVI implementation).

One SVI iteration (reference hmmsgd_metaobs.py:347-445):
  host : learning rate, minibatch sampling, stationary init (eig, :413-418),
         psi-expectations (:502-504)                      -- O(K^3), once per iteration
  GPU  : for ALL windows of the minibatch at once: emission expected log-lik,
         forward/backward, posteriors, expected sufficient statistics, local bound
         (:487-519, :857-928, :271; the reference's serial ``for data in minibatch``)
  RCCL : one all-reduce of the packed statistics when several GPUs share the minibatch
  host : natural-gradient step (:1010-1084), identical on every rank

Quirks reproduced on purpose: Q1 wrap-around product-of-
marginals transition statistic, Q2 ``prior_tran-1`` once per window, Q3 batch factors
from the constructor's L and S, Q4 local bound summed over all t, Q5 un-normalised
eigenvector as ``var_init``, Q8 ``metaobs_noverlap`` returning S+1 windows, Q9 masked
rows contribute to lliks but not to the emission statistics.
"""
from __future__ import division

import sys
import time
import weakref

import numpy as np
import numpy.random as npr
from numpy import newaxis as npa
from scipy.special import digamma

from .hmmbase import FAMILY, VariationalHMMBase, is_niw_gaussian, is_diag_gaussian, dirichlet_elbo
from .distributions import Gaussian, Categorical, DiagonalGaussian, ProductCategorical, ProductPoisson
from . import util
from . import _lib as L

eps = 1e-9

tau0 = 1.
kappa0 = 0.7
metaobs_half0 = 1
mb_sz0 = 1


class _StackedStats(list):
    """``emit_inter`` of a fused minibatch E-step: behaves like the reference's list of K
    ``[xbar, neff, S, neff]`` items and also carries the stacked arrays."""

    def __init__(self, xbar, neff, S):
        super(_StackedStats, self).__init__(
            util._obj(xbar[k], float(neff[k]), S[k], float(neff[k])) for k in range(len(neff)))
        self.xbar, self.neff, self.S = xbar, neff, S


class MetaObs(object):
    """Inclusive index bounds of a meta-observation (reference :42-45)."""

    def __init__(self, i1, i2):
        self.i1 = i1
        self.i2 = i2


def _lazy_window_attr(name):
    """``lliks / lalpha / lbeta / var_x`` of the last window of a fused minibatch: the reference
    leaves them on the object after every iteration (:396-436); here they are fetched from the
    device on first access instead of every iteration (the large-batch device path does not
    even materialise logarithms unless asked).  Assigning the attribute works as usual."""
    key = "_val_" + name

    def get(self):
        pend = self.__dict__.get("_pending_rows")
        if pend is not None and name in pend[2]:
            row0, nrows, names = pend
            names.discard(name)
            self.__dict__[key] = self.engine.read_rows(name, row0, nrows)
        return self.__dict__[key]

    def set_(self, value):
        pend = self.__dict__.get("_pending_rows")
        if pend is not None:
            pend[2].discard(name)
        self.__dict__[key] = value

    return property(get, set_)


class VBHMM(VariationalHMMBase):
    """ Stochastic variational inference for finite HMMs using natural gradients;
    consecutive groups of nodes are sampled as a "meta-observation"."""

    lliks = _lazy_window_attr("lliks")
    lalpha = _lazy_window_attr("lalpha")
    lbeta = _lazy_window_attr("lbeta")
    var_x = _lazy_window_attr("var_x")

    @staticmethod
    def make_param_dict(prior_init, prior_tran, prior_emit, tau=tau0,
                        kappa=kappa0, metaobs_half=metaobs_half0, mb_sz=mb_sz0,
                        mask=None):
        return {'prior_init': prior_init, 'prior_tran': prior_tran,
                'prior_emit': prior_emit, 'mask': mask, 'tau': tau,
                'kappa': kappa, 'metaobs_half': metaobs_half, 'mb_sz': mb_sz}

    def set_labels(self, labels):
        """Not supported by this class: its iterations run in the engine's resident SVI loop and its adaptive
        windows through ``grow_windows``, and neither takes labels.  ``hmmbatchcd.VBHMM`` and
        ``hmmbatchsgd.VBHMM`` honour them."""
        if labels is None:
            self.labels = None
            return
        raise NotImplementedError("hmmsgd_metaobs.VBHMM.set_labels: the resident SVI loop and grow_windows do not "
                                  "take labels; use hmmbatchcd.VBHMM or hmmbatchsgd.VBHMM")

    def set_state_sets(self, allowed):
        """Not supported by this class, for the reason ``set_labels`` gives."""
        if allowed is None:
            self.state_sets = None
            return
        raise NotImplementedError("hmmsgd_metaobs.VBHMM.set_state_sets: the resident SVI loop and grow_windows do "
                                  "not take allowed-state sets; use hmmbatchcd.VBHMM or hmmbatchsgd.VBHMM")

    def set_metaobs_fun(self):
        if self.metaobs_fun_name == 'unif':
            self.metaobs_fun = self.metaobs_unif
        elif self.metaobs_fun_name == 'noverlap':
            self.metaobs_fun = self.metaobs_noverlap
        else:
            raise RuntimeError("Unknown value for metaobs_fun: %s" % (self.metaobs_fun_name,))

    def __init__(self, obs, prior_init, prior_tran,
                 prior_emit, tau=tau0, kappa=kappa0,
                 metaobs_half=metaobs_half0, mb_sz=mb_sz0, mask=None,
                 full_predprob=False, init_init=None, init_tran=None,
                 maxit=100, verbose=False, adagrad=False, metaobs_fun='unif',
                 seed=None, sts=None, fullpred_freq=10, fullpred_sched=None,
                 growBuffer=False, bufferBudget=False, engine=None, device=0, comm=None, dtype="f64"):
        np.random.seed(seed)
        self.seed = seed

        super(VBHMM, self).__init__(obs, prior_init, prior_tran,
                                    prior_emit, mask=mask, init_init=init_init,
                                    init_tran=init_tran, verbose=verbose,
                                    sts=sts, engine=engine, device=device, dtype=dtype)
        if self._multi():
            # (the batch factors (T - 2L - 1)/(2L S), quirk Q3, have no agreed multi-sequence form)
            raise RuntimeError("hmmsgd_metaobs.VBHMM takes one sequence: a list of several is supported "
                               "by the batch classes (hmmbatchcd, hmmbatchsgd) only")

        self.elbo = -np.inf
        self.tau = tau
        self.kappa = kappa
        self.lrate = tau ** (-kappa)
        self.full_predprob = full_predprob
        self.fullpred_freq = fullpred_freq
        if fullpred_sched is not None:
            self.fullpred_sched = fullpred_sched
        else:
            self.fullpred_sched = np.arange(0, maxit, 10)

        self.mataobs_fun_name = metaobs_fun  # (sic) reference typo kept, quirk Q10
        if metaobs_fun == 'unif':
            self.metaobs_fun = self.metaobs_unif
            self.metaobs_fun_name = 'unif'
        elif metaobs_fun == 'noverlap':
            self.metaobs_fun = self.metaobs_noverlap
            self.metaobs_fun_name = 'noverlap'
        else:
            raise RuntimeError("Unknown value for metaobs_fun: %s" % (metaobs_fun,))

        self.adagrad = adagrad
        if adagrad:
            self.ada_G = 1.0 * np.ones(self.prior_tran.shape)

        self.maxit = maxit
        self.growBuffer = growBuffer
        self.bufferBudget = bufferBudget

        if metaobs_half < 1:
            raise RuntimeError("metaobs (%d) must be >= 1." % (metaobs_half,))
        self.metaobs_half = metaobs_half
        self.mb_sz = mb_sz
        self.cur_mo = None
        self.batchfactor = 1.
        self.comm = comm

        metaobs_sz = 2 * metaobs_half + 1
        self.var_x = np.random.rand(metaobs_sz, self.K)
        self.var_x /= np.sum(self.var_x, axis=1)[:, np.newaxis]
        self.lalpha = np.empty((metaobs_sz, self.K))
        self.lbeta = np.empty((metaobs_sz, self.K))
        self.lliks = np.empty((metaobs_sz, self.K))

    def __getstate__(self):
        d = super(VBHMM, self).__getstate__()
        d['comm'] = None
        return d

    # -- minibatch samplers (reference :210-255) ----------------------------------------
    def metaobs_unif(self, N, L_, n):
        ll = L_
        uu = N - 1 - L_
        c_vec = npr.randint(ll, uu + 1, n)
        return [MetaObs(c - L_, c + L_) for c in c_vec]

    def metaobs_noverlap(self, N, L_, n):
        """Returns n+1 windows and rejects only |dc| <= L (quirk Q8, reference :229-255)."""
        ll = L_
        uu = N - 1 - L_
        c_vec = np.inf * np.ones(n)
        minibatch = list()
        c = npr.randint(ll, uu + 1, 1)[0]
        minibatch.append(MetaObs(c - L_, c + L_))
        for i in range(n):
            c = npr.randint(ll, uu + 1, 1)[0]
            while np.any(np.abs(c_vec - c) <= L_):
                c = npr.randint(ll, uu + 1, 1)[0]
            c_vec[i] = c
            minibatch.append(MetaObs(c - L_, c + L_))
        return minibatch

    # -- bounds ---------------------------------------------------------------------------
    def local_lower_bound(self):
        """sum_t LSE_k lalpha[t,k] of the current meta-observation (reference :257-271)."""
        if self._lZ is not None:
            return self._lZ
        return np.sum(np.logaddexp.reduce(self.lalpha, axis=1))

    def global_lower_bound(self):
        """reference :273-296."""
        return dirichlet_elbo(self.prior_tran, self.var_tran) + self._emit_vlb()

    # -- the SVI loop -----------------------------------------------------------------------
    def _stationary_init(self):
        """reference :413-418 (same for every window of a minibatch: computed once)."""
        A_mean = self.var_tran / np.sum(self.var_tran, axis=1)[:, npa]
        # The reference takes |eigenvector| of the largest eigenvalue of A_mean.T from
        # np.linalg.eig: for a strictly positive row-stochastic matrix that is the Perron vector
        # (eigenvalue 1, unique), unit L2 norm.  The same vector from one linear solve,
        # pi (A - I + 1 1^T) = 1^T, is ~10x cheaper than the general eigen-decomposition that
        # otherwise costs more than the device E-step of a 64-window minibatch; eig stays the
        # fallback if the solve is singular (zero rows in var_tran).
        K = self.K
        try:
            pi = np.linalg.solve(A_mean.T - np.eye(K) + 1.0, np.ones(K))
            if not (np.all(np.isfinite(pi)) and pi.min() > 0):
                raise np.linalg.LinAlgError
            self.var_init = pi / np.sqrt(np.dot(pi, pi))
        except np.linalg.LinAlgError:
            ew, ev = np.linalg.eig(A_mean.T)
            ew_dec = np.argsort(ew)[::-1]
            self.var_init = np.abs(ev[:, ew_dec[0]])

    def _alloc_local(self, halfL):
        metaobs_sz = 2 * halfL + 1
        self.var_x = np.random.rand(metaobs_sz, self.K)
        self.var_x /= np.sum(self.var_x, axis=1)[:, np.newaxis]
        self.lalpha = np.empty((metaobs_sz, self.K))
        self.lbeta = np.empty((metaobs_sz, self.K))
        self.lliks = np.empty((metaobs_sz, self.K))

    def infer(self, adaptive=False, perIter=10, epsilon=1e-6, minHalfL=1,
              avgResidual=False, Lincrement=1, Lcutoff=1000, fused=True, device_loop=None):
        """ Runs stochastic variational inference (reference :298-485).

        ``fused=True`` (default): all windows of a minibatch in one device E-step.  On top of
        that, when nothing on the object overrides the loop's pieces (NIW Gaussian emitters,
        no AdaGrad), the whole iteration -- stationary init, psi-expectations, E-step, global
        natural-gradient step, ELBO -- runs on the device with the variational state resident in
        HBM (``device_loop=False`` keeps the global step and the ELBO on the host); the object's
        attributes are filled in when the loop ends (and wherever the loop itself needs them on
        the host: adaptive L / buffer growth, ``full_predprob``, ``verbose``)."""
        np.random.seed(self.seed)
        if (any(getattr(type(self), n) is not getattr(VBHMM, n) for n in
                ("local_update", "intermediate_pars", "intermediate_pars_buffer", "forward_msgs",
                 "backward_msgs", "local_lower_bound"))
                or not self._device_family()):
            # subclass overrides, or an emission family the device statistics kernels
            # do not know (the reference dispatches on the type too, :887,907):
            # follow the reference loop literally, E-step recursions still on the device
            fused = False

        growBuffer = self.growBuffer
        bufferBudget = self.bufferBudget
        maxit = self.maxit
        if self.metaobs_fun is None:
            self.set_metaobs_fun()

        self.elbo_vec = np.inf * np.ones(maxit)
        K = self.K
        self.iter_time = np.inf * np.ones(maxit)

        mb_sz = self.mb_sz
        L_ = self.metaobs_half
        miniL = L_
        bufferL = L_
        if (L_ is None or adaptive) and growBuffer:
            raise RuntimeError("Cannot specify both adaptive and buffer simultaneously!")

        # (the reference reads self.obs afresh in every call: so does this one.  Opt-in
        #  `self.assume_obs_unchanged = True` skips the upload while hmmbase._obs_fingerprint's
        #  sampled probe finds the buffer unchanged -- 256 MB at T = 1e6)
        # wall-clock marks of the call's fixed part (not a reference attribute; bench.py reports it):
        # obs upload | svi_begin | host submission of the iterations | wait + state read-back | last window
        wall = self.infer_wall_ms = {}
        t_mark = time.perf_counter()
        if not self._obs_unchanged():
            self._obs_dirty = True
        self._upload_obs()
        wall["upload_obs"] = (time.perf_counter() - t_mark) * 1e3

        if fused and device_loop is not False and self._svi_device_ok():
            # variational state resident in HBM for the whole loop (engine.svi_*)
            self._infer_device(adaptive, perIter, epsilon, minHalfL, avgResidual, Lincrement, Lcutoff)
            t_mark = time.perf_counter()
            self._resolve_pending()
            wall["last_window"] = wall.get("last_window", 0.0) + (time.perf_counter() - t_mark) * 1e3
            self.metaobs_fun = None
            return

        for it in range(maxit):
            start_time = time.time()
            self.lrate = (it + self.tau) ** (-self.kappa)

            if L_ is None or (adaptive and it % perIter == 0):
                L_ = self.select_L(mb_sz, epsilon=epsilon, minHalfL=minHalfL,
                                   avgResidual=avgResidual, Lincrement=Lincrement,
                                   Lcutoff=Lcutoff)
                self._alloc_local(L_)
                miniL = L_

            if growBuffer and it % perIter == 0:
                bufferL = self.select_buffer(self.mb_sz, epsilon=epsilon, halfL=L_,
                                             avgResidual=avgResidual,
                                             Lincrement=Lincrement, Lcutoff=Lcutoff)
                self._alloc_local(bufferL)
                miniL = bufferL
                if bufferBudget:
                    mb_sz = self.buffer_budget(bufferL)

            minibatch = self.metaobs_fun(self.T, miniL, mb_sz)

            if fused:
                A_inter, emit_inter, lb = self._minibatch_estep(
                    minibatch, miniL, (bufferL, L_) if growBuffer else None)
            else:
                lb = 0.
                route = self._suffstats_route()
                segs = []
                A_inter = np.zeros_like(self.var_tran)
                if type(self.var_emit[0]) in (Categorical, ProductCategorical):
                    # the reference calls util.NIW_zero_nat_pars here for every family
                    # (:399), which raises for a Categorical; zeros of the right shape instead
                    # (ProductCategorical: the D columns side by side, F = sum of the V_d entries)
                    emit_inter = [np.zeros(self.var_emit[0].num_parameters()) for k in range(K)]
                elif type(self.var_emit[0]) is ProductPoisson:
                    emit_inter = [np.zeros((2, self.var_emit[0].D)) for k in range(K)]      # [sx | n]
                elif is_diag_gaussian(self.var_emit[0]):
                    emit_inter = [np.zeros((4, self.D)) for k in range(K)]
                else:
                    emit_inter = [util.NIW_zero_nat_pars(self.var_emit[0]) for k in range(K)]
                for data in minibatch:
                    self.cur_mo = data
                    self._stationary_init()
                    self.local_update(metaobs=data)
                    if route:
                        # the posteriors intermediate_pars(_buffer) would read (reference :857-1008);
                        # their statistics are taken for the whole minibatch below
                        if growBuffer:
                            segs.append((data.i1 + bufferL - L_, data.i2 - bufferL + L_,
                                         np.array(self.var_x[bufferL - L_:bufferL + L_ + 1, :], dtype=np.float64)))
                        else:
                            segs.append((data.i1, data.i2, np.array(self.var_x, dtype=np.float64)))
                    else:
                        if growBuffer:
                            A_i, e_i = self.intermediate_pars_buffer(data, bufferL, L_)
                        else:
                            A_i, e_i = self.intermediate_pars(data)
                        A_inter += A_i
                        for k in range(K):
                            emit_inter[k] += e_i[k]
                    lb += self.local_lower_bound()
                if segs:
                    A_inter, emit_inter = self._segments_inter(segs, A_inter, emit_inter)

            self.global_update(A_inter, emit_inter)
            self.iter_time[it] = time.time() - start_time

            lb += self.global_lower_bound()
            self.elbo_vec[it] = lb
            if self.verbose:
                print("iter: %d, ELBO: %.2f" % (it, lb))
                sys.stdout.flush()

            if self.full_predprob and it in self.fullpred_sched:
                # the reference writes into arrays whose allocation is commented out
                # (quirk Q11); allocate them lazily instead of raising AttributeError
                if not hasattr(self, 'pred_logprob_full_mean'):
                    self.pred_logprob_full_mean = np.inf * np.ones(maxit)
                    self.pred_logprob_full_std = np.inf * np.ones(maxit)
                tmp = self.pred_logprob_full()
                self.pred_logprob_full_mean[it] = np.nanmean(tmp)
                self.pred_logprob_full_std[it] = np.nanstd(tmp)

        # the last window's lliks / lalpha / lbeta / var_x now (no lazy state survives infer:
        # a later call that uploads new parameters could no longer rebuild them)
        self._resolve_pending()

        # So that the hmm object can be pickled
        self.metaobs_fun = None

    # pieces of the loop a subclass (or a wrapper set on the instance) may replace: then the
    # host loop, which calls them, is used
    _LOOP_HOOKS = ("local_update", "intermediate_pars", "intermediate_pars_buffer", "global_update",
                   "global_lower_bound", "local_lower_bound", "_minibatch_estep", "_stationary_init",
                   "_psi_expectations", "_emit_vlb", "_global_update_niw_stacked")

    def _svi_device_ok(self):
        eng = self.engine
        fam = self._svi_family()
        if fam is None or not hasattr(eng, FAMILY[fam].svi_method):
            return False
        if self.adagrad and not hasattr(eng, "svi_set_adagrad"):
            return False
        if not self._svi_plain_vlb(fam):
            return False
        for name in self._LOOP_HOOKS:
            if name in self.__dict__ or getattr(type(self), name) is not getattr(VBHMM, name):
                return False
        if self.comm is not None and not hasattr(self.comm, "bind_engine"):
            return False
        # transition pseudo-counts this small need the log-domain recursion, which the engine
        # selects per globals upload (include/svihmm.h: SVIHMM_SVI_MIN_PSEUDOCOUNT)
        # (and the loop's range argument needs prior_tran >= 1: quirk Q2 scales prior_tran - 1 by
        #  ~T / 2L, which drives var_tran towards zero or below for sparser priors)
        if np.min(self.var_tran) < L.SVI_MIN_PSEUDOCOUNT or np.min(self.prior_tran) < 1.0:
            return False
        return True

    def _infer_device(self, adaptive, perIter, epsilon, minHalfL, avgResidual, Lincrement, Lcutoff):
        """The loop of reference :347-445 with one engine call per iteration; same random stream
        (minibatch sampling, select_L / select_buffer draws, the re-initialisation draws of
        :360-365) and same arithmetic as the host loop."""
        eng = self.engine
        comm = self.comm
        if comm is not None:
            comm.bind_engine(eng)
        maxit, K = self.maxit, self.K
        growBuffer, bufferBudget = self.growBuffer, self.bufferBudget
        mb_sz = self.mb_sz
        L_ = self.metaobs_half
        miniL = bufferL = L_
        fam = self._svi_family()
        wall = self.__dict__.setdefault("infer_wall_ms", {})
        t_mark = time.perf_counter()
        self._svi_begin(fam, maxit)
        if self.adagrad:        # the accumulator of reference :1036-1040 joins the resident state
            eng.svi_set_adagrad(self.ada_G)
        self.__dict__.pop("_pending_rows", None)
        if hasattr(eng, "on_next_mutation"):
            eng.on_next_mutation(None)
        host_fresh = True            # the object's attributes equal the device state
        T = self.T
        wall["svi_begin"] = (time.perf_counter() - t_mark) * 1e3
        t_mark = time.perf_counter()
        # quirk Q3: batch factors from the CONSTRUCTOR's L and S, whatever the windows are
        bA = (T - 2 * self.metaobs_half - 1) / (2. * self.metaobs_half * self.mb_sz)
        bE = (T - 2 * self.metaobs_half - 1) / ((2. * self.metaobs_half + 1.) * self.mb_sz)
        last = None
        loop_globals_live = False
        own_unif = getattr(self.metaobs_fun, "__func__", None) is VBHMM.metaobs_unif
        for it in range(maxit):
            self.lrate = (it + self.tau) ** (-self.kappa)
            resize = (L_ is None or (adaptive and it % perIter == 0)) or (growBuffer and it % perIter == 0)
            if resize and not host_fresh:
                self._svi_pull_state()
                host_fresh = True
            if L_ is None or (adaptive and it % perIter == 0):
                L_ = self.select_L(mb_sz, epsilon=epsilon, minHalfL=minHalfL, avgResidual=avgResidual,
                                   Lincrement=Lincrement, Lcutoff=Lcutoff)
                self._alloc_local(L_)
                miniL = L_
            if growBuffer and it % perIter == 0:
                bufferL = self.select_buffer(self.mb_sz, epsilon=epsilon, halfL=L_, avgResidual=avgResidual,
                                             Lincrement=Lincrement, Lcutoff=Lcutoff)
                self._alloc_local(bufferL)
                miniL = bufferL
                if bufferBudget:
                    mb_sz = self.buffer_budget(bufferL)
            if own_unif:
                # metaobs_unif (:210-227) without the list of MetaObs objects: the same single
                # randint draw, window starts as an array (64 objects per iteration were most of
                # the loop's host time)
                c_vec = npr.randint(miniL, T - 1 - miniL + 1, mb_sz)
                all_starts = np.asarray(c_vec, dtype=np.int64) - miniL
                nwin = len(all_starts)
                last_mo = MetaObs(c_vec[-1] - miniL, c_vec[-1] + miniL) if nwin else None
            else:
                minibatch = self.metaobs_fun(T, miniL, mb_sz)
                all_starts = np.array([mo.i1 for mo in minibatch], dtype=np.int64)
                nwin = len(minibatch)
                last_mo = minibatch[-1] if nwin else None
            starts = all_starts if comm is None else all_starts[comm.rank::comm.size]
            Lm = 2 * miniL + 1
            flags = L.TRANS_WRAP | L.KEEP_LBETA
            if it == maxit - 1:
                flags |= L.SVI_KEEP_WINDOW
            inner = (bufferL - L_, 2 * L_ + 1) if growBuffer else None
            eng.svi_iteration(it, starts, nwin, Lm, flags, self.lrate, bA, bE, inner=inner)
            host_fresh = False
            loop_globals_live = True      # the handle's ltran / mod_init stem from the loop (see the hook below)
            self.cur_mo = last_mo
            last = (len(starts), Lm)
            if self.verbose:
                e, _ = eng.svi_read_elbo(it + 1)
                print("iter: %d, ELBO: %.2f" % (it, e[it]))
                sys.stdout.flush()
            if self.full_predprob and it in self.fullpred_sched:
                self._svi_pull_state()
                host_fresh = True
                if it == maxit - 1:
                    self._register_last_window(eng, last)
                if not hasattr(self, 'pred_logprob_full_mean'):
                    self.pred_logprob_full_mean = np.inf * np.ones(maxit)
                    self.pred_logprob_full_std = np.inf * np.ones(maxit)
                # the hook uploads psi-expectations of the UPDATED state to the handle; the
                # reference's full_local_update keeps them in locals (:1157-1159), its object still
                # holds the last local_update's (:502-504): take the loop's off the handle first.
                # After the LAST iteration these are exactly the reference's (no further globals
                # kernel exists).  Mid-loop (it < maxit - 1) svihmm_svi_iteration has already
                # pre-launched iteration it + 1's k_svi_globals into the handle's single ltran /
                # mod_init buffers, so mod_init / mod_tran then hold the psi-expectations of the
                # UPDATED var_tran -- one global step ahead of reference :502-504.  Nothing on the
                # path reads them before the next iteration overwrites them (pred_logprob_full
                # computes its own, :1157-1159); only a caller inspecting the attributes from
                # inside a validation hook sees the difference.
                if loop_globals_live and hasattr(eng, "read_globals"):
                    self.mod_init, self.mod_tran = eng.read_globals()
                tmp = self.pred_logprob_full()
                loop_globals_live = False
                self.pred_logprob_full_mean[it] = np.nanmean(tmp)
                self.pred_logprob_full_std[it] = np.nanstd(tmp)
        wall["submit_iterations"] = (time.perf_counter() - t_mark) * 1e3
        t_mark = time.perf_counter()
        if not host_fresh:
            self._svi_pull_state()
        e, ms = eng.svi_read_elbo(maxit)
        self.elbo_vec[:] = e
        self.iter_time[:] = ms * 1e-3
        wall["wait_and_read_state"] = (time.perf_counter() - t_mark) * 1e3
        t_mark = time.perf_counter()
        # the reference leaves the last local_update's psi-expectations on the object (:502-504).
        # (A validation hook after the last iteration has overwritten the handle's copy: they were
        #  read before it ran.  The loop always runs to maxit, so no globals kernel of a further
        #  iteration has been pre-launched into the handle's buffers at this point.)
        if loop_globals_live and hasattr(eng, "read_globals"):
            self.mod_init, self.mod_tran = eng.read_globals()
        if "_pending_rows" not in self.__dict__ and "_val_done" not in self.__dict__:
            self._register_last_window(eng, last)
        self.__dict__.pop("_val_done", None)
        wall["last_window"] = (time.perf_counter() - t_mark) * 1e3

    def _register_last_window(self, eng, last):
        """lliks / lalpha / lbeta / var_x of the last window of the last minibatch, fetched from
        the device on first access (what the reference leaves on the object, :405-436)."""
        if last is None or last[0] == 0:
            return
        nb, Lm = last
        self._pending_rows = ((nb - 1) * Lm, Lm, {"lliks", "lalpha", "lbeta", "var_x"})
        self._lZ = None
        self.__dict__["_val_done"] = True
        if hasattr(eng, "on_next_mutation"):
            ref = weakref.ref(self)
            eng.on_next_mutation(lambda: ref() is not None and ref()._resolve_pending())

    def _resolve_pending(self):
        pend = self.__dict__.get("_pending_rows")
        if pend is not None:
            for name in list(pend[2]):
                getattr(self, name)
            self.__dict__.pop("_pending_rows", None)

    def _pgauss_fastpath(self):
        # ProductGaussian emitters keep the route of a plugin this class does not know: host lliks through
        # expected_log_likelihood (the natural-gradient step here has no branch for the family)
        return False

    def _suffstats_route(self):
        """Whether the host loop takes the statistics of its windows' posteriors on the device
        (one ``engine.suffstats`` call per minibatch) instead of ``intermediate_pars`` on the host:
        only where that method, its buffered form and the arithmetic behind them are this class's,
        the emission family has device statistics and no communicator shards the minibatch."""
        for name in ("intermediate_pars", "intermediate_pars_buffer", "_intermediate"):
            if name in self.__dict__ or getattr(type(self), name) is not getattr(VBHMM, name):
                return False
        if self.comm is not None or not hasattr(self.engine, "suffstats"):
            return False
        return self._device_family()

    def _segments_inter(self, segs, A_inter, emit_inter):
        """``(A_inter, emit_inter)`` of the windows ``segs = [(loff, uoff, var_x), ...]``: what the
        serial accumulation of ``_intermediate(var_x, loff, uoff)`` gives (:398-436, quirk Q1 wrap),
        from one device call.  Posteriors whose shape is not that of their segment (a
        ``local_update`` override may leave anything behind) go the host way for the whole batch."""
        K = self.K
        Lm = segs[0][1] - segs[0][0] + 1
        if all(u - l + 1 == Lm and q.shape == (Lm, K) for l, u, q in segs):
            q = np.stack([q for _, _, q in segs])
            # (what local_update left on the engine, made sure of: all three uploads are idempotent)
            self._upload_obs()
            self._push_globals()
            self._push_emission()
            st = self.engine.suffstats(np.array([l for l, _, _ in segs], dtype=np.int64), Lm, q,
                                       flags=L.TRANS_WRAP)
            return self._stats_to_inter(st, len(segs))
        for l, u, q in segs:
            A_i, e_i = self._intermediate(q, l, u)
            A_inter += A_i
            for k in range(K):
                emit_inter[k] += e_i[k]
        return A_inter, emit_inter

    def _stats_to_inter(self, st, nwin):
        """Packed device statistics of ``nwin`` windows -> ``(A_inter, emit_inter)`` exactly as the
        serial accumulation of the reference (:398-436) would hold them."""
        K, D = self.K, self.D
        # quirk Q2: prior_tran - 1 is part of every window's A_i
        A_inter = st.A_raw + nwin * (self.prior_tran - 1.)
        if hasattr(st, "counts"):
            # Categorical (reference :907-926): every window contributes alpha_0 + counts - 1
            emit_inter = [nwin * (G.alphav_0 - 1.) + st.counts[k] for k, G in enumerate(self.var_emit)]
        elif hasattr(st, "col_counts"):
            # ProductCategorical: the same per column, the columns side by side
            emit_inter = [np.concatenate([nwin * (a0 - 1.) + c[k] for a0, c in zip(G.alphav_0, st.col_counts)])
                          for k, G in enumerate(self.var_emit)]
        elif hasattr(st, "sx"):
            # ProductPoisson: expected sufficient statistics [sum q c, sum q] per state and column
            emit_inter = [np.stack([st.sx[k], st.n[k]]) for k in range(K)]
        elif hasattr(st, "xsq"):
            # diagonal family: expected sufficient statistics [sum q x, n, sum q x^2, n] per state
            emit_inter = [np.stack([st.xbar[k], np.full(D, st.neff[k]), st.xsq[k], np.full(D, st.neff[k])])
                          for k in range(K)]
        else:
            emit_inter = _StackedStats(st.xbar.copy(), st.neff.copy(), st.S.copy())
        return A_inter, emit_inter

    def _minibatch_estep(self, minibatch, miniL, buffer=None):
        """All windows of the minibatch in one device E-step; returns
        ``(A_inter, emit_inter, lb)`` exactly as the serial accumulation of the
        reference (:398-436) would.  With a communicator the windows are sharded
        round-robin over the ranks and the packed statistics are all-reduced."""
        K, D = self.K, self.D
        Lm = 2 * miniL + 1
        # the previous iteration's lazily held window state is superseded, not fetched
        self.__dict__.pop("_pending_rows", None)
        eng = self.engine
        if hasattr(eng, "on_next_mutation"):
            eng.on_next_mutation(None)
        self._stationary_init()
        self._psi_expectations()
        comm = self.comm
        mine = minibatch if comm is None else minibatch[comm.rank::comm.size]
        starts = np.array([mo.i1 for mo in mine], dtype=np.int64)
        nwin = len(minibatch)
        inner = None
        if buffer is not None:
            bufferL, L_ = buffer
            inner = (bufferL - L_, 2 * L_ + 1)
        if len(starts):
            # emission factors before the globals: the device's upload -> Cholesky -> theta chain
            # is what the emission GEMM waits for, the globals are needed by the sweeps only
            # KEEP_LBETA: the reference leaves lbeta of the last window on the object
            flags = self._push_emission(windows=list(starts), Lm=Lm) | L.TRANS_WRAP | L.KEEP_LBETA
        else:
            flags = L.TRANS_WRAP
        self._push_globals()
        # an empty shard still produces (zero) statistics so every rank joins the all-reduce
        st = self.engine.estep(starts, Lm, flags=flags, read=(comm is None), inner=inner)
        if comm is not None:
            st = comm.allreduce_stats(self.engine, K, D)
        A_inter, emit_inter = self._stats_to_inter(st, nwin)
        lb = float(st.lb[0])
        # leave the object as the reference does after the loop: state of the last window
        self.cur_mo = minibatch[-1]
        if len(starts):
            b = len(starts) - 1
            # state of the last window, fetched on first access (valid until the next upload)
            self._pending_rows = (b * Lm, Lm, {"lliks", "lalpha", "lbeta", "var_x"})
            self._lZ = None
            # any later engine call that uploads parameters or reuses the intermediate buffers
            # (pred_logprob_full, full_local_update, select_L, local_update, ...) first lets this
            # object fetch those rows while they are still the last window's
            if hasattr(eng, "on_next_mutation"):
                ref = weakref.ref(self)
                eng.on_next_mutation(lambda: ref() is not None and ref()._resolve_pending())
        return A_inter, emit_inter, lb

    # -- single meta-observation local update (reference :487-519) ----------------------------
    def local_update(self, metaobs=None):
        if metaobs is None:
            loff, uoff = 0, self.T - 1
        else:
            loff, uoff = metaobs.i1, metaobs.i2
        Lm = uoff - loff + 1
        self._psi_expectations()
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission(windows=[loff], Lm=Lm)
        if (type(self).forward_msgs is not VBHMM.forward_msgs
                or type(self).backward_msgs is not VBHMM.backward_msgs):
            self._local_update_literal([loff], Lm, flags, metaobs if metaobs is not None else MetaObs(loff, uoff))
            return
        r = self.engine.forward_backward([loff], Lm, flags=flags)
        self.lalpha = r["lalpha"][0]
        self.lbeta = r["lbeta"][0]
        self.var_x = r["var_x"][0]
        self._lZ = float(r["local_lb"][0])
        self.lliks = self.engine.read_intermediate("lliks", 1, Lm)[0]

    # -- adaptive window length (reference :521-661) --------------------------------------------
    def _local_messages_batch(self, centers, halflength):
        """var_x of the windows centred at ``centers`` (all of half-width
        ``halflength``) in one device call; what ``get_local_messages`` returns, batched."""
        Lm = 2 * halflength + 1
        starts = np.asarray(centers, dtype=np.int64) - halflength
        self._upload_obs()
        flags = self._push_emission(windows=list(starts), Lm=Lm)
        r = self.engine.forward_backward(starts, Lm, flags=flags, want=("var_x",))
        return r["var_x"]

    def _prepare_messages(self):
        # reference get_local_messages recomputes these every call (:675-677)
        self._psi_expectations()
        self._push_globals()

    # the growth rules of select_L / select_buffer in one device call (``svihmm_grow_windows``); False: the
    # lock-step host loops below, one device E-step per candidate
    device_growth = True

    def _device_growth_ok(self):
        """The device route applies: the engine offers it, the emission family lives on the device (no
        host-evaluated lliks) and the type overrides none of the per-window message hooks the host loop
        would call."""
        if not self.device_growth or not hasattr(self.engine, "grow_windows"):
            return False
        if not self._device_family():
            return False
        cls = type(self)
        return all(getattr(cls, nm) is getattr(VBHMM, nm)
                   for nm in ("get_local_messages", "get_marginal", "get_forward", "get_backward"))

    def _grow_on_device(self, indices, half0, probe_off, Lincrement, Lcutoff, epsilon, rule):
        if not len(indices):
            return -1
        self._upload_obs()
        flags = self._push_emission()
        half, _, _ = self.engine.grow_windows(indices, half0, probe_off=probe_off, increment=Lincrement,
                                              cutoff=Lcutoff, epsilon=epsilon, rule=rule, flags=flags)
        return int(np.max(half))

    def select_L(self, numIndices=1, epsilon=1e-5, minHalfL=1, avgResidual=False,
                 Lincrement=1, Lcutoff=1000):
        """reference :521-569; the per-index growth loops run in lock-step so every
        candidate L is one batched device E-step over the still-active indices."""
        indices = npr.choice(self.T - 2 * minHalfL - 1, size=numIndices) + minHalfL
        self._prepare_messages()
        n = len(indices)
        if self._device_growth_ok():
            return self._grow_on_device(indices, minHalfL, 0, Lincrement, Lcutoff, epsilon, 1 if avgResidual else 0)
        Lcur = np.full(n, minHalfL, dtype=int)
        q_old = self._local_messages_batch(indices, minHalfL)[:, minHalfL, :]
        q_diff = np.full(n, np.finfo(np.float64).max)
        count = np.zeros(n, dtype=int)
        run_av = np.zeros(n); run_old = np.zeros(n)
        active = np.ones(n, dtype=bool)
        while True:
            for i in np.where(active)[0]:
                ind, Li = indices[i], Lcur[i]
                if ind - Li < 1 + Lincrement or ind + Li + Lincrement + 1 > self.T or Li > Lcutoff:
                    active[i] = False
                    continue
                if not avgResidual:
                    if q_diff[i] < epsilon:
                        active[i] = False
                else:
                    count[i] += 1
                    if count[i] > 1 and (run_av[i] - run_old[i]) / (count[i] - 1) < epsilon:
                        active[i] = False
            if not active.any():
                break
            # all active indices share the same L (they start together, grow together)
            idx = np.where(active)[0]
            Lnew = Lcur[idx[0]] + Lincrement
            q_new = self._local_messages_batch(indices[idx], Lnew)[:, Lnew, :]
            d = np.sum(np.abs(q_new - q_old[idx]), axis=1)
            if not avgResidual:
                q_diff[idx] = d
            else:
                run_old[idx] = run_av[idx]
                run_av[idx] += d
            q_old[idx] = q_new
            Lcur[idx] = Lnew
        return int(np.max(Lcur)) if n else -1

    def buffer_budget(self, halfL, budget=400):
        return int(np.ceil(budget / (2 * halfL + 1)))

    def select_buffer(self, numIndices=1, epsilon=1e-5, halfL=10,
                      avgResidual=False, Lincrement=1, Lcutoff=1000):
        """reference :579-661 (non-avgResidual branch; the avgResidual branch of the
        reference uses ``var_new`` before assignment, :648, and cannot run)."""
        if avgResidual:
            raise RuntimeError("select_buffer(avgResidual=True) is broken in the reference "
                               "(hmmsgd_metaobs.py:648 uses var_new before assignment)")
        indices = npr.choice(self.T - 2 * halfL - 1, size=numIndices) + halfL
        self._prepare_messages()
        n = len(indices)
        if self._device_growth_ok():
            return self._grow_on_device(indices, halfL, halfL, Lincrement, Lcutoff, epsilon, 0)
        bufL = np.full(n, halfL, dtype=int)
        v0 = self._local_messages_batch(indices, halfL)
        q_old_left = v0[:, 0, :].copy()
        q_old_right = v0[:, 2 * halfL, :].copy()
        dl = np.full(n, np.finfo(np.float64).max)
        dr = dl.copy()
        active = np.ones(n, dtype=bool)
        while True:
            for i in np.where(active)[0]:
                ind, b = indices[i], bufL[i]
                if ind - b < 1 + Lincrement or ind + b + Lincrement + 1 > self.T or b > Lcutoff:
                    active[i] = False
                elif dl[i] < epsilon and dr[i] < epsilon:
                    active[i] = False
            if not active.any():
                break
            idx = np.where(active)[0]
            bnew = bufL[idx[0]] + Lincrement
            v = self._local_messages_batch(indices[idx], bnew)
            ql = v[:, bnew - halfL, :]
            qr = v[:, bnew + halfL, :]
            dl[idx] = np.sum(np.abs(ql - q_old_left[idx]), axis=1)
            dr[idx] = np.sum(np.abs(qr - q_old_right[idx]), axis=1)
            q_old_left[idx] = ql
            q_old_right[idx] = qr
            bufL[idx] = bnew
        return int(np.max(bufL)) if n else -1

    def get_local_messages(self, ind, halflength):
        """reference :663-700: var_x of the window centred at ``ind``."""
        self._prepare_messages()
        return self._local_messages_batch([ind], halflength)[0]

    def get_marginal(self, var_over_x, index):
        return np.squeeze(var_over_x[index, :])

    def _messages(self, metaobs, lliks, mod_tran, mod_init, want):
        self.engine.set_globals(mod_init, mod_tran)
        self.engine.set_lliks(np.ascontiguousarray(lliks)[None])
        r = self.engine.forward_backward(None, lliks.shape[0], flags=L.USE_HOST_LLIKS,
                                         want=(want,), B=1)
        return r[want][0]

    def get_forward(self, metaobs, lliks, mod_tran, mod_init):
        """reference :711-740."""
        return self._messages(metaobs, lliks, mod_tran, mod_init, "lalpha")

    def get_backward(self, metaobs, lliks, mod_tran):
        """reference :742-771."""
        return self._messages(metaobs, lliks, mod_tran, np.zeros(self.K), "lbeta")

    def forward_msgs(self, metaobs=None):
        """reference :775-803."""
        self.lalpha = self._messages(metaobs, self.lliks, self.mod_tran, self.mod_init, "lalpha")
        self._lZ = None

    def backward_msgs(self, metaobs=None):
        """reference :828-855."""
        self.lbeta = self._messages(metaobs, self.lliks, self.mod_tran, self.mod_init, "lbeta")

    def forward_msgs_real_data(self, lalpha_init=None):
        """reference :805-826 (whole chain)."""
        if lalpha_init is not None:
            raise RuntimeError("lalpha_init override is not supported on the device path")
        self._upload_obs()
        self._push_globals()
        flags = self._push_emission()
        r = self.engine.forward_backward([0], self.T, flags=flags, want=("lalpha",))
        return r["lalpha"][0]

    # -- natural-gradient direction of ONE window from host arrays (reference :857-1008) -------
    def intermediate_pars(self, metaobs=None):
        if metaobs is None:
            loff, uoff = 0, self.T
        else:
            loff, uoff = metaobs.i1, metaobs.i2
        return self._intermediate(self.var_x, loff, uoff)

    def intermediate_pars_buffer(self, metaobs, bufferL, L_):
        if metaobs is None:
            loff, uoff = 0, self.T
        else:
            loff, uoff = metaobs.i1 + bufferL - L_, metaobs.i2 - bufferL + L_
        return self._intermediate(self.var_x[bufferL - L_:bufferL + L_ + 1, :], loff, uoff)

    def _intermediate(self, var_x, loff, uoff):
        obs = self.obs
        mask = self.mask
        tran_mf = self.prior_tran.copy()
        for t in range(loff, uoff + 1):
            tran_mf += np.outer(var_x[t - loff - 1, :], var_x[t - loff, :])
        A_inter = tran_mf - 1.
        inds = np.logical_not(mask[loff:(uoff + 1)])
        emit_inter = list()
        if is_niw_gaussian(self.var_emit[0]):
            for k in range(self.K):
                G = self.var_emit[k]
                weights = var_x[inds, k]
                emit_inter.append(util.NIW_suffstats(G, obs[loff:(uoff + 1), :][inds, :], weights))
        elif is_diag_gaussian(self.var_emit[0]):
            x = obs[loff:(uoff + 1), :][inds, :]
            for k in range(self.K):
                n, sx, sxx = self.var_emit[k]._get_weighted_statistics(x, var_x[inds, k])
                emit_inter.append(np.stack([sx, np.full(x.shape[1], n), sxx, np.full(x.shape[1], n)]))
        elif type(self.var_emit[0]) is Categorical:
            for k in range(self.K):
                G = self.var_emit[k]
                w = var_x[inds, k]
                data = np.asarray(obs[loff:(uoff + 1)][inds]).astype(int).ravel()
                C = G.num_parameters()
                z = np.zeros((data.shape[0], C))
                z[np.arange(data.shape[0]), data] = 1
                wz = w[:, None] * z
                alpha_mf = G._posterior_hypparams(*G._get_weighted_statistics(data, wz))
                emit_inter.append(alpha_mf - 1.)
        elif type(self.var_emit[0]) is ProductCategorical:
            # the Categorical branch per column, over the rows whose entry is present: alpha_0 + counts - 1
            xi, ok = self.var_emit[0]._present(obs[loff:(uoff + 1)][inds])
            for k in range(self.K):
                G = self.var_emit[k]
                w = var_x[inds, k]
                cols = []
                for d, a0 in enumerate(G.alphav_0):
                    z = np.zeros((xi.shape[0], len(a0)))
                    z[np.where(ok[:, d])[0], xi[ok[:, d], d]] = 1
                    cols.append(a0 + (w[:, None] * z).sum(0) - 1.)
                emit_inter.append(np.concatenate(cols))
        elif type(self.var_emit[0]) is ProductPoisson:
            x = obs[loff:(uoff + 1)][inds]
            for k in range(self.K):
                sx, n = self.var_emit[k]._get_weighted_statistics(x, var_x[inds, k])
                emit_inter.append(np.stack([sx, n]))
        return A_inter, emit_inter

    # -- global natural-gradient step (reference :1010-1084) -------------------------------------
    def global_update(self, A_inter, emit_inter):
        lrate = self.lrate
        L_ = self.metaobs_half
        S = self.mb_sz
        T = self.T

        nats_old = self.var_tran - 1.
        bfact = (T - 2 * L_ - 1) / (2. * L_ * S)
        A_up = bfact * A_inter
        if self.adagrad:
            self.ada_G += nats_old ** 2
            adaMatrix = self.ada_G ** .25
            nats_new = (1. - 1.0 / adaMatrix) * nats_old + A_up / adaMatrix
        else:
            nats_new = (1. - lrate) * nats_old + lrate * A_up
        self.var_tran = nats_new + 1.

        bfact = (T - 2 * L_ - 1) / ((2. * L_ + 1.) * S)
        if self._niw_fastpath() and isinstance(emit_inter, _StackedStats):
            self._global_update_niw_stacked(lrate, bfact, emit_inter)
        elif is_niw_gaussian(self.var_emit[0]):
            for k in range(self.K):
                G = self.var_emit[k]
                nats_old = util.NIW_mf_natural_pars(G.mu_mf, G.sigma_mf, G.kappa_mf, G.nu_mf)
                prior_hypparam = util.NIW_mf_natural_pars(G.mu_0, G.sigma_0, G.kappa_0, G.nu_0)
                nats_new = (1. - lrate) * nats_old \
                    + lrate * (prior_hypparam + bfact * emit_inter[k])
                util.NIW_mf_moment_pars(G, *nats_new)
        elif is_diag_gaussian(self.var_emit[0]):
            # the Gaussian branch's blend (reference :1050-1069) in the diagonal family's natural
            # parameters [nus mu, nus, 2 betas + nus mu^2, 2 alphas] (an extension: the reference
            # dispatches on Gaussian / Categorical only)
            for k in range(self.K):
                G = self.var_emit[k]
                nats_old = G.to_natural(G.mf_mu, G.mf_nus, G.mf_alphas, G.mf_betas)
                prior_hypparam = G.to_natural(G.mu_0, G.nus_0, G.alphas_0, G.betas_0)
                nats_new = (1. - lrate) * nats_old + lrate * (prior_hypparam + bfact * emit_inter[k])
                G._set_mf(*G.from_natural(nats_new))
        elif type(self.var_emit[0]) is Categorical:
            for k in range(self.K):
                G = self.var_emit[k]
                nats_old = G.alpha_mf - 1.
                nats_new = (1. - lrate) * nats_old + lrate * bfact * emit_inter[k]
                G._alpha_mf = nats_new + 1.
                G.weights = G._alpha_mf / G._alpha_mf.sum()
        elif type(self.var_emit[0]) is ProductCategorical:
            # the Categorical rule element by element (emit_inter[k]: the D columns side by side)
            for k in range(self.K):
                G = self.var_emit[k]
                nats_old = np.concatenate(G.alpha_mf) - 1.
                nats_new = (1. - lrate) * nats_old + lrate * bfact * emit_inter[k]
                G._set_alpha(np.split(nats_new + 1., np.cumsum(G.V)[:-1]))
        elif type(self.var_emit[0]) is ProductPoisson:
            # the Gaussian branch's blend (reference :1050-1069, the prior once) in the Gamma natural parameters
            # (a - 1, -b): their offsets cancel, and the factors stay positive for every lrate in [0, 1]
            for k in range(self.K):
                G = self.var_emit[k]
                sx, n = emit_inter[k]
                G._set_mf((1. - lrate) * G.alpha_mf + lrate * (G.alpha_0 + bfact * sx),
                          (1. - lrate) * G.beta_mf + lrate * (G.beta_0 + bfact * n))

    def _global_update_niw_stacked(self, lrate, bfact, E):
        """The K-loop of reference :1050-1069 + util.py:28-60 on stacked arrays: the same
        element-wise arithmetic (so the same floating-point results), without 4K small
        NumPy object-array operations per iteration."""
        ve = self.var_emit
        D = self.D
        mu, sg, ka, nu = self._emission_arrays()
        mu0, sg0, ka0, nu0 = self._prior_arrays()

        def nat(m, s_, k_, n_):          # util.NIW_mf_natural_pars
            return (k_[:, None] * m, k_, s_ + np.einsum('ki,kj->kij', m, m) * k_[:, None, None],
                    n_ + 2 + D)
        o = nat(mu, sg, ka, nu)
        p0 = nat(mu0, sg0, ka0, nu0)
        e = (E.xbar, E.neff, E.S, E.neff)
        new = [(1. - lrate) * o[i] + lrate * (p0[i] + bfact * e[i]) for i in range(4)]
        m_new = new[0] / new[1][:, None]                       # util.NIW_mf_moment_pars
        k_new = new[1]
        s_new = new[2] - np.einsum('ki,kj->kij', m_new, m_new) * k_new[:, None, None]
        n_new = new[3] - 2 - D
        for k, G in enumerate(ve):
            G.mu_mf = m_new[k]; G.sigma_mf = s_new[k]
            G.kappa_mf = k_new[k]; G.nu_mf = n_new[k]
            G.mu = G.mu_mf
            G.sigma = G.sigma_mf / (G.nu_mf - D - 1)

    # -- predictive log-probabilities (reference :1086-1145) ----------------------------------------
    def pred_logprob(self, metaobs=None):
        cur_mo = self.cur_mo
        if metaobs is None:
            metaobs = cur_mo
        if ((metaobs is not cur_mo) and
                (metaobs.i1 != cur_mo.i1 and metaobs.i2 != cur_mo.i2)):  # quirk Q14 ("and")
            self.local_update(metaobs=metaobs)
        K = self.K
        loff, uoff = metaobs.i1, metaobs.i2
        obs_full = getattr(self, 'obs_full', self.obs)   # infer never sets obs_full (Q14)
        obs = obs_full[loff:(uoff + 1), :]
        mask = self.mask[loff:(uoff + 1)]
        nmiss = np.sum(mask)
        if nmiss == 0:
            return None
        logprob = np.zeros((nmiss, K))
        for k, odist in enumerate(self.var_emit):
            logprob[:, k] = np.log(self.var_x[mask, k] + eps) \
                + odist.expected_log_likelihood(obs[mask, :])
        return np.mean(np.logaddexp.reduce(logprob, axis=1))

    def pred_logprob_full(self):
        obs_full = getattr(self, 'obs_full', self.obs)
        if self._niw_fastpath() and obs_full is self.obs:
            # whole computation on the device (chain E-step as a blocked scan, emission term of
            # the held-out rows, reduction): two doubles come back instead of var_x[T,K]
            mod_init = digamma(self.var_init + eps) - digamma(np.sum(self.var_init) + eps)
            tran_sum = np.sum(self.var_tran, axis=1)
            mod_tran = digamma(self.var_tran + eps) - digamma(tran_sum[:, npa] + eps)
            self._upload_obs()
            self.engine.set_globals(mod_init, mod_tran)
            flags = self._push_emission(nan_mask=True)
            val, _ = self.engine.pred_logprob([0], self.T, flags=flags)
            return val
        full_var_x = self.full_local_update()
        K = self.K
        obs = getattr(self, 'obs_full', self.obs)
        mask = self.mask
        nmiss = np.sum(mask)
        if nmiss == 0:
            return None
        logprob = np.zeros((nmiss, K))
        for k, odist in enumerate(self.var_emit):
            logprob[:, k] = np.log(full_var_x[mask, k] + eps) \
                + odist.expected_log_likelihood(obs[mask, :])
        return np.mean(np.logaddexp.reduce(logprob, axis=1))

    def _full_estep_device(self):
        """full_local_update without the var_x readback (hamming_dist(None, true_sts))."""
        mod_init = digamma(self.var_init + eps) - digamma(np.sum(self.var_init) + eps)
        tran_sum = np.sum(self.var_tran, axis=1)
        mod_tran = digamma(self.var_tran + eps) - digamma(tran_sum[:, npa] + eps)
        self._upload_obs()
        self.engine.set_globals(mod_init, mod_tran)
        flags = self._push_emission(nan_mask=True)
        self.engine.forward_backward([0], self.T, flags=flags, want=())

    def _expect_prepare(self):
        """``reconstruct()`` / ``impute()`` need posteriors of all T rows; this class's last batch is a minibatch of
        windows.  Where the engine does not hold the whole chain's batch, ``full_local_update()`` runs first: on an
        engine with ``posterior_expect`` its rows stay in HBM for the device call, elsewhere the returned ``var_x``
        is averaged on the host.  The window attributes (``var_x`` of the last window) stay as they are."""
        if self._expect_engine() is not None:
            return None
        var_x = self.full_local_update()
        return None if self._expect_engine() is not None else var_x

    def full_local_update(self):
        """Whole-chain E-step with missing rows treated as NaN (lliks row = 0),
        reference :1147-1205.  obs is not mutated (the reference NaN-masks it in place
        and restores it); returns var_x[T,K]."""
        mod_init = digamma(self.var_init + eps) - digamma(np.sum(self.var_init) + eps)
        tran_sum = np.sum(self.var_tran, axis=1)
        mod_tran = digamma(self.var_tran + eps) - digamma(tran_sum[:, npa] + eps)
        self._upload_obs()
        self.engine.set_globals(mod_init, mod_tran)
        flags = self._push_emission(nan_mask=True)
        r = self.engine.forward_backward([0], self.T, flags=flags, want=("var_x",))
        return r["var_x"][0]
