/* svihmm.h -- C ABI of the MI355X-native SVI-HMM E-step engine (libsvihmm_hip.so).
 *
 * This is the drop-in boundary for the hot path of dillonalaird/pysvihmm:
 *   emission expected log-likelihood -> log-domain forward/backward ->
 *   posterior marginals -> expected sufficient statistics (natural-gradient
 *   direction) -> (all-reduce) -> host global step.
 * The reference has a single native boundary on this path, the Cython function
 *   hmm_fast.FFBS(self, var_init, lalpha_init=None)          (hmm_fast.pyx:43-124)
 * bound as VariationalHMMBase.ffbs_fast (hmmbase.py:409-411); everything else on
 * the path is NumPy inside Python methods.  Each entry point below names the
 * reference code (file:line under /root/reference) whose arithmetic it replaces.
 *
 * Conventions
 *   - Plain C: pointers + sizes, no C++/torch types.  All arrays are C-contiguous
 *     row-major float64 unless stated; "host" pointers are borrowed for the call
 *     only (caller keeps ownership); the library owns all device memory behind
 *     the opaque handle.
 *   - Every function returns 0 on success, non-zero on failure; the message of
 *     the last failure on the calling thread is svihmm_last_error().  The Python
 *     host raises RuntimeError (the reference's only exception type,
 *     hmmbase.py:134, hmmsgd_metaobs.py:76,177,191,344).
 *   - One thread per handle, one handle per device (the reference is
 *     single-threaded and non-re-entrant).  Calls are synchronous with respect to
 *     their host output buffers; device work runs on the handle's own HIP stream.
 *   - A "window" is a meta-observation (hmmsgd_metaobs.py:42-45): Lm consecutive
 *     rows of obs starting at starts[b] (inclusive bounds i1=starts[b],
 *     i2=starts[b]+Lm-1).  A full-chain E-step is B=1, starts={0}, Lm=T.
 */
#ifndef SVIHMM_H
#define SVIHMM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* 3 (addition, nothing else changed meaning): svihmm_svi_begin_mcat, svihmm_svi_begin_poisson.
 * 3 (addition, nothing else changed meaning): svihmm_estep_sequence_subset.
 * 3 (addition, nothing else changed meaning): svihmm_viterbi_sequences, svihmm_ffbs_sequences.
 * 3 (addition, nothing else changed meaning): svihmm_set_sequences, svihmm_estep_sequences.
 * 3 (addition, nothing else changed meaning): svihmm_grow_windows.
 * 3 (addition, nothing else changed meaning): svihmm_ffbs_windows.
 * 3 (addition, nothing else changed meaning): svihmm_viterbi.
 * 3: svihmm_export_packed / svihmm_import_packed, svihmm_svi_set_adagrad / _read_adagrad,
 *    svihmm_svi_begin_diag / _begin_cat / _read_factors added, slot mask
 *    of svihmm_profile_enable (round 4; nothing else changed meaning).
 * 2: svihmm_get_shift added, svihmm_shift_obs no longer changes what later calls mean (the shift is
 *    the handle's business), svihmm_set_emission_diag added; 1 was rounds 1-2 (svi_*,
 *    set_precision, shift_obs, ffbs_sample, comm_count were added under it). */
#define SVIHMM_ABI_VERSION 3

typedef struct svihmm_ctx svihmm_ctx;

/* ---- flags ------------------------------------------------------------------ */
/* Masked rows are treated as NaN rows when computing lliks (-> lliks row = 0):
 * full_local_update semantics, hmmsgd_metaobs.py:1166-1168,1176.  Without it
 * masked rows still contribute to lliks (infer() semantics, quirk Q9,
 * hmmsgd_metaobs.py:314-315 commented out). */
#define SVIHMM_MASK_AS_NAN 1u
/* Transition statistic sum_{t=0}^{Lm-1} q[t-1] (x) q[t] with t-1 wrapping to the
 * window's last row (quirk Q1, hmmsgd_metaobs.py:877-878).  Without it the batch
 * form sum_{t=1}^{Lm-1} (hmmbatchcd.py:183-184, hmmbatchsgd.py:224-225). */
#define SVIHMM_TRANS_WRAP 2u
/* Use the lliks previously uploaded with svihmm_set_lliks (generic emission
 * plugin route) instead of evaluating the NIW emission kernel. */
#define SVIHMM_USE_HOST_LLIKS 4u
/* svihmm_estep_minibatch only: also write lbeta to HBM during the sweep (the log-domain fused
 * backward sweep otherwise keeps it in registers).  A hint: without it a later read of lbeta
 * costs one more backward sweep over the lliks still held (and fails once the parameters have
 * changed); the scaled sweeps rebuild all logs on demand and ignore the flag. */
#define SVIHMM_KEEP_LBETA 8u

/* svihmm_svi_iteration only: make the log-domain lliks / lalpha / lbeta of the batch's LAST window
 * readable (svihmm_read_rows) after the call -- they are otherwise rebuilt on demand from the
 * current parameters, which the iteration's global step replaces.  The reference leaves the
 * state of the last meta-observation on the object (hmmsgd_metaobs.py:405-436). */
#define SVIHMM_SVI_KEEP_WINDOW 16u
#define SVIHMM_SVI_MIN_PSEUDOCOUNT 2.5e-3

/* ---- errors / lifecycle ------------------------------------------------------- */
const char* svihmm_last_error(void);
int svihmm_abi_version(void);
int svihmm_device_count(int* n_out);
int svihmm_create(int device_id, svihmm_ctx** out);
int svihmm_destroy(svihmm_ctx* h);
int svihmm_sync(svihmm_ctx* h);

/* ---- precision mode -----------------------------------------------------------------
 * SVIHMM_F64 (default): the reference's own type throughout (hmmbase.py:102-103).
 * SVIHMM_F32: north_star's second tolerance ("posteriors and natural gradients within 1e-3 fp32").
 *   For the E-step fast path it covers -- NIW emissions, K <= 64, window batches (not the
 *   whole-chain scan, not host-supplied lliks) -- the scaled emission likelihoods and the scaled
 *   forward / backward messages are STORED as fp32 (half the HBM traffic of the sweeps) and the
 *   expected-sufficient-statistics GEMM runs on v_mfma_f32_16x16x4_f32 (twice the matrix rate),
 *   each row chunk accumulated in fp32 and the chunks reduced in fp64.  The emission quadratic
 *   form of batches from 8192 rows (D <= 32; from 32768 rows at D <= 64) is evaluated CENTRED, c_k - |U_k x + b_k|^2 with
 *   U_k = sqrt(nu_k/2) L_k^-1, on the bf16 matrix pipe: x and U_k as three bf16 terms each (= the
 *   values to fp32 accuracy), six products into fp32 accumulators (round 3; the expanded feature
 *   form of the fp64 kernels cancels ~1e5 : 1, which fp32 cannot carry -- smaller batches and
 *   D > 32 keep that fp64 GEMM).  The arithmetic of the recursion itself stays fp64 (exact
 *   binary exponents; the launch is HBM-bound, not flop-bound).  Inputs and outputs of the ABI
 *   stay float64.
 *   Round 5: the centred bf16 x 3 emission covers D <= 64 (64-dimension pair records), the statistics GEMM on
 *   the bf16 pipe covers D <= 64 and wide models, and NIW models with 64 < K <= 256, D <= 64 run the whole fast
 *   path in the fp32 format from 32 768 rows and 192 windows per batch (BASELINE configs[4]: 19 instead of 45 ms
 *   per epoch step, statistics within 3.2e-4 of fp64).
 *   Calls outside that fast path run in fp64 regardless (smaller batches of wide models, other families,
 *   whole-chain scans, host-supplied lliks, transition expectations outside a float's range);
 *   svihmm_get_precision reports whether the last E-step batch actually ran in the fp32 format. */
#define SVIHMM_F64 0
#define SVIHMM_F32 1
int svihmm_set_precision(svihmm_ctx* h, int32_t mode);
int svihmm_get_precision(svihmm_ctx* h, int32_t* mode_out, int32_t* last_batch_f32_out);

/* ---- inputs ----------------------------------------------------------------- */
/* obs[T,D], mask[T] (1 = missing, may be NULL): hmmbase.py:60-65,122-123.
 * Copied to HBM once; NaN entries are preserved.
 * Coordinates: the resident copy is kept CENTRED, obs_dev[t] = obs[t] - c, with c chosen by the
 * library at upload (a point inside the data: column means of a row sample; svihmm_generate: the
 * average of the state means; svihmm_alloc_obs: taken from the first block that arrives) because
 * the emission GEMM evaluates the NIW quadratic form expanded around the resident copy's origin
 * and loses ~5e-16 (mu-c)'W(mu-c) to cancellation.  The model is shift-equivariant and c never
 * shows at this boundary: every mean that comes in (svihmm_set_emission_niw / _diag,
 * svihmm_svi_begin, svihmm_set_emission_prior, svihmm_niw_vlb_terms) or goes out
 * (svihmm_svi_read_state) and all statistics (svihmm_estep_minibatch*, svihmm_read_packed) are in
 * the CALLER's coordinates, exactly as the reference evaluates everything in the coordinates of
 * self.obs (hmmbase.py:219-229).  Only svihmm_allreduce_packed touches it internally: every rank
 * has its own c, so the sum is formed in the common caller coordinates. */
int svihmm_set_obs(svihmm_ctx* h, const double* obs, int64_t T, int32_t D,
                   const uint8_t* mask);

/* The same resident copy filled in pieces (gen_synthetic.py:188-191 read_data_mmap streams
 * [size, D] blocks of the on-disk float64 array): svihmm_alloc_obs sizes it (mask zeroed when
 * with_mask), svihmm_set_obs_rows uploads rows [row0, row0+nrows) and returns when the block
 * is on the device.  Rows never written are undefined. */
int svihmm_alloc_obs(svihmm_ctx* h, int64_t T, int32_t D, int32_t with_mask);
/* Moves the library's centre: c += shift[D] (resident copy, device-side NIW state and prior of a
 * running SVI loop follow; NaN rows stay NaN).  Purely a conditioning hint -- no later call
 * changes its meaning, results stay in the caller's coordinates.  Useful when the automatic
 * centre is poor (strongly drifting data) or was switched off.  svihmm_get_shift reads c[D]. */
int svihmm_shift_obs(svihmm_ctx* h, const double* shift);
int svihmm_get_shift(svihmm_ctx* h, double* shift_out);
int svihmm_set_obs_rows(svihmm_ctx* h, int64_t row0, int64_t nrows, const double* obs,
                        const uint8_t* mask);

/* mod_init[K], ltran[K,K] in the log domain: the psi-expectations of
 * hmmbase.py:214-216 / hmmsgd_metaobs.py:502-504 (computed on the host with
 * SciPy's digamma, uploaded once per minibatch).  The FFBS variant passes
 * ltran = log(var_tran + DBL_EPSILON) instead (hmm_fast.pyx:91-93).
 * Dynamic range: the fast recursions carry exp(ltran).  If any entry lies below
 * SVIHMM_LTRAN_LINEAR_MIN (Dirichlet pseudo-counts of ~2e-3 and less: psi(1e-3) = -1000, not
 * representable) every recursion with these globals runs the reference's own
 * np.logaddexp.reduce form instead (hmmbase.py:295, 319; one exp per state PAIR and step --
 * correct, 5-7x slower); the fp32 mode needs entries above
 * SVIHMM_LTRAN_F32_MIN and computes in fp64 otherwise. */
#define SVIHMM_LTRAN_LINEAR_MIN (-600.0)
#define SVIHMM_LTRAN_F32_MIN (-60.0)
int svihmm_set_globals(svihmm_ctx* h, int32_t K, const double* mod_init,
                       const double* ltran);

/* NIW mean-field emission factors mu[K,D], sigma[K,D,D], kappa[K], nu[K]
 * (pybasicbayes Gaussian.{mu_mf,sigma_mf,kappa_mf,nu_mf}); replaces the K calls
 * odist.expected_log_likelihood(obs) at hmmbase.py:219-220,
 * hmmsgd_metaobs.py:508-509,685-686,815-816,1175-1176, hmm_fast.pyx:84-85.
 * The Cholesky factorisation runs on the device and the call does not wait for it: a
 * sigma that is not positive definite is reported by the next synchronising call
 * (svihmm_sync, svihmm_loglik, svihmm_forward_backward, svihmm_estep_minibatch with an
 * output buffer, svihmm_read_packed).  Reported the same way: a factor so far from the library's
 * centre c of the resident observations for its spread ((mu-c)' (nu/2 sigma^-1) (mu-c) > 1e9,
 * i.e. a state mean > 3e4 standard deviations away from the data) that the emission GEMM -- which
 * evaluates the quadratic form expanded around c -- would lose more than 5e-7 in the
 * log-likelihoods; svihmm_shift_obs moves the centre.
 * D <= SVIHMM_NIW_MAX_D; wider observations go the svihmm_set_lliks route (the classes do). */
#define SVIHMM_NIW_MAX_D 96
int svihmm_set_emission_niw(svihmm_ctx* h, int32_t K, int32_t D, const double* mu,
                            const double* sigma, const double* kappa,
                            const double* nu);

/* Diagonal-covariance Gaussian factors (pybasicbayes DiagonalGaussian; BASELINE configs[0]; the
 * plugin objects the reference evaluates at hmmbase.py:219-220 and updates with
 * meanfieldupdate at hmmbatchcd.py:189): per state and dimension a normal-inverse-gamma mean-field
 * factor  sigma_d^2 ~ InvGamma(alphas, betas),  mu_d | sigma_d^2 ~ N(mu, sigma_d^2 / nus);  all four
 * arrays [K,D].  E_q log N(x | mu, diag sigma^2) is linear in the 2 D + 1 features (x_d^2, x_d, 1):
 * the emission and statistics GEMMs run on that feature table instead of the (D+1)(D+2)/2
 * products a full covariance needs (D = 32: 80 instead of 576 feature rows).  Afterwards the
 * packed statistics have the layout
 *     [ A_raw K*K | xbar K*D | neff K | xsq K*D | lb ]      (svihmm_packed_len)
 * with xsq[k,d] = sum over unmasked rows of q[t,k] x[t,d]^2 -- what the conjugate update needs
 * (nus += n, mu = (nus0 mu0 + xbar)/nus, alphas += n/2, betas += (xsq + nus0 mu0^2 - nus mu^2)/2).
 * Same asynchronous status word as svihmm_set_emission_niw (a non-positive nus / alphas / betas
 * entry, or a factor > 3e4 standard deviations from the data).  The device-resident SVI loop
 * (svihmm_svi_*) is NIW only; this family runs through svihmm_estep_minibatch*. */
#define SVIHMM_DIAG_MAX_D 128
int svihmm_set_emission_diag(svihmm_ctx* h, int32_t K, int32_t D, const double* mu,
                             const double* nus, const double* alphas, const double* betas);

/* Generic plugin route: lliks[B,Lm,K] evaluated by an arbitrary emission object on
 * the host (any object with expected_log_likelihood), already nan_to_num'ed. */
int svihmm_set_lliks(svihmm_ctx* h, const double* lliks, int32_t B, int32_t Lm);

/* ---- a3: emission expected log-likelihood ---------------------------------------- */
/* out_lliks[B,Lm,K] = nan_to_num(E_q log p(obs[starts[b]+t] | theta_k)). */
int svihmm_loglik(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm,
                  uint32_t flags, double* out_lliks);

/* ---- a4..a7: messages, posterior, local bound ------------------------------------- */
/* lalpha/lbeta/var_x [B,Lm,K], local_lb[B]; any output pointer may be NULL.
 *   lalpha : hmmbase.py:292-295 == hmmsgd_metaobs.py:800-803
 *   lbeta  : hmmbase.py:316-320 == hmmsgd_metaobs.py:851-855
 *   var_x  : hmmbase.py:226-229 == hmmsgd_metaobs.py:516-519
 *   local_lb[b] = sum_t LSE_k lalpha[b,t,k]  (hmmsgd_metaobs.py:271; quirk Q4) */
int svihmm_forward_backward(svihmm_ctx* h, const int64_t* starts, int32_t B,
                            int32_t Lm, uint32_t flags, double* out_lalpha,
                            double* out_lbeta, double* out_var_x,
                            double* out_local_lb);

/* ---- a3..a9: whole minibatch E-step -> packed expected sufficient statistics --- */
/* packed = [ A_raw(K*K) | xbar(K*D) | neff(K) | S(K*D*D) | lb(1) ], length
 * svihmm_packed_size(K,D):
 *   A_raw = sum_windows sum_t q[t-1] (x) q[t]       (hmmsgd_metaobs.py:876-878;
 *           the caller adds B*(prior_tran-1), quirk Q2)
 *   xbar_k, neff_k, S_k = sum over unmasked rows of q[t,k]*{x, 1, x x'}
 *                                                    (util.py:73-83, :884-904)
 *   lb    = sum_windows local_lb                     (hmmsgd_metaobs.py:436)
 * out_packed may be NULL: the result then stays in HBM for
 * svihmm_allreduce_packed / svihmm_read_packed. */
int64_t svihmm_packed_size(int32_t K, int32_t D);
int svihmm_estep_minibatch(svihmm_ctx* h, const int64_t* starts, int32_t B,
                           int32_t Lm, uint32_t flags, double* out_packed);
int svihmm_read_packed(svihmm_ctx* h, double* out_packed);
/* Buffered meta-observations (growBuffer): the E-step runs on windows of length Lm,
 * the statistics are taken over the inner segment [inner_off, inner_off+inner_len) of
 * each window only, with the wrap-around term inside that segment
 * (intermediate_pars_buffer, hmmsgd_metaobs.py:932-1008); lb still sums over the
 * whole window (hmmsgd_metaobs.py:436). */
int svihmm_estep_minibatch_ex(svihmm_ctx* h, const int64_t* starts, int32_t B,
                              int32_t Lm, int32_t inner_off, int32_t inner_len,
                              uint32_t flags, double* out_packed);

/* Expected sufficient statistics of posteriors the CALLER supplies (a message or local-update override
 * on the host: the reference's "Override this for specialized behavior", hmmbase.py:279,304), without
 * an E-step.  var_x [B,Lm,K] is host memory; row t of window b is the posterior of observation row
 * starts[b] + t, used as given (no renormalisation: zero rows and rows that do not sum to one are
 * fine).  K is the handle's (svihmm_set_globals) and must equal the emission family's.
 *   A_raw = sum_windows sum_t q[t-1] (x) q[t]:  with SVIHMM_TRANS_WRAP t = 0..Lm-1 and t-1 wrapping to
 *           the window's last row (hmmsgd_metaobs.py:876-878, quirk Q1; Lm = 1: the row is its own
 *           predecessor), without it t = 1..Lm-1 (hmmbatchcd.py:182-184);
 *   emission statistics over the unmasked rows (NaN symbols of a Categorical model skipped) in the
 *   packed layout of the current family (NIW, diagonal, Categorical), exactly as
 *   svihmm_estep_minibatch returns it, in the caller's coordinates (util.py:73-83, :884-904);
 *   lb = 0 (the caller adds B*(prior_tran-1), quirk Q2).
 * Buffered windows (intermediate_pars_buffer, hmmsgd_metaobs.py:932-1008): pass the inner segment's
 * posteriors with starts shifted to i1 + bufferL - L.  Always fp64 (the precision mode and what
 * svihmm_get_precision reports are unchanged).  The posteriors go to a device buffer of their own: the
 * intermediates of the last E-step (svihmm_read_intermediate / _read_rows, svihmm_state_argmax, the
 * kept window of svihmm_svi_iteration) read the same afterwards.  Transfers above 4 MB are staged
 * through pinned memory.  out_packed may be NULL (result in HBM for svihmm_read_packed /
 * svihmm_allreduce_packed / svihmm_export_packed).  Fails without resident observations or an
 * emission family, on a K mismatch, B < 1 or Lm < 1, or a window outside [0, T). */
int svihmm_suffstats(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                     const double* var_x, double* out_packed);

/* ---- several sequences of unequal length on one handle ----------------------------------------
 * Recordings, trials, chromosomes: the resident rows are N independent chains laid end to end.  The
 * statistics of the whole are the sums over the sequences; no message and no transition pair crosses a join.
 *
 * svihmm_set_sequences declares that: sequence s is rows [seq_off[s], seq_off[s+1]).  seq_off has N + 1
 *   entries, seq_off[0] = 0, strictly increasing, seq_off[N] = T; a length of 1 is allowed.  N = 0 (seq_off may
 *   then be NULL) removes the declaration, and so does every call that replaces the resident rows
 *   (svihmm_set_obs, svihmm_alloc_obs, svihmm_generate).  Fails with a message (the handle stays usable, an
 *   earlier declaration stays in force): no observations, NULL seq_off with N > 0, N < 0, offsets that break
 *   the rules above.
 *   While a declaration is in force every entry point that checks windows against [0, T) (svihmm_loglik,
 *   _forward_backward, _estep_minibatch(_ex), _suffstats, _pred_logprob, _viterbi, _ffbs_windows, the start
 *   windows of _grow_windows, _svi_iteration) also rejects a window that holds rows of two sequences; the
 *   message names the window.  (The candidate windows svihmm_grow_windows evaluates while it grows are checked
 *   like any window batch: growth that would reach across a join fails with that message instead of reading a
 *   neighbour's rows.)  A window inside one sequence gives exactly what it gives without a declaration, and
 *   without a declaration nothing changes.
 *
 * svihmm_estep_sequences: the whole E-step of all N declared sequences under the globals currently set and
 *   the current emission family (NIW, diagonal, Categorical).  For sequence s it computes what
 *   svihmm_forward_backward(h, {seq_off[s]}, 1, len_s, flags, ..) computes: the chain starts from mod_init.
 *   packed (the family's current layout, svihmm_packed_len):
 *     emission statistics over the unmasked rows of all sequences;
 *     A_raw = sum_s sum_{t=1}^{len_s-1} q[t-1] (x) q[t]  (batch form, hmmbatchcd.py:182-184); with
 *       SVIHMM_TRANS_WRAP additionally, per sequence, the pair (last row of s, first row of s) -- the
 *       per-window rule of quirk Q1;
 *     lb = sum_s local_lb[s].
 *   out_seq_lb[N]: local_lb of each sequence (sum_t LSE_k lalpha_t[k], quirk Q4).
 *   out_q0[K] = sum_s var_x[seq_off[s]], added in ascending s (var_init = prior_init + out_q0).
 *   Any of the three pointers may be NULL; the packed result stays in HBM for svihmm_read_packed /
 *   _allreduce_packed / _export_packed.  SVIHMM_MASK_AS_NAN as elsewhere.
 *   Routing: a sequence of at least 2048 rows goes through the whole-chain blocked scan
 *   (svihmm_forward_backward's route for B = 1), one after the other; all shorter ones -- and every sequence
 *   when an ltran entry lies below SVIHMM_LTRAN_LINEAR_MIN, which takes the literal logaddexp form as in
 *   svihmm_forward_backward -- run in ONE launch of the ragged log-domain sweeps, one (sequence, direction)
 *   pair per wavefront (K <= 64) or workgroup, longest first.  The statistics are one pass over all T rows.
 *   A run is bit-reproducible, and the posterior rows and local_lb of a sequence do not depend on which other
 *   sequences are declared or in what order (given the same resident rows).
 *   Always fp64: the precision mode and what svihmm_get_precision reports are unchanged.  K <= 256.
 *   Fails with a message before any device work (the handle stays usable): no declaration, no globals, no
 *   emission family or no observations; a K mismatch between globals and emission family; K > 256;
 *   SVIHMM_USE_HOST_LLIKS; T beyond the statistics GEMM's 32-bit row offsets.
 *   Towards a running resident SVI loop it behaves as svihmm_suffstats does.
 *   Intermediates afterwards: var_x of all T rows is readable as one [1, T, K] batch
 *   (svihmm_read_intermediate / _read_rows, what = 3) and svihmm_state_argmax decodes all T rows; what = 0, 1, 2
 *   fail with "... svihmm_estep_sequences keeps var_x only".
 * The E-step of a chosen subset of the declared sequences: svihmm_estep_sequence_subset below.
 * Decoding all declared sequences in one call: svihmm_viterbi_sequences / svihmm_ffbs_sequences below.
 * The resident SVI loop on minibatches of whole sequences: svihmm_svi_sequences / svihmm_svi_iteration_sequences
 *   (with the svihmm_svi_* family below).
 * Not covered: hmmsgd_metaobs.VBHMM on a list (its batch factors, quirk Q3, have no agreed multi-sequence
 *   form; the boundary check above lets a caller sample windows safely), the fp32 mode, host lliks in
 *   svihmm_estep_sequences, K > 256; in the resident loop on sequences additionally AdaGrad and a communicator
 *   (multi-GPU minibatches of sequences). */
int svihmm_set_sequences(svihmm_ctx* h, const int64_t* seq_off, int32_t N);
int svihmm_estep_sequences(svihmm_ctx* h, uint32_t flags, double* out_packed, double* out_seq_lb,
                           double* out_q0);

/* svihmm_estep_sequence_subset: the E-step of a minibatch of WHOLE sequences -- what svihmm_estep_sequences defines,
 *   restricted to the M listed ones, under the globals currently set and the current emission family (NIW, diagonal,
 *   Categorical).  Stochastic variational inference over sequences draws M of the N, scales these statistics by N / M
 *   and takes a Robbins-Monro step.
 *   idx[M]: declared sequences, each entry in [0, N), M >= 1, in any order.  Duplicates are allowed and every
 *   occurrence counts once (sampling with replacement).
 *   For occurrence m it computes what svihmm_forward_backward(h, {seq_off[idx[m]]}, 1, len, flags, ..) computes.
 *   packed (the family's current layout): emission statistics over the unmasked rows of all occurrences; A_raw in the
 *   batch form summed over the occurrences, with SVIHMM_TRANS_WRAP additionally each occurrence's own (last row,
 *   first row) pair; lb = sum_m local_lb.
 *   out_seq_lb[M]: local_lb of each occurrence, in the order of idx.
 *   out_q0[K]: the sum of the occurrences' first posterior rows, added in ascending m.
 *   Any of the three pointers may be NULL; the packed result stays in HBM for svihmm_read_packed /
 *   _allreduce_packed / _export_packed.  SVIHMM_MASK_AS_NAN as elsewhere.
 *   Reproducibility: with idx = 0, 1, .., N - 1 the packed buffer, out_seq_lb, out_q0 and the posterior rows are
 *   bit-identical to svihmm_estep_sequences on the same handle; the posterior rows and local_lb of a listed sequence
 *   are the same bits as in the full call, whatever else is listed and wherever it stands in idx; two identical
 *   calls are bit-identical.
 *   Cost follows R = sum_m len(idx[m]): the listed rows (and mask bytes) are gathered bit for bit into a compact copy
 *   that belongs to the handle (one launch, 2 R D 8 bytes moved), and emission, sweeps and statistics run on that
 *   copy.  No kernel is launched over T rows and no buffer of T K or T D elements is written.  (Once, where a
 *   Categorical table reads a resident copy that is still centred, the copy is brought back to exact symbol
 *   indices first, as in front of every lookup launch.)
 *   Routing as in svihmm_estep_sequences: listed sequences of at least 2048 rows through the whole-chain scan, one
 *   after the other; all others -- every one when an ltran entry lies below SVIHMM_LTRAN_LINEAR_MIN -- in ONE
 *   ragged launch, longest first.  Always fp64: the precision mode and what svihmm_get_precision reports are
 *   unchanged.  K <= 256.
 *   Afterwards: var_x of the R listed rows is readable as one [1, R, K] batch (what = 3), in the order of idx, and
 *   svihmm_state_argmax decodes those R rows; what = 0, 1, 2 fail with "... svihmm_estep_sequence_subset keeps var_x
 *   of the listed rows only".  The resident rows, the mask, T, the handle's centre and the declaration are exactly
 *   as before -- after a failed call too -- and a following svihmm_estep_sequences returns the bits it returned
 *   before.
 *   Fails with a message before any device work (the handle stays usable): NULL handle; no declaration; idx NULL or
 *   M < 1; an entry outside [0, N) (the message gives its position and value); no globals, no emission family or no
 *   observations; a K mismatch between globals and emission family; K > 256; SVIHMM_USE_HOST_LLIKS; R beyond the
 *   statistics GEMM's 32-bit row offsets.
 *   Towards a running resident SVI loop it behaves as svihmm_suffstats does. */
int svihmm_estep_sequence_subset(svihmm_ctx* h, const int32_t* idx, int32_t M, uint32_t flags,
                                 double* out_packed, double* out_seq_lb, double* out_q0);

/* svihmm_set_labels: partially labelled rows -- the states of some resident rows are known (annotated regions,
 *   behavioural epochs, trials whose condition fixes the state) and every E-step and decoder honours them.
 *   labels: host int32 [T].  labels[t] = -1: row t is free; labels[t] = k >= 0: row t is known to be in state k.
 *   NULL removes the labels.  svihmm_set_obs, svihmm_alloc_obs and svihmm_generate remove them as well (T changes);
 *   svihmm_set_obs_rows and svihmm_set_sequences keep them.
 *   Fails with a message, an earlier set staying in force: no observations; an entry below -1 (the message gives the
 *   row and the value).
 *   The labels live in HBM as int32 [T]; the host keeps the largest label and its first row only.
 *   While labels are in force every call that evaluates lliks on the device sees
 *       ll[t][k] = (labels[t] < 0 || k == labels[t]) ? ll[t][k] : -inf,
 *   a select applied after the family's llik.  SVIHMM_MASK_AS_NAN is applied first, so the kept entry has its original
 *   bits; a masked labelled row means "state known, observation missing": its ll is 0 at the label and -inf elsewhere,
 *   and it stays out of the emission statistics as before.
 *   Such a call is defined to give what the same call gives under SVIHMM_USE_HOST_LLIKS on exactly those clamped
 *   lliks, wherever that call exists: svihmm_loglik, svihmm_read_intermediate / _read_rows with what = 0 and lalpha /
 *   lbeta hand out the -inf values, var_x is 0.0 at forbidden pairs, lb keeps its formula (quirk Q4) on the clamped
 *   lliks.
 *   Honoured by: svihmm_loglik, _forward_backward, _estep_minibatch(_ex), _viterbi, _ffbs_windows, _ffbs,
 *   _estep_sequences, _estep_sequence_subset (the listed sequences' labels are gathered with their rows),
 *   _viterbi_sequences, _ffbs_sequences.
 *   Unaffected: svihmm_suffstats (the caller's posteriors), svihmm_state_argmax, export / import / all-reduce, and
 *   svihmm_heldout_rows / _entries -- their emission term is the family's own llik, unclamped; the posterior rows
 *   they read already carry the labels.  Calls on host lliks (SVIHMM_USE_HOST_LLIKS) take the lliks as uploaded.
 *   Refused with a message before any device work while labels are set (the handle and a running resident loop stay
 *   intact): svihmm_svi_iteration, svihmm_svi_iteration_sequences, svihmm_grow_windows, svihmm_pred_logprob; and an
 *   E-step-type call whose globals have K at or below the largest label (the message gives that label, its row and
 *   K).
 *   A label whose state has probability zero under mod_init, ltran and the row's llik leaves that window's results
 *   unspecified (-inf or NaN, never a fault).
 *   fp32 mode: a labelled batch runs in fp64 and svihmm_get_precision reports last_batch_f32 = 0; the mode itself
 *   is left as set.  With no labels set nothing changes: the same kernels are chosen and the same bits result. */
int svihmm_set_labels(svihmm_ctx* h, const int32_t* labels);

/* svihmm_set_state_sets: allowed-state sets per resident row -- the weaker statement than a label: "this region is one
 *   of these three states", "this epoch is anything but state 0", "these trials never visit states 4-7".
 *   allowed: host uint64 [T][W], W = (K + 63) / 64.  Bit k % 64 of word k / 64 of row t says that state k is allowed
 *   at row t; a row with all K bits set is free.  NULL removes the sets (K is then ignored).  svihmm_set_obs,
 *   svihmm_alloc_obs and svihmm_generate remove them as well; svihmm_set_obs_rows and svihmm_set_sequences keep them.
 *   Sets and labels are alternatives: a successful call with a non-NULL array removes labels, a successful
 *   svihmm_set_labels with a non-NULL array removes sets; NULL to either removes only its own kind.
 *   Fails with a message, whatever was in force staying in force: no observations; K outside [1, 256]; a row that
 *   allows no state; a bit at or beyond K set in a row's last word (the message gives the first offending row, found
 *   in one pass over the array).
 *   The sets live in HBM as uint64 [T][W]; the host keeps K only.
 *   While sets are in force every call that evaluates lliks on the device sees
 *       ll[t][k] = allowed(t, k) ? ll[t][k] : -inf,
 *   a select applied after the family's llik and after SVIHMM_MASK_AS_NAN, so the kept entries have their original
 *   bits; a masked constrained row means "state in this set, observation missing".  As with labels, such a call is
 *   defined to give what the same call gives under SVIHMM_USE_HOST_LLIKS on exactly those clamped lliks, wherever that
 *   call exists; a row whose set holds one state is a labelled row, bit for bit.
 *   Honoured by, unaffected by and refused by the same calls as labels (svihmm_set_labels above); the refusals of
 *   svihmm_svi_iteration, svihmm_svi_iteration_sequences, svihmm_grow_windows and svihmm_pred_logprob name this call,
 *   and an E-step-type call whose globals have a K other than the sets' K fails with a message that gives both.
 *   svihmm_estep_sequence_subset gathers the listed sequences' mask rows with their rows.
 *   A set none of whose states has positive probability under mod_init, ltran and the row's llik leaves that window's
 *   results unspecified (-inf or NaN, never a fault).
 *   fp32 mode: a constrained batch runs in fp64 and svihmm_get_precision reports last_batch_f32 = 0; the mode itself
 *   is left as set.  With neither labels nor sets nothing changes: the same kernels and the same bits. */
int svihmm_set_state_sets(svihmm_ctx* h, const uint64_t* allowed, int32_t K);

/* svihmm_viterbi_sequences: the MAP state path of EVERY declared sequence (svihmm_set_sequences) in one call, under
 *   the globals currently set and the current emission family.
 *   out_z: host int32[T], row r holds the state of resident row r (the sequences laid end to end, as declared);
 *   out_score: host double[N].  Either pointer may be NULL, not both.
 *   Contract: for sequence s the result is what svihmm_viterbi(h, {seq_off[s]}, 1, len_s, flags, ..) defines -- the
 *   recursion and the operation order fixed there (one add per (i, j), a strict `>` scan over ascending i, one add of
 *   ll), delta started from mod_init at the sequence's first row.  Given the lliks the call itself evaluated, z and
 *   score are bit-identical to that recursion in NumPy on each sequence's rows, and a sequence's path and score are
 *   the same bits whatever else is declared and in whatever order (given the same ll rows).
 *   Lliks: ONE emission pass over all T rows (NIW, diagonal, Categorical; SVIHMM_MASK_AS_NAN as elsewhere).
 *   SVIHMM_USE_HOST_LLIKS is accepted when the batch uploaded by svihmm_set_lliks has shape [1][T][K]: its rows are
 *   the concatenated rows.  Always fp64; K <= 256 (one-byte back-pointers).
 *   Routing: a sequence whose back-pointers fit the 64 KiB LDS budget (len <= 1008 at K <= 64, 240 above; every
 *   sequence when out_z is NULL) is decoded inside ONE forward launch, longest first, its LDS sized by the longest
 *   of them; all longer sequences share ONE more forward launch that writes psi to HBM, and are
 *   backtracked together by composing per-chunk state maps as svihmm_viterbi does.  No atomics, no reductions
 *   across sequences.
 *   Fails with a message before any device work (the handle stays usable): NULL handle; both outputs NULL; no
 *   declaration; no globals; no observations or no emission family (unless host lliks); a K mismatch between globals
 *   and emission family; K > 256; host lliks of a shape other than [1][T][K]; T > 2^31 - 1; (number of row
 *   chunks of the long sequences) x (64 or 256) >= 2^31.
 *   Intermediates afterwards: the lliks of all T rows are readable as one [1, T, K] batch (svihmm_read_intermediate /
 *   _read_rows, what = 0); what = 1, 2, 3 fail with a message that names this call.  The packed statistics held in
 *   HBM and what svihmm_get_precision reports are untouched.
 *
 * svihmm_ffbs_sequences: S forward-filter backward-sample paths of EVERY declared sequence from ONE forward filter.
 *   out_z: host int32[S][T] (draw-major, resident rows inside a draw); out_lalpha: host double[T][K] or NULL.
 *   Forward filter: runs once; for sequence s it is the filter of svihmm_ffbs_windows on the window {seq_off[s]},
 *   Lm = len_s: log domain, started from mod_init.  Routing mirrors svihmm_estep_sequences: sequences below 2048
 *   rows -- and every sequence when an ltran entry lies below SVIHMM_LTRAN_LINEAR_MIN, or with host lliks -- in ONE
 *   launch of the ragged log-domain forward sweep; longer ones one after the other through the whole-chain blocked
 *   scan with the log-domain repair of svihmm_ffbs.  NIW, diagonal and Categorical families, SVIHMM_MASK_AS_NAN;
 *   SVIHMM_USE_HOST_LLIKS with an uploaded batch of shape [1][T][K].  Always fp64; K <= 256.
 *   Draws: for every draw s < S and sequence q with last row e
 *       z[s][e] ~ softmax_k( lalpha[e][k] ),    z[s][r] ~ softmax_k( lalpha[r][k] + logA[k][ z[s][r+1] ] )
 *   Draw rule (part of the contract): lp_k the sum above, m = max_k lp_k, p_k = exp(lp_k - m), c_k the running sum
 *   of p in ascending state order, tot = c_{K-1}; the draw is the smallest k with u * tot <= c_k, K - 1 if there is
 *   none.  Where u * tot lies within rounding of some c_k either neighbouring state may be returned (the caveat
 *   of svihmm_ffbs).  A (sequence, draw) pair gives the same path whatever S, N, the other sequences and their
 *   order are.
 *   Uniform source: the uniform of (draw s, resident row r) is entry g = s*T + r.  `uniforms` non-NULL is host
 *   double[S][T].  uniforms == NULL: u is generated on the device, nothing is uploaded: Philox4x32-10 with key
 *   `seed`, counter row g, stream 0, the first two words through the 53-bit mapping svihmm_generate uses for its
 *   transition uniform.
 *   logA: host double[K][K], used as logA[k][z_next] like svihmm_ffbs (need not be the filter's ltran).  -inf entries
 *   mean probability zero; +inf, NaN or a column without a finite entry fail.
 *   Sequences below 2048 rows are sampled in one launch, one lane per (sequence, draw) pair, pairs ordered longest
 *   sequence first; longer ones compose per-chunk state maps once per (sequence, draw) as svihmm_ffbs does.  No device
 *   buffer scales with S*T*K: lalpha is held once, only z and the caller's uniforms scale with S*T.
 *   Fails with a message before any device work (the handle stays usable): NULL handle; NULL logA or out_z; S < 1;
 *   S*N >= 2^31; a bad logA; and the cases of svihmm_viterbi_sequences (no declaration, no globals, no observations
 *   or emission family unless host lliks, K mismatch, K > 256, host lliks of another shape, T > 2^31 - 1).
 *   Intermediates afterwards: the lliks of all T rows are readable (what = 0); lalpha is handed out through
 *   out_lalpha only: what = 1, 2, 3 fail with a message that names this call.  The packed statistics held in HBM
 *   and what svihmm_get_precision reports are untouched. */
int svihmm_viterbi_sequences(svihmm_ctx* h, uint32_t flags, int32_t* out_z, double* out_score);
int svihmm_ffbs_sequences(svihmm_ctx* h, uint32_t flags, const double* logA, int32_t S, const double* uniforms,
                          uint64_t seed, int32_t* out_z, double* out_lalpha);

/* ---- the SVI loop with the variational state resident in HBM ----------------------------------
 * hmmsgd_metaobs.VBHMM.infer (:347-445) iterates  { stationary init :413-418, psi-expectations
 * :502-504, E-step over the minibatch :405-436, global natural-gradient step :1010-1069
 * (util.py:28-60), elbo_vec[it] = lb + global_lower_bound() :444-445, :273-296 }.  With these
 * entry points var_tran and the K NIW factors stay on the device between iterations: per
 * iteration the host sends the window starts and three scalars, and nothing has to come back
 * until the caller wants the ELBO trace or the parameters.  Calls are asynchronous (they return
 * when the work is enqueued); svihmm_svi_read_elbo / svihmm_svi_read_state synchronise.
 *
 * svihmm_svi_begin: uploads the state.  prior_tran / var_tran [K,K]; NIW prior (mu0 [K,D],
 *   sigma0 [K,D,D], kappa0 [K], nu0 [K]) and current factors (mu, sigma, kappa, nu);
 *   prior_logpart[k] = invwishart_log_partitionfunction(sigma0[k], nu0[k]) (constant of the
 *   factors' ELBO term, computed once by the host); zsign = +1 / -1: the sign with which that
 *   constant enters get_vlb (pybasicbayes / Bishop 10.74, see distributions.Gaussian.get_vlb).
 *   The observations must be resident (svihmm_set_obs / svihmm_generate).  Fails when an entry
 *   of prior_tran is below 1 or one of var_tran below SVIHMM_SVI_MIN_PSEUDOCOUNT: with
 *   prior_tran >= 1 no entry of var_tran falls below min(var_tran, 1) during the loop (the step adds
 *   rho bA nwin (prior_tran - 1) with bA nwin ~ T / 2L, quirk Q2 -- negative and large for sparser
 *   priors), so psi(var_tran) stays inside the range of the linear-domain recursions; other
 *   Dirichlet models take the per-call route (svihmm_set_globals decides per upload).
 * svihmm_svi_iteration(it, ...): one iteration on windows starts[B] of length Lm (statistics over
 *   the inner segment, as svihmm_estep_minibatch_ex; flags: SVIHMM_TRANS_WRAP | ...).
 *   nwin_total = windows of the whole minibatch (= B on one GPU; with a communicator the ranks
 *   hold shards and the packed statistics are all-reduced before the step): quirk Q2 adds
 *   nwin_total * (prior_tran - 1).  rho = (it + tau)^-kappa; bfactA = (T-2L-1)/(2L*S),
 *   bfactE = (T-2L-1)/((2L+1)*S) from the CONSTRUCTOR's L, S (quirk Q3).
 * svihmm_svi_read_elbo: elbo_vec[0..n) and the device time of each iteration in ms (device clock:
 *   from the iteration's first kernel -- or the end of the previous iteration when the loop runs back
 *   to back -- to the last workgroup of its theta builder; either may be NULL).  The loop orders its
 *   streams with device-side counters; a dependency that is not met within a minute (a kernel of
 *   the loop never ran) makes this call fail and ends the loop.  svihmm_svi_read_state: current var_tran [K,K], var_init [K] (the stationary vector
 *   of the last iteration, quirk Q5; after svihmm_svi_sequences the LEARNED initial-state factor), NIW factors; any
 *   pointer may be NULL. */
int svihmm_svi_begin(svihmm_ctx* h, int32_t K, int32_t D, const double* prior_tran,
                     const double* var_tran, const double* mu0, const double* sigma0,
                     const double* kappa0, const double* nu0, const double* prior_logpart,
                     const double* mu, const double* sigma, const double* kappa, const double* nu,
                     int32_t maxit, double zsign);
int svihmm_svi_iteration(svihmm_ctx* h, int32_t it, const int64_t* starts, int32_t B,
                         int32_t nwin_total, int32_t Lm, int32_t inner_off, int32_t inner_len,
                         uint32_t flags, double rho, double bfactA, double bfactE);
/* The same loop for the two families whose factors are element-wise (round 4):
 * svihmm_svi_begin_diag: distributions.DiagonalGaussian (per dimension a normal-inverse-gamma factor;
 *   prior_blk / factor_blk = [mu | nus | alphas | betas], each [K][D], means in the caller's
 *   coordinates): the Gaussian branch's blend hmmsgd_metaobs.py:1050-1069 in this family's natural
 *   parameters [nu mu, nu, 2 beta + nu mu^2, 2 alpha], theta by the device builder, ELBO term
 *   -KL(q || prior).  (The reference dispatches on Gaussian / Categorical only: an extension.)
 * svihmm_svi_begin_cat: Categorical emitters over ONE integer-valued observation column (D = 1),
 *   Dirichlet factors alpha[K][V] and prior alpha0[K][V]: global step hmmsgd_metaobs.py:1071-1084 with
 *   every window's alpha_0 + counts - 1 (:907-926), the E log theta table rebuilt on the device.
 * svihmm_svi_iteration / svihmm_svi_read_elbo / svihmm_svi_set_adagrad work for every family;
 * svihmm_svi_read_factors hands back the state in the family's block layout (NIW: [mu | sigma |
 * kappa | nu]; any of the three pointers may be NULL). */
int svihmm_svi_begin_diag(svihmm_ctx* h, int32_t K, int32_t D, const double* prior_tran, const double* var_tran,
                          const double* prior_blk, const double* factor_blk, int32_t maxit);
int svihmm_svi_begin_cat(svihmm_ctx* h, int32_t K, int32_t V, const double* prior_tran, const double* var_tran,
                         const double* alpha0, const double* alpha, int32_t maxit);
int svihmm_svi_read_factors(svihmm_ctx* h, double* var_tran, double* var_init, double* factors_out);
/* The same loop for the two table-driven families (declared here, described with svihmm_set_emission_mcat /
 * svihmm_set_emission_poisson below, whose K, D, V, F and C limits, feature offsets and presence rules they share):
 * svihmm_svi_begin_mcat: distributions.ProductCategorical, D Dirichlet factors per state; alpha0 / alpha [K][F],
 *   feature off_d + v.  Per element the Categorical rule of svihmm_svi_begin_cat,
 *     alpha' = ((1 - rho)(alpha - 1) + (rho bE)(nwin (alpha0 - 1) + counts)) + 1
 *   (every window contributes alpha0 + counts - 1 per column, hmmsgd_metaobs.py:907-926, 1071-1084): a D = 1 model
 *   steps like svihmm_svi_begin_cat bit for bit.  ELBO term: the sum over the columns of the Dirichlet term.
 * svihmm_svi_begin_poisson: distributions.ProductPoisson, Gamma factors; prior_blk = [a0 | b0], factor_blk = [a | b],
 *   each [K][D]; logfact[c] = lgamma(c + 1), c = 0..C, as for svihmm_set_emission_poisson.  The Gaussian branch's
 *   blend (hmmsgd_metaobs.py:1050-1069, the prior once) in the Gamma natural parameters (a - 1, -b):
 *     a' = (1 - rho) a + rho (a0 + bE sx[k][d]),   b' = (1 - rho) b + rho (b0 + bE n[k][d]),
 *   positive for every rho in [0, 1].  ELBO term: -sum_d KL(Gamma(a, b) || Gamma(a0, b0)).
 * Both fail with a message before any state is touched -- the handle and a loop begun earlier stay as they were --
 * on: a NULL pointer; K < 1 or K > 256; D outside the family's range or different from the resident observations';
 * a V[d] < 1; F > SVIHMM_MCAT_MAX_F; C outside [0, SVIHMM_POISSON_MAX_COUNT]; a non-finite logfact[c]; a Dirichlet or
 * Gamma parameter that is not > 0.  What svihmm_svi_begin checks of prior_tran / var_tran holds as well.
 * The E log theta table (k_mcat_table), respectively the (E log lambda, E lambda) pairs (k_pois_table), are rebuilt on
 * the device every iteration.  svihmm_svi_iteration, _read_elbo, _set_adagrad, _read_adagrad, svihmm_read_globals,
 * SVIHMM_SVI_KEEP_WINDOW, the inner segment and a communicator's all-reduce work as for the other families;
 * svihmm_svi_read_factors hands back alpha [K][F], respectively [a | b]; svihmm_svi_read_state refuses (NIW layout).
 * A svihmm_set_emission_mcat / _poisson upload of the same family and shape (K and V[], respectively K and D) keeps
 * the loop alive, as svihmm_set_emission_cat does for its family; any other emission upload ends it. */
int svihmm_svi_begin_mcat(svihmm_ctx* h, int32_t K, int32_t D, const int32_t* V /*[D]*/,
                          const double* prior_tran, const double* var_tran,
                          const double* alpha0 /*[K][F]*/, const double* alpha /*[K][F]*/, int32_t maxit);
int svihmm_svi_begin_poisson(svihmm_ctx* h, int32_t K, int32_t D,
                             const double* prior_tran, const double* var_tran,
                             const double* prior_blk /*[a0 | b0], each [K][D]*/,
                             const double* factor_blk /*[a | b]*/,
                             const double* logfact /*[C + 1]*/, int32_t C, int32_t maxit);
/* AdaGrad-scaled transition step (hmmsgd_metaobs.py:179-183 ada_G = ones, :1036-1040
 * ada_G += nats_old^2; adaMatrix = ada_G^.25; nats_new = (1 - 1/adaMatrix) nats_old + A_up/adaMatrix):
 * after svihmm_svi_begin, svihmm_svi_set_adagrad uploads the K x K accumulator (NULL: the plain rho
 * step again); it stays on the device with var_tran, svihmm_svi_read_adagrad hands it back. */
int svihmm_svi_set_adagrad(svihmm_ctx* h, const double* ada_G);
int svihmm_svi_read_adagrad(svihmm_ctx* h, double* ada_G_out);
int svihmm_svi_read_elbo(svihmm_ctx* h, int32_t n, double* out_elbo, double* out_ms);
/* mod_init[K] / ltran[K,K] as the recursions currently hold them (either may be NULL): the last
 * svihmm_set_globals upload, or -- after svihmm_svi_iteration -- the psi-expectations that
 * iteration computed on the device (hmmsgd_metaobs.py:502-504; the reference leaves them on the
 * object as mod_init / mod_tran). */
int svihmm_read_globals(svihmm_ctx* h, double* mod_init_out, double* ltran_out);
int svihmm_svi_read_state(svihmm_ctx* h, double* var_tran, double* var_init, double* mu,
                          double* sigma, double* kappa, double* nu);

/* The resident loop on minibatches of WHOLE declared sequences (hmmbatchsgd.VBHMM(seq_minibatch = M)): after any
 * svihmm_svi_begin* the loop steps on M of the N sequences of svihmm_set_sequences per iteration instead of windows of
 * one chain.  The initial-state factor is a LEARNED Dirichlet (no stationary vector, no quirk Q2 / Q3).
 *
 * svihmm_svi_sequences(prior_init[K], var_init[K]): puts both into the resident state and switches the loop to the
 *   sequence form.  Needs a running loop and a declaration.  Fails with a message before any state is touched on: no
 *   loop; no declaration; a NULL pointer; an entry of prior_init or var_init that is not finite or lies below
 *   SVIHMM_SVI_MIN_PSEUDOCOUNT (every later var_init is a convex combination of var_init and prior_init + bf q0, so
 *   none falls below the smaller of the two -- svihmm_svi_begin's argument for var_tran); an AdaGrad accumulator is
 *   set; a communicator is attached (multi-GPU minibatches of sequences are out of scope).
 *   Afterwards svihmm_svi_iteration fails and names svihmm_svi_iteration_sequences, and svihmm_svi_set_adagrad with an
 *   accumulator fails; without this call svihmm_svi_iteration_sequences fails and names it.  The next
 *   svihmm_svi_begin* starts a window loop again.  From this call on the loop is ordered by its streams and events
 *   (no device-side counters; svihmm_svi_recoveries is not raised).
 * svihmm_svi_iteration_sequences(it, idx[M], flags, rho, bfact): one iteration, asynchronous.  With bf = bfact (N / M):
 *   1. globals: ltran as in the window loop; mod_init[k] = psi(var_init[k] + eps) - psi(sum var_init + eps) from the
 *      resident learned var_init.  svihmm_read_globals afterwards returns these -- the globals the iteration's E-step
 *      ran under (formed from the state BEFORE its step).
 *   2. E-step: exactly what svihmm_estep_sequence_subset(idx, M, flags) defines (routing, presence rules,
 *      SVIHMM_MASK_AS_NAN, SVIHMM_TRANS_WRAP, duplicates once per occurrence), always fp64; nothing is read back.
 *   3. step, every product and sum rounded on its own:
 *        var_init' = (1 - rho) var_init + rho (prior_init + bf q0)
 *        var_tran' = ((1 - rho)(var_tran - 1) + rho ((prior_tran - 1) + bf A_raw)) + 1      (the prior once)
 *        emission factors: the family's blend with bE = bf (NIW, diagonal, Poisson: the window loop's expressions);
 *        Categorical / multi-column Categorical: alpha' = ((1 - rho)(alpha - 1) + rho ((alpha0 - 1) + bf counts)) + 1
 *   4. elbo[it] = bf lb + dirichlet(prior_init, var_init') + sum_i dirichlet_row_i(prior_tran, var_tran')
 *      + sum_k vlb_k(factors'): hmmbase.lower_bound() with _lZ = bf lb on the state after the step.
 *   svihmm_svi_read_elbo, _read_factors, _read_state and svihmm_read_globals work as before; var_init is the learned
 *   factor.  After an iteration var_x of the R listed rows is readable (what = 3) and svihmm_read_packed gives the
 *   statistics the step consumed, as after svihmm_estep_sequence_subset; the declaration, the resident rows, the mask,
 *   T and the centre are untouched.
 *   Fails before any device work on: it outside [0, maxit); idx NULL; M < 1; an entry outside [0, N) (position and
 *   value in the message); SVIHMM_USE_HOST_LLIKS; SVIHMM_SVI_KEEP_WINDOW; rho or bfact not finite; R beyond the
 *   statistics GEMM's row offsets; and what svihmm_estep_sequence_subset refuses about the model (K > 256). */
int svihmm_svi_sequences(svihmm_ctx* h, const double* prior_init /*[K]*/, const double* var_init /*[K]*/);
int svihmm_svi_iteration_sequences(svihmm_ctx* h, int32_t it, const int32_t* idx, int32_t M,
                                   uint32_t flags, double rho, double bfact);

/* Categorical emissions (hmmsgd_metaobs.py:907-926, 1071-1084; pybasicbayes Categorical):
 * obs must be [T][1] holding the symbol index 0..V-1 as a double; logp[k][v] =
 * E_q log theta_k[v] = psi(alpha_mf[k][v]) - psi(sum_v alpha_mf[k][v]) (host, SciPy digamma).
 * Afterwards the E-step entry points use the table instead of the NIW kernel and the packed
 * statistics have the layout [A_raw K*K | counts K*V | lb] (counts[k][v] = sum of var_x[t,k]
 * over unmasked rows with symbol v); svihmm_packed_len gives the current length. */
int svihmm_set_emission_cat(svihmm_ctx* h, int32_t K, int32_t V, const double* logp);
int64_t svihmm_packed_len(svihmm_ctx* h);

/* Multi-column Categorical emissions: D discrete tracks per row, independent given the state,
 *   p(x_t | z_t = k) = prod_d Cat(x_t[d] | theta_{k,d}).
 * V[d] >= 1 is the number of symbols of column d, F = sum_d V[d], off_d the exclusive prefix sum of V;
 * logp[k][off_d + v] = E_q log theta_{k,d}[v] = psi(alpha_{k,d}[v]) - psi(sum_v alpha_{k,d}[v]) (host, SciPy
 * digamma, per column).  obs is [T][D], each entry a symbol index stored as a double and truncated with (int)x
 * as for svihmm_set_emission_cat.
 * Entry (t, d) is PRESENT when it is not NaN and 0 <= (int)x < V[d].  An entry that is not present is skipped:
 * it adds nothing to the row's llik and nothing to the counts; the row's other columns are not affected.
 * lliks: ll[t][k] = s, where s starts at +0.0 and receives one plain add of logp[k][off_d + x_td] per present
 * column in ascending d (all zeros for a row masked under SVIHMM_MASK_AS_NAN): given the same table, bit-identical
 * to that loop in NumPy, and for D = 1 what svihmm_set_emission_cat returns.
 * Packed statistics (svihmm_packed_len): [A_raw K*K | counts K*F | lb], counts[k][off_d + v] = sum of var_x[t][k]
 * over the rows t with mask[t] == 0 (whatever the flags) whose entry d is present with symbol v.  A_raw, lb,
 * SVIHMM_TRANS_WRAP and the inner segment of svihmm_estep_minibatch_ex behave as for the Categorical family, and
 * so does every entry point that dispatches on the emission family: loglik, forward_backward, estep_minibatch(_ex),
 * suffstats, estep_sequences, estep_sequence_subset, viterbi(_sequences), ffbs, ffbs_windows, ffbs_sequences,
 * grow_windows, state_argmax, read_intermediate / read_rows, read_packed, export / import / allreduce_packed,
 * heldout_rows and heldout_entries.
 * The symbol columns stay exact integers in the resident copy: an upload while the family is active is not
 * centred, a copy centred earlier is brought back, a Gaussian family that follows centres again.
 * Fails with a message before any device work (the handle stays usable): NULL V or logp; K < 1 or K > 256;
 * D < 1 or D > SVIHMM_MCAT_MAX_D; a V[d] < 1; F > SVIHMM_MCAT_MAX_F; a non-finite table entry; and, at the first
 * E-step-type call, resident observations whose D differs from the family's.
 * The resident SVI loop takes the family through svihmm_svi_begin_mcat (above); after this call alone
 * svihmm_svi_iteration refuses with a message that says so.
 * Out of scope, each refused with a message: svihmm_pred_logprob (NIW only) and the fp32 mode
 * (svihmm_get_precision reports last_batch_f32 = 0). */
#define SVIHMM_MCAT_MAX_D 128
#define SVIHMM_MCAT_MAX_F 1024
int svihmm_set_emission_mcat(svihmm_ctx* h, int32_t K, int32_t D, const int32_t* V /*[D]*/,
                             const double* logp /*[K][F]*/);

/* Poisson count emissions: D count tracks per row, independent given the state,
 *   p(x_t | z_t = k) = prod_d Poisson(x_t[d] | lambda_{k,d}),  mean-field factors q(lambda_{k,d}) = Gamma(a_{k,d},
 * b_{k,d}) (shape, rate).  The host forms the expectations (SciPy): elog[k][d] = psi(a) - log(b), erate[k][d] = a / b,
 * and the table logfact[c] = lgamma(c + 1) for c = 0..C (scipy.special.gammaln): a table keeps lgamma off the device
 * and makes the lliks reproducible to the bit.  obs is [T][D], each entry a count stored as a double.
 * Entry (t, d) is PRESENT when it is not NaN and x >= 0.0 && x < (double)(C + 1), compared as doubles (+inf, -0.5, -1
 * and C + 1 are absent); its count is c = (int)x (3.7 counts as 3).  An absent entry adds nothing to the row's llik
 * and nothing to the statistics; the row's other columns are not affected.
 * lliks, for row t and state k: s = +0.0, g = +0.0; for the present d in ascending order p = (double)c_d * elog[k][d]
 * (one rounded multiply, never fused with the add), s = s + p, s = s - erate[k][d], g = g + logfact[c_d]; then
 * ll[t][k] = s - g.  Given the same tables this is bit-identical to that loop in NumPy.  A row masked under
 * SVIHMM_MASK_AS_NAN, or one with no present entry, gives +0.0 for every k.
 * Packed statistics (svihmm_packed_len): [A_raw K*K | stat K*2D | lb], stat[k] = [sx[k][0..D) | n[k][0..D)],
 * sx[k][d] = sum var_x[t][k] c_td and n[k][d] = sum var_x[t][k], both over the rows t with mask[t] == 0 (whatever
 * the flags) whose entry d is present: the conjugate update is a = a0 + sx, b = b0 + n.  A_raw, lb,
 * SVIHMM_TRANS_WRAP and the inner segment of svihmm_estep_minibatch_ex behave as for the Categorical families.  The
 * statistics carry no coordinates: export, import and all-reduce pass them through unchanged.
 * Every entry point that dispatches on the emission family takes this one: loglik, forward_backward,
 * estep_minibatch(_ex), suffstats, estep_sequences, estep_sequence_subset, viterbi(_sequences), ffbs, ffbs_windows,
 * ffbs_sequences, grow_windows (both methods), state_argmax, read_intermediate / read_rows, read_packed, export /
 * import / allreduce_packed, heldout_rows and heldout_entries.  Always fp64, K <= 256.
 * The counts stay exact in the resident copy, as for svihmm_set_emission_mcat: an upload while the family is active
 * is not centred, a copy centred earlier is brought back before the first lookup (an entry within 2^-20, relative,
 * of an integer becomes that integer; a fractional entry keeps its value to rounding, so 3.7 still counts as 3 and
 * -0.5 stays absent), a Gaussian family that follows centres again.
 * Fails with a message before any device work, with the handle and the family set before still in force: NULL elog,
 * erate or logfact; K < 1 or K > 256; D < 1 or D > SVIHMM_POISSON_MAX_D; C < 0 or C > SVIHMM_POISSON_MAX_COUNT; a
 * non-finite elog[k][d], erate[k][d] or logfact[c] (the message names the entry); and, at the first E-step-type call,
 * resident observations whose D differs from the family's.
 * The resident SVI loop takes the family through svihmm_svi_begin_poisson (above); after this call alone
 * svihmm_svi_iteration refuses with a message that says so.
 * Out of scope, each refused with a message: svihmm_pred_logprob (NIW only) and the fp32 mode
 * (svihmm_get_precision reports last_batch_f32 = 0). */
#define SVIHMM_POISSON_MAX_D     128
#define SVIHMM_POISSON_MAX_COUNT ((1 << 20) - 1)
int svihmm_set_emission_poisson(svihmm_ctx* h, int32_t K, int32_t D,
                                const double* elog /*[K][D]*/, const double* erate /*[K][D]*/,
                                const double* logfact /*[C + 1]*/, int32_t C);

/* Gaussian tracks with missing entries: D real-valued columns per row, independent given the state,
 *   p(x_t | z_t = k) = prod_{d present} N(x_t[d] | mu_{k,d}, sigma^2_{k,d}),  a normal-inverse-gamma mean-field factor
 * (mu, nus, alphas, betas) per (k, d).  The host forms the three tables (SciPy), each [K][D]: mu,
 * hprec[k][d] = -0.5 alphas / betas and cst[k][d] = -0.5 / nus - 0.5 (log betas - psi(alphas)) - 0.5 log 2 pi, so no
 * digamma and no log of a parameter runs on the device.  obs is [T][D] doubles.
 * Entry (t, d) is PRESENT when x > -SVIHMM_PGAUSS_ABSENT && x < SVIHMM_PGAUSS_ABSENT, compared as doubles: a NaN
 * fails both, +-inf and 1e308-style sentinels are absent.  An absent entry adds nothing to the row's llik and nothing
 * to the statistics; the row's other columns are not affected.  (svihmm_set_emission_diag, in contrast, gives a whole
 * NaN row for one NaN entry.)
 * lliks, for row t and state k: s = +0.0; for the present d in ascending order r = x - mu[k][d], p = r * r,
 * p = p * hprec[k][d], s = s + p, s = s + cst[k][d], every operation rounded on its own (never fused); then
 * ll[t][k] = s.  The centred form evaluated directly: it needs no centred resident copy.  Given the same tables and
 * the same resident values this is bit-identical to that loop in NumPy.  A row masked under SVIHMM_MASK_AS_NAN, or
 * one with no present entry, gives +0.0 for every k.
 * Packed statistics (svihmm_packed_len): [A_raw K*K | stat K*3D | lb], stat[k] = [sxx[k][0..D) | sx[k][0..D) |
 * n[k][0..D)], taken about the caller's origin[D] with r = x - origin[d]: sxx[k][d] = sum var_x[t][k] (r * r),
 * sx[k][d] = sum var_x[t][k] r, n[k][d] = sum var_x[t][k], all over the rows t with mask[t] == 0 (whatever the
 * flags) whose entry d is present.  An origin near the data (a column's mean over its present entries, say) keeps
 * sxx - sx^2 / n from cancelling for data far from zero.  A_raw, lb, SVIHMM_TRANS_WRAP and the inner segment of
 * svihmm_estep_minibatch_ex behave as for the Categorical families.  The statistics carry only the caller's own
 * origin: export, import and all-reduce pass them through unchanged.
 * Every entry point that dispatches on the emission family takes this one: loglik, forward_backward,
 * estep_minibatch(_ex), suffstats, estep_sequences, estep_sequence_subset, viterbi(_sequences), ffbs, ffbs_windows,
 * ffbs_sequences, grow_windows (both methods), state_argmax, read_intermediate / read_rows, read_packed, export /
 * import / allreduce_packed, heldout_rows, heldout_entries.  Always fp64, K <= 256.
 * The resident copy follows the rule of the symbol families: an upload while the family is in force is not centred;
 * a copy an earlier Gaussian family centred is brought back by the plain shift before the first lookup, which
 * restores the values to rounding only, NOT to the bit; a Gaussian family that follows centres again.  The
 * bit-identity above therefore holds for rows uploaded while this family is in force (and for rows never centred);
 * rows that went through a centring and back agree with the loop on the caller's values to rounding.  That rounding is
 * relative to the centre: the Gaussian families centre on the mean of every entry below 1.7e308 in magnitude, so rows
 * that hold 1e200-style sentinels belong uploaded while this family is in force (set the family, then the rows).
 * Fails with a message before any device work, with the handle and the family set before still in force: a NULL mu,
 * hprec, cst or origin; K < 1 or K > 256; D < 1 or D > SVIHMM_PGAUSS_MAX_D; a non-finite mu[k][d], hprec[k][d],
 * cst[k][d] or origin[d]; a positive hprec[k][d]; a |mu[k][d]| or |origin[d]| at or above SVIHMM_PGAUSS_ABSENT (so
 * no square can overflow; the message names the entry); and, at the first E-step-type call, resident observations
 * whose D differs from the family's.
 * Out of scope, each refused with a message: the resident SVI loop (svihmm_svi_begin_* replaces the family;
 * svihmm_svi_iteration after this call alone refuses), svihmm_pred_logprob (NIW only) and the fp32 mode
 * (svihmm_get_precision reports last_batch_f32 = 0). */
#define SVIHMM_PGAUSS_MAX_D  128
#define SVIHMM_PGAUSS_ABSENT 1e150
int svihmm_set_emission_pgauss(svihmm_ctx* h, int32_t K, int32_t D, const double* mu /*[K][D]*/,
                               const double* hprec /*[K][D]*/, const double* cst /*[K][D]*/,
                               const double* origin /*[D]*/);

/* ELBO bookkeeping of the SVI loop (hmmsgd_metaobs.py:273-296 global_lower_bound,
 * hmmbase.py:183-185: sum_k var_emit[k].get_vlb()): the data-dependent scalars of the NIW
 * factors' term for the given mean-field parameters (D <= SVIHMM_NIW_MAX_D; D <= 64 runs the
 * single-wave factorisation, wider factors the workgroup-per-state one the E-step uses there) --
 * out[k] = log det sigma_mf[k], out[K+k] = tr(sigma_mf[k]^-1 sigma_0[k]),
 * out[2K+k] = (mu_mf[k]-mu_0[k])' sigma_mf[k]^-1 (mu_mf[k]-mu_0[k]); the host adds the
 * closed-form parts (digamma / gammaln of nu, kappa).  The prior (mu_0[K,D], sigma_0[K,D,D])
 * is uploaded once with svihmm_set_emission_prior.  A pure function of its arguments: the
 * E-step's own parameter set and the intermediates of the last E-step are not touched. */
int svihmm_set_emission_prior(svihmm_ctx* h, int32_t K, int32_t D, const double* mu0,
                              const double* sigma0);
int svihmm_niw_vlb_terms(svihmm_ctx* h, int32_t K, int32_t D, const double* mu,
                         const double* sigma, const double* kappa, const double* nu,
                         double* out3K);

/* Mean predictive log-probability of the held-out (masked) rows of the given windows
 * (hmmsgd_metaobs.py:1086-1145 pred_logprob / pred_logprob_full, hmmbase.py:322-340):
 * E-step with `flags` (SVIHMM_MASK_AS_NAN: the masked rows are missing), then the mean over
 * the masked rows of LSE_k( log(var_x[t,k] + 1e-9) + E_q log p(x_t | k) ) with the emission
 * term evaluated on the true observations.  out2[0] = mean (NaN if nothing is masked),
 * out2[1] = number of masked rows.  NIW emission only (a host-supplied lliks batch has no
 * "true observation" term). */
int svihmm_pred_logprob(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm,
                        uint32_t flags, double out2[2]);

/* Held-out log-probability against the POSTERIOR BATCH CURRENTLY HELD: the var_x rows svihmm_read_rows(what = 3)
 * would hand out, nrows of them, left by svihmm_forward_backward, svihmm_estep_minibatch(_ex), svihmm_estep_sequences
 * or svihmm_estep_sequence_subset (svihmm_suffstats computes on the caller's posteriors and leaves the batch held as
 * it is).  Neither function runs an E-step of its own, so one E-step can be scored several ways; both are always fp64,
 * take K <= 256 and touch neither the packed statistics, the precision report nor var_x.  Towards a running resident
 * SVI loop they behave as svihmm_suffstats does.  Both results are bit-reproducible run to run (fixed assignment of
 * rows / entries to workgroups, partials added in workgroup order, no atomics).
 *
 * svihmm_heldout_rows (hmmbase.py:322-340), every family: for each batch row g whose resident row has mask != 0,
 *   lp_g = LSE_k( log(var_x[g][k] + 1e-9) + ll_true[g][k] ),
 * ll_true the family's llik of the row's resident values with the masking flag off.  After a window batch the rows
 * are starts[b] + t (a row in two windows counts once per occurrence), after svihmm_estep_sequences all T rows,
 * after svihmm_estep_sequence_subset the R gathered rows with the gathered copy's own values and mask bytes.
 * out2 = {mean, count}, {NaN, 0} when no scored row is masked or the handle has no mask (then nothing is launched);
 * out_lp (host, [nrows], optional): lp_g for the masked rows, NaN elsewhere.  The E-step is expected to have run
 * with SVIHMM_MASK_AS_NAN; the call does not check that.
 *
 * svihmm_heldout_entries, the multi-column Categorical, the Poisson and the Gaussian-tracks family: entry e is (g = row[e], d = col[e],
 * x = val[e]), g a row of the batch held;
 *   lp_e = LSE_k( log(var_x[g][k] + 1e-9) + term_k ),
 *   multi-column Categorical: term_k = logp[k][off_d + (int)x]
 *   Poisson: t = (double)c * elog[k][d] (one rounded multiply, never fused), t = t - erate[k][d], t = t - logfact[c],
 *            c = (int)x.
 *   Gaussian tracks (svihmm_set_emission_pgauss): t = x - mu[k][d], t = t * t, t = t * hprec[k][d],
 *            t = t + cst[k][d], each rounded on its own.
 * An entry whose x is not PRESENT under the family's own rule (above, NaN included) is skipped: out_lp[e] = NaN, not
 * counted.  Duplicates count once each.  out2 = {mean over the counted entries, count}, {NaN, 0} when n = 0 (no
 * launch) or nothing is counted.  The resident value at (g, d) is not looked at: blanking it before the E-step is the
 * caller's job.
 *
 * Both fail with a message before any device work, the handle staying usable: NULL handle or out2; n < 0; NULL
 * arrays with n > 0; a row[e] outside [0, nrows) or a col[e] outside [0, D) (the message gives e and the value); no
 * posterior batch held -- no E-step-type call yet, or svihmm_loglik, svihmm_pred_logprob, a decoder or
 * svihmm_grow_windows ran since, or new rows were uploaded (the message names the calls that leave one); K > 256 or
 * a K of the globals that is not the batch's; _entries: another family than the three above; _rows: no
 * emission family, a family other than the batch's, or a batch of host lliks (no "true observation"). */
int svihmm_heldout_rows(svihmm_ctx* h, double out2[2], double* out_lp /*[nrows] or NULL*/);
int svihmm_heldout_entries(svihmm_ctx* h, int64_t n, const int64_t* row /*[n]*/, const int32_t* col /*[n]*/,
                           const double* val /*[n]*/, double out2[2], double* out_lp /*[n] or NULL*/);

/* Posterior expectations of a per-state table against the POSTERIOR BATCH CURRENTLY HELD, under the contract of the
 * two held-out calls above: the nrows = lastB * lastLm rows svihmm_read_rows(what = 3) hands out (window-major after a
 * window batch, a row in two windows once per window; all T rows after svihmm_estep_sequences; the R gathered rows
 * after svihmm_estep_sequence_subset), no E-step, always fp64, K <= 256; the packed statistics, the precision report,
 * var_x and the batch itself stay as they are (a held-out call afterwards finds the batch).  Towards a running
 * resident SVI loop they behave as svihmm_suffstats does.  They do not depend on the emission family: `table`
 * (host, [K][F] row-major, 1 <= F <= SVIHMM_MCAT_MAX_F) is whatever the caller wants averaged -- state means for the
 * smoothed signal and for imputation, rates, predictive symbol probabilities --, no family need be set, a batch that
 * ran on host lliks (SVIHMM_USE_HOST_LLIKS) is taken and the resident observations are not read.  A batch computed in
 * the fp32 mode is taken as well: its var_x is handed out as fp64 rows.
 *
 * svihmm_posterior_expect: out[g][f] = sum_k var_x[g][k] table[k][f] for every batch row g (host, [nrows][F]), an fp64
 *   MFMA GEMM.  The order in which the K products of an output are added is fixed by the kernel and is the same for
 *   every row and grid: two calls give the same bits, and so does the same var_x row met in two batches.  Within
 *   K 2^-52 sum_k |var_x[g][k] table[k][f]| of the exact sum.
 * svihmm_posterior_expect_entries: out[e] = sum_k var_x[row[e]][k] table[k][col[e]] (host, [n]) for a sparse list,
 *   k ascending from s = 0.0, p = var_x * table rounded, s = s + p rounded (never fused): a host loop restates it bit
 *   for bit.  Duplicates are allowed; n = 0 launches nothing.
 *
 * Both fail with a message before any device work, the handle staying usable: NULL handle, table or out; F outside
 * [1, SVIHMM_MCAT_MAX_F]; n < 0; NULL row / col with n > 0; a row[e] outside [0, nrows) or a col[e] outside [0, F)
 * (the message gives e and the value); a non-finite table entry (the message gives k and f); no posterior batch held
 * (as the held-out calls say it); K > 256 or a K of the globals that is not the batch's. */
int svihmm_posterior_expect(svihmm_ctx* h, int32_t F, const double* table /*[K][F]*/, double* out /*[nrows][F]*/);
int svihmm_posterior_expect_entries(svihmm_ctx* h, int32_t F, const double* table /*[K][F]*/, int64_t n,
                                    const int64_t* row /*[n]*/, const int32_t* col /*[n]*/, double* out /*[n]*/);

/* State decoding of the last estep/forward_backward call for the evaluation metrics
 * (hmmbase.py:346-355 hamming_dist; util.py:236-277 munkres_match's count matrix):
 * z[r] = argmax_k var_x[r, k] for the n = B*Lm rows (window-major; the first maximum wins like
 * np.argmax) and, when true_sts (host, int32[n], same row order) is given,
 * conf[pred*K + true] = number of rows decoded as `pred` whose label is `true` (labels outside
 * [0, K) are skipped).  out_z (host int32[n]) and out_conf (host int64[K*K]) are optional. */
int svihmm_state_argmax(svihmm_ctx* h, const int32_t* true_sts, int32_t* out_z,
                        int64_t* out_conf);

/* Viterbi / MAP state paths: the most probable state SEQUENCE of every window (svihmm_state_argmax
 * decodes the marginals row by row -- right for the Hamming metric, hmmbase.py:346-355, but its rows can
 * be joined by transitions of (near-)zero probability).  For each window b of Lm rows starting at
 * starts[b], with the globals currently set (mod_init, ltran) and the current emission family:
 *     delta[0][j] = mod_init[j] + ll[0][j]
 *     delta[t][j] = max_i (delta[t-1][i] + ltran[i][j]) + ll[t][j]       psi[t][j] = the first maximising i
 *     z[Lm-1] = first argmax_j delta[Lm-1][j];  z[t-1] = psi[t][z[t]];   score[b] = max_j delta[Lm-1][j]
 * ll is exactly what svihmm_loglik returns for the windows with the same flags: NIW, diagonal and
 * Categorical families, svihmm_set_lliks data with SVIHMM_USE_HOST_LLIKS (starts is then not used and may
 * be NULL), SVIHMM_MASK_AS_NAN gives masked rows ll = 0.
 * Operation order (part of the contract): ONE add per (i, j); a max over i in ascending order in which only
 * a strictly larger value replaces the incumbent, so the lowest index wins ties like np.argmax and an
 * all -inf column decodes to predecessor 0; then ONE add of ll[t][j].  There is no multiplication, hence no
 * fused multiply-add: given identical ll, delta, score and the path are bit-identical to the same three
 * steps in NumPy ((delta[:, None] + ltran) -> argmax / max over axis 0 -> + ll[t]).
 * The recursion lives in the log domain and has none of the dynamic-range limits of the scaled sweeps:
 * ltran entries below SVIHMM_LTRAN_LINEAR_MIN, or -inf, take the same kernels.  Always fp64 (the precision
 * mode and what svihmm_get_precision reports are unchanged).  K <= 256 (one-byte back-pointers).
 * out_z: host int32[B*Lm], window-major like svihmm_state_argmax; out_score: host double[B]; either may be
 * NULL (not both).  Windows whose back-pointers fit in LDS are decoded in one launch; longer ones -- the
 * whole chain B = 1, Lm = T included -- keep psi in HBM and backtrack without a sequential pass, by
 * composing per-chunk state maps as svihmm_ffbs does.  The forward pass over one window is sequential.
 * Fails with a message, before any device work, without globals, without an emission family or
 * observations (unless host lliks), on a K mismatch between globals and emission family, B < 1 or
 * Lm < 1, a window outside [0, T), K > 256, or host lliks of another shape.
 * Intermediates: like svihmm_loglik the call writes the handle's lliks buffer -- afterwards the lliks of
 * THESE windows are readable (svihmm_read_intermediate / _read_rows, what = 0) and lalpha / lbeta / var_x of
 * an earlier E-step are not; the packed statistics held in HBM (svihmm_read_packed / _allreduce_packed /
 * _export_packed) are not touched. */
int svihmm_viterbi(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                   int32_t* out_z, double* out_score);

/* Forward-filter backward-sample for window batches, many draws from ONE forward filter (hmm_fast.pyx:43-124;
 * its lalpha_init branch, :80-95, exists so that a filter can serve repeated draws): S state paths of every
 * window b of Lm rows starting at starts[b].
 * Forward filter: runs once, in the log domain, with the globals currently set (mod_init, ltran) and the current
 *   emission family; lalpha[b] is what svihmm_forward_backward returns for these windows and `flags` (the same
 *   kernels: the per-window log-domain recursion, for B = 1 and Lm >= 2048 the blocked scan with the log-domain
 *   repair of svihmm_ffbs).  NIW, diagonal and Categorical families, svihmm_set_lliks data with
 *   SVIHMM_USE_HOST_LLIKS (starts is then not used and may be NULL), SVIHMM_MASK_AS_NAN gives masked rows ll = 0.
 *   Always fp64: the precision mode and what svihmm_get_precision reports are unchanged.
 * Draws: for every draw s < S and window b
 *     z[s][b][Lm-1] ~ softmax_k( lalpha[b][Lm-1][k] )
 *     z[s][b][t]    ~ softmax_k( lalpha[b][t][k] + logA[k][ z[s][b][t+1] ] )
 * Draw rule (part of the contract): lp_k the sum above, m = max_k lp_k, p_k = exp(lp_k - m), c_k the running sum
 *   of p in ascending state order, tot = c_{K-1}; the draw is the smallest k with u * tot <= c_k, K - 1 if there is
 *   none.  Where u * tot lies within rounding of some c_k either neighbouring state may be returned (the caveat
 *   of svihmm_ffbs).  A (window, draw) pair gives the same path whatever S, B or the other windows are.
 * Uniform source: `uniforms` non-NULL is host double[S][B][Lm], u of (s, b, t) is entry g = (s*B + b)*Lm + t.
 *   uniforms == NULL: u is generated on the device, nothing is uploaded: Philox4x32-10 with key `seed`, counter
 *   row g, stream 0, the first two words through the 53-bit mapping svihmm_generate uses for its transition
 *   uniform.
 * logA: host double[K][K], used as logA[k][z_next] like svihmm_ffbs (need not be the filter's ltran).  -inf entries
 *   mean probability zero; +inf, NaN or a column without a finite entry fail.
 * out_z: host int32[S][B][Lm], window-major inside a draw like svihmm_viterbi; out_lalpha: host double[B][Lm][K]
 *   or NULL.
 * Fails with a message, before any device work: NULL logA or out_z; S < 1, B < 1 or Lm < 1 (or S*B >= 2^31); a
 *   window outside [0, T); no globals, no emission family or no observations (unless host lliks), host lliks of
 *   another shape; a K mismatch between globals and emission family; K > 256; a bad logA.  The handle stays
 *   usable after a failed call.
 * Windows below 2048 rows are sampled in one launch, one lane per (window, draw); longer ones -- the whole chain
 *   B = 1, Lm = T included -- compose per-chunk state maps once per (window, draw) as svihmm_ffbs does (for
 *   B = 1, S = 1, Lm = T the path is svihmm_ffbs's).  No device buffer scales with S*Lm*K: lalpha is held once,
 *   only z and the caller's uniforms scale with S*B*Lm.
 * Intermediates: the call writes the handle's lliks / lalpha buffers -- afterwards lliks and lalpha of THESE
 *   windows are readable (svihmm_read_intermediate / _read_rows), lbeta / var_x of an earlier E-step are not; the
 *   packed statistics held in HBM (svihmm_read_packed / _allreduce_packed / _export_packed) are not touched. */
int svihmm_ffbs_windows(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                        const double* logA, int32_t S, const double* uniforms, uint64_t seed,
                        int32_t* out_z, double* out_lalpha);

/* Adaptive window length and buffer growth on the device (hmmsgd_metaobs.py:521-569 select_L, :579-661
 * select_buffer "GrowBuf"): for each of n centres the half-width at which the posterior of its probe rows stops moving.
 * T = the resident rows; ll = what svihmm_loglik returns for them with `flags` (NIW, diagonal and Categorical
 * families, SVIHMM_MASK_AS_NAN); q_b = the posterior of the window [c - b, c + b] under the globals currently set,
 * started from mod_init at row c - b (get_local_messages, :663-700); the probes are its rows c - m and c + m,
 * m = probe_off.  select_L is half0 = minHalfL, m = 0; select_buffer is half0 = m = halfL.
 * Growth rule, per centre and independent of all other centres (eps = epsilon, inc = increment):
 *     b = half0; q_old = probes(b); d_l = d_r = DBL_MAX; count = 0; run = old = (0, 0)
 *     loop: if c - b < 1 + inc or c + b + inc + 1 > T or b > cutoff: stop
 *           rule 0: if d_l < eps and d_r < eps: stop
 *           rule 1: count += 1; if count > 1 and (run_l - old_l)/(count - 1) < eps and (run_r - old_r)/(count - 1) < eps: stop
 *           b += inc; q_new = probes(b); d_x = sum_k |q_new_x[k] - q_old_x[k]|; old = run; run += d; q_old = q_new
 * out_half[i] = the final b; out_steps[i] (may be NULL) = growth steps taken; out_trace (may be NULL):
 *   out_trace[(i*trace_cap + s)*2 + {0, 1}] = (d_l, d_r) of step s, NaN past a centre's steps; steps beyond trace_cap
 *   are counted, not stored; for m = 0 both entries are equal.
 * method:
 *   SVIHMM_GROW_PRODUCTS  one emission pass over the rows every centre can reach (n windows of ONE common length
 *       W = min(2 R + 1, T), R = the largest half-width the sequence ends and the cutoff let any centre reach,
 *       window i starting at clamp(c_i - R, 0, T - W)), then one launch, one workgroup per centre: the candidates are
 *       nested, so with G_t = A diag(e_t), A = exp(ltran), e_t = exp(ll_t - max_k ll_t) the probe marginals are
 *       q_left ~ (v' F_b) (.) (Mid R_b 1), q_right ~ (v' F_b Mid) (.) (R_b 1), v = exp(mod_init + ll_{c-b}), where
 *       F_b = G_{c-b+1} .. G_{c-m} grows on the left, R_b = G_{c+m+1} .. G_{c+b} on the right and
 *       Mid = G_{c-m+1} .. G_{c+m} is built once: two K x K x K products per added row (v_mfma_f64_16x16x4_f64)
 *       instead of a whole forward / backward pass per candidate.  Matrices are rescaled by exact powers of two.
 *       Needs K <= 64 and every ltran entry >= SVIHMM_LTRAN_LINEAR_MIN; fails with a message otherwise.  A centre's
 *       result is bit-identical whatever n and the other centres are.
 *   SVIHMM_GROW_LITERAL   the rule as written: per candidate the E-step of svihmm_forward_backward on the windows of
 *       the centres still growing; the probe rows, residuals and the rule's state stay on the device, per candidate
 *       only the n "grows again" flags come back.  Any K svihmm_forward_backward serves, any ltran.
 *   SVIHMM_GROW_AUTO      PRODUCTS where it applies, LITERAL otherwise.
 * Always fp64: the precision mode and what svihmm_get_precision reports are unchanged.
 * Fails with a message, before any device work (the handle stays usable): NULL centers or out_half; n < 1,
 *   increment < 1, half0 < 0, probe_off < 0 or probe_off > half0; rule not 0 or 1; epsilon not finite; trace_cap < 0;
 *   an unknown method; a start window [c - half0, c + half0] outside [0, T); no observations, no globals or no
 *   emission family; a K mismatch between globals and emission family; SVIHMM_USE_HOST_LLIKS (host lliks have no row
 *   axis to grow along); method PRODUCTS where the kernel does not apply.
 * Intermediates: like svihmm_loglik the call writes the handle's lliks buffer -- afterwards the lliks of the LAST
 *   window batch it evaluated are readable (svihmm_read_intermediate / _read_rows, what = 0): the n reach windows of
 *   length W (PRODUCTS), the last candidate's windows of the centres that grew longest (LITERAL); lalpha / lbeta /
 *   var_x of an earlier E-step are not.  The packed statistics held in HBM are not touched. */
#define SVIHMM_GROW_AUTO     0
#define SVIHMM_GROW_LITERAL  1   /* one log-domain forward/backward per candidate, by the library */
#define SVIHMM_GROW_PRODUCTS 2   /* the matrix-product kernel; fails where it does not apply */
int svihmm_grow_windows(svihmm_ctx* h, const int64_t* centers, int32_t n,
                        int32_t half0, int32_t probe_off, int32_t increment, int32_t cutoff,
                        double epsilon, int32_t rule, uint32_t flags, int32_t method,
                        int32_t* out_half, int32_t* out_steps,
                        double* out_trace, int32_t trace_cap);

/* Readback of the intermediates of the last estep/forward_backward call
 * (what 0: lliks, 1: lalpha, 2: lbeta, 3: var_x; each [B,Lm,K]).
 * Large batches (B >= 192, K <= 64) run scaled linear-domain sweeps that never write a
 * logarithm: var_x is formed on first read, and the log-domain lliks / lalpha / lbeta of the
 * requested windows are recomputed by the log-domain kernels (exact, same values as a
 * svihmm_forward_backward call on those windows).  That recomputation uses the CURRENT
 * observations / globals / emission parameters: read log-domain intermediates before the
 * next svihmm_set_* call (a read after one fails with an explicit error; ranges already
 * rebuilt stay readable). */
int svihmm_read_intermediate(svihmm_ctx* h, int32_t what, double* out);
/* nrows rows starting at flattened row row0 of the same [B*Lm, K] arrays. */
int svihmm_read_rows(svihmm_ctx* h, int32_t what, int64_t row0, int64_t nrows,
                     double* out);

/* ---- synthetic sequences generated in HBM (gen_synthetic.py:27-44 generate_data) ---------- */
/* Start in state 0; z_t drawn from row z_{t-1} of the transition matrix by np.random.choice's
 * inverse CDF (cdf[K,K] = cumsum(tran, axis=1) / cumsum[:, -1], searchsorted side='right');
 * x_t = means[z_t] + chols[z_t] n_t with n_t ~ N(0, I) (chols: lower Cholesky factors [K,D,D]).
 * Counter-based randomness (Philox4x32-10 keyed by `seed`; row t: stream 0 = transition uniform,
 * stream 1 + p = Box-Muller pair for components 2p, 2p+1), so a run is reproducible and the
 * state chain needs no sequential pass (composition of per-row maps).  The sequence becomes
 * the resident observation copy (no mask); K <= 64.  svihmm_read_generated copies the states
 * (int32[T]) and / or the observations ([T,D]) to the host. */
int svihmm_generate(svihmm_ctx* h, int64_t T, int32_t K, int32_t D, const double* cdf,
                    const double* means, const double* chols, uint64_t seed);
int svihmm_read_generated(svihmm_ctx* h, int32_t* sts_out, double* obs_out);

/* ---- a12: forward-filter backward-sample (hmm_fast.pyx:43-124) ---------------- */
/* Forward filter over the whole chain with the globals currently set (the host
 * passes the Cython variant's mod_init/ltran), then z[T-1] ~ softmax(lalpha[T-1]),
 * z[t] ~ softmax_k(lalpha[t,k] + log_tran_col[k, z[t+1]]) by inverse CDF
 * (rand_discrete, hmm_fast.pyx:29-36) with uniforms[t] in [0,1) supplied by the
 * caller (libc rand() streams are not reproducible on a device).
 * logA[K,K] = log(var_tran + DBL_EPSILON).  out_z[T] int64, out_lalpha[T,K] or NULL.
 * Long chains (K <= 64, T >= 2048) take no sequential pass over T: the forward filter runs as
 * the blocked scan of the full-chain E-step, the draws z[t] = F_t(z[t+1]) are composed as maps
 * over row chunks (same path as the sequential sampler unless a uniform lies within rounding of
 * a CDF step); out_lalpha is exact also for entries the scaled scan loses to underflow. */
int svihmm_ffbs(svihmm_ctx* h, const double* logA, const double* uniforms,
                uint32_t flags, int64_t* out_z, double* out_lalpha);

/* Backward sampling only, from forward messages the caller supplies: the `lalpha_init` branch of
 * FFBS (hmm_fast.pyx:80-95 skips the likelihoods and the filter, :97-122 samples).  lalpha[T,K]
 * host; logA / uniforms / out_z as svihmm_ffbs.  The resident observations are not used. */
int svihmm_ffbs_sample(svihmm_ctx* h, int64_t T, int32_t K, const double* lalpha,
                       const double* logA, const double* uniforms, int64_t* out_z);

/* ---- multi-GPU: one process per GPU, RCCL over xGMI ----------------------------- */
/* uid is a 128-byte ncclUniqueId produced on rank 0 and distributed by the host. */
int svihmm_comm_unique_id(char uid_out[128]);
int svihmm_comm_init(svihmm_ctx* h, const char uid[128], int32_t rank,
                     int32_t nranks);
int svihmm_comm_destroy(svihmm_ctx* h);
/* ncclCommCount of the handle's communicator (0 when none): the number of ranks RCCL itself
 * sees, reported by bench.py so that an N-GPU line can be told from N independent replicas. */
int svihmm_comm_count(svihmm_ctx* h, int32_t* nranks_out);
/* In-place ncclAllReduce(sum, double) of the packed statistics in HBM: the
 * "A_inter += A_i ; emit_inter[k] += e_i[k]" accumulation of
 * hmmsgd_metaobs.py:430-436 extended across ranks. */
int svihmm_allreduce_packed(svihmm_ctx* h);
/* The same exchange with the sum formed by the HOST (a communicator other than RCCL -- MPI, gloo --
 * or two handles on one device): svihmm_export_packed hands out exactly what the all-reduce puts on
 * the wire -- this rank's statistics in the callers' common coordinates (every rank's resident copy
 * has its own centre) -- and svihmm_import_packed takes the reduced vector back into the handle, from
 * where svihmm_read_packed continues as after svihmm_allreduce_packed (hmmsgd_metaobs.py:430-436). */
int svihmm_export_packed(svihmm_ctx* h, double* out_packed);
int svihmm_import_packed(svihmm_ctx* h, const double* packed_in);
/* Generic all-reduce of a small host vector (op 0: sum, 1: max) through HBM;
 * used for barriers and max-over-ranks timing. */
int svihmm_allreduce_host(svihmm_ctx* h, double* buf, int64_t n, int32_t op);

/* Measurement hooks (per-kernel HIP-event timing, kernel-generation selection for A/B runs and the
 * test suite, the MFMA operand-layout self-test) are NOT part of this boundary: include/svihmm_debug.h. */

#ifdef __cplusplus
}
#endif
#endif /* SVIHMM_H */
