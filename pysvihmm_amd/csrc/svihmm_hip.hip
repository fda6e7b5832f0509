// svihmm_hip.hip -- MI355X (gfx950 / CDNA4) SVI-HMM E-step engine: kernels + C ABI.
//
// Hot path of dillonalaird/pysvihmm (see include/svihmm.h for the reference
// file:line each entry point replaces).  Everything is fp64 (the reference is
// float64 throughout, hmmbase.py:102-103).
//
// Data layout in HBM (all row-major float64):
//   obs   [T][D]                  resident for the life of the handle
//   theta [Fp][Kp]                emission parameters in "augmented feature" form:
//                                 feature f=(a,b), 0<=a<=b<=D over x~=(x_0..x_{D-1},1):
//                                 phi_f(x) = x~_a * x~_b ;  ll[t,k] = sum_f phi_f(x_t) theta[f,k]
//   ll / la / lb / q [B*Lm][K]    per-window intermediates (window-major == API layout)
//   part  [nchunk][Ftot][Kp]      per-workgroup partial statistics, Ftot = Fp + Kp
//                                 rows [0,Fp): sum_t phi_f(x_t) q[t,k]  (S, xbar, neff)
//                                 rows [Fp,Fp+Kp): sum_t q[t-1,i] q[t,k] (transition stat)
//   packed [K*K + K*D + K + K*D*D + 1]
//
// Recursions: log-domain storage, linear-domain mat-vec.  With m = max_i la[t-1,i],
//   la[t,j] = m + log( sum_i exp(la[t-1,i]-m) * exp(ltran[i,j]) ) + ll[t,j]
// is algebraically the reference's LSE_i(la[t-1,i] + ltran[i,j]) + ll[t,j]
// (hmmbase.py:295) with K exps + K logs per step instead of K^2.
#include "host.h"
#include <algorithm>
#include "device_helpers.h"
#include "kernels_misc.h"
#include "kernels_heldout.h"
#include "kernels_expect.h"
#include "kernels_svi.h"

thread_local std::string g_err;
static const char* kKernNames[SVIHMM_NKERN] = {
    "emission", "forward_backward", "posterior", "stats", "finalize", "ffbs_sample",
    "misc", "allreduce", "h2d", "d2h", "reserved0", "reserved1"};

extern "C" {

const char* svihmm_last_error(void) { return g_err.c_str(); }
int svihmm_abi_version(void) { return SVIHMM_ABI_VERSION; }
const char* svihmm_kernel_name(int32_t slot) {
  return (slot >= 0 && slot < SVIHMM_NKERN) ? kKernNames[slot] : "";
}

int svihmm_device_count(int* n_out) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) { *n_out = 0; return fail(std::string("hipGetDeviceCount: ") + hipGetErrorString(e)); }
  *n_out = n;
  return 0;
}

int svihmm_create(int device_id, svihmm_ctx** out) {
  if (!out) return fail("svihmm_create: out is NULL");
  int n = 0;
  HIPCK(hipGetDeviceCount(&n));
  if (n <= 0) return fail("svihmm_create: no HIP device visible (the HIP path has no CPU fallback)");
  if (device_id < 0 || device_id >= n) return fail("svihmm_create: bad device id");
  svihmm_ctx* h = new svihmm_ctx();
  h->device = device_id;
  HIPCK(hipSetDevice(device_id));
  HIPCK(hipStreamCreateWithFlags(&h->stream, hipStreamNonBlocking));
  {   // the device's shape, once: batch-size thresholds and workgroup rounds are expressed through it (host.h, cu_scaled)
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, device_id) == hipSuccess && v > 0) h->ncu = v;
    v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxThreadsPerMultiProcessor, device_id) == hipSuccess && v >= 64)
      h->waves_per_cu = v / 64;
  }
  *out = h;
  return 0;
}

int svihmm_destroy(svihmm_ctx* h) {
  if (!h) return 0;
  hipSetDevice(h->device);
  hipStreamSynchronize(h->stream);
  if (h->stream2) hipStreamSynchronize(h->stream2);   // side streams of the SVI loop may still
  if (h->stream3) hipStreamSynchronize(h->stream3);   // hold kernels that touch the buffers below
  if (h->comm) { ncclCommDestroy(h->comm); h->comm = nullptr; }
  for (auto& p : h->pending) { hipEventDestroy(p.e0); hipEventDestroy(p.e1); }
  for (auto e : h->pool) hipEventDestroy(e);
  Buf* bufs[] = {&h->obs, &h->mask, &h->mod_init, &h->ltran, &h->Aexp, &h->AexpT, &h->theta, &h->niw,
                 &h->fab, &h->starts, &h->user_q, &h->user_starts, &h->vit, &h->ll, &h->la, &h->lb, &h->q, &h->lse_part,
                 &h->local_lb, &h->logz, &h->part, &h->packed, &h->scratch, &h->kexp, &h->hx, &h->gx,
                 &h->zfac, &h->llE, &h->m_ll, &h->m_la, &h->m_lb, &h->chain, &h->chain2, &h->cat_table, &h->mcat_meta, &h->pois_logfact, &h->pg_origin, &h->partc, &h->theta_orb, &h->prior, &h->vlb_aux, &h->gen_z,
                 &h->svi_state, &h->svi_prior, &h->svi_work, &h->commtmp, &h->ll0, &h->a0v, &h->a0e,
                 &h->shift_d, &h->uwb, &h->uwd, &h->AexpF, &h->AexpTF, &h->svi_sync, &h->pipe_cnt,
                 &h->pipe_tabs[0].buf, &h->pipe_tabs[1].buf, &h->pipe_tabs[2].buf, &h->pipe_tabs[3].buf,
                 &h->pipe_tabs[4].buf, &h->pipe_tabs[5].buf, &h->pipe_tabs[6].buf, &h->pipe_tabs[7].buf,
                 &h->seq_off_d, &h->seq_q, &h->seq_work, &h->seq_ord, &h->seq_out, &h->dec_tab,
                 &h->sub_obs, &h->sub_mask, &h->sub_tab, &h->heldout, &h->labels, &h->sub_labels,
                 &h->sets, &h->sub_sets};
  for (Buf* b : bufs) release(*b);
  if (h->vlb_host) { hipHostFree(h->vlb_host); h->vlb_host = nullptr; }
  if (h->svi_elbo) { hipHostFree(h->svi_elbo); h->svi_elbo = nullptr; }
  if (h->svi_ea) hipEventDestroy(h->svi_ea);
  if (h->svi_eb) hipEventDestroy(h->svi_eb);
  if (h->svi_ec) hipEventDestroy(h->svi_ec);
  if (h->svi_ed) hipEventDestroy(h->svi_ed);
  if (h->stream3) hipStreamDestroy(h->stream3);
  for (auto e : h->svi_ev) hipEventDestroy(e);
  for (int i = 0; i < 2; ++i) {
    if (h->ev_em[i]) hipEventDestroy(h->ev_em[i]);
    if (h->ev_sw[i]) hipEventDestroy(h->ev_sw[i]);
  }
  if (h->stream2) hipStreamDestroy(h->stream2);
  for (auto& ps : h->pins) { if (ps.p) hipHostFree(ps.p); if (ps.ev) hipEventDestroy(ps.ev); }
  for (auto& ss : h->svi_starts) if (ss.p) hipHostFree(ss.p);
  if (h->pin_status) hipHostFree(h->pin_status);
  if (h->svi_ts) hipHostFree(h->svi_ts);
  if (h->starts_slot) hipHostFree(h->starts_slot);
  if (h->mirror) hipHostFree(h->mirror);
  hipStreamDestroy(h->stream);
  delete h;
  return 0;
}

static int check_emission_status(svihmm_ctx* h);
static int pinned(svihmm_ctx* h, size_t bytes, void** out, int* slot_out);
static int pull_small(svihmm_ctx* h, void* dst, const void* pin, size_t bytes);
static int pin_release(svihmm_ctx* h, int slot);
static double* svi_ptr(svihmm_ctx* h, int which);
static int wait_side_streams(svihmm_ctx* h);
static void sample_center(const svihmm_ctx* h, const double* obs, int64_t T, int D, std::vector<double>& c);
static int reset_shift(svihmm_ctx* h, const std::vector<double>& c, int64_t row0, int64_t nrows);
static int shift_rows(svihmm_ctx* h, const double* delta, int64_t row0, int64_t nrows, int round_symbols);
static int store_shift(svihmm_ctx* h, const std::vector<double>& c);
static int params_follow_centre(svihmm_ctx* h, const double* delta);
static int drop_auto_status(svihmm_ctx* h);
static int d2h_sync_small(svihmm_ctx* h, void* dst, const void* src, size_t bytes);
static int upload_staged(svihmm_ctx* h, void* dst, const void* src, size_t bytes);
static void to_centred(const svihmm_ctx* h, double* mu, int K, int D);
// The side-stream ELBO kernels in flight read niw / theta / logdet / var_tran: the stream waits for their event before
// any of those is rewritten
static int wait_vlb(svihmm_ctx* h) {
  if (h->vlb_pending) { HIPCK(hipStreamWaitEvent(h->stream, h->svi_ed, 0)); h->vlb_pending = false; }
  return 0;
}
// Upload the pieces, end to end, into dst through one pinned staging slot: pulled by a kernel, no stream
// synchronisation.  centre_K > 0: the leading [centre_K][centre_D] block is means in the caller's coordinates and
// travels centred (to_centred).  On a failure the slot is simply not marked busy.
struct Piece { const double* p; size_t n; };
static int upload_blocks(svihmm_ctx* h, void* dst, std::initializer_list<Piece> pieces, int centre_K = 0,
                         int centre_D = 0) {
  size_t n = 0;
  for (const Piece& q : pieces) n += q.n;
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, n * sizeof(double), &pin, &slot));
  double* hp = (double*)pin;
  for (const Piece& q : pieces) { std::memcpy(hp, q.p, q.n * sizeof(double)); hp += q.n; }
  if (centre_K > 0) to_centred(h, (double*)pin, centre_K, centre_D);
  CK(pull_small(h, dst, pin, n * sizeof(double)));
  return pin_release(h, slot);
}
int svihmm_set_precision(svihmm_ctx* h, int32_t mode) {
  if (!h || (mode != SVIHMM_F64 && mode != SVIHMM_F32)) return fail("svihmm_set_precision: mode must be SVIHMM_F64 or SVIHMM_F32");
  h->prec = mode;
  return 0;
}
// whether the last E-step batch ran in fp32: a value held over calls that are no E-step batch, else the live flags
static int f32_report(const svihmm_ctx* h) {
  return h->f32_report_hold >= 0 ? h->f32_report_hold : (h->cur_f32 || h->eh_float) ? 1 : 0;
}
// Holds that report over a pass that is not an E-step batch of the caller's, on every path out of the scope.
// internal: the pass addresses declared sequences' rows as windows of its own (seq_internal lifts the boundary
// check); fp64: the precision mode is set aside for the pass.
struct ReportHold {
  svihmm_ctx* h; int report, prec; bool internal;
  ReportHold(svihmm_ctx* h_, bool internal_, bool fp64) : h(h_), report(f32_report(h_)), prec(h_->prec), internal(internal_) {
    if (internal) h->seq_internal = true;
    if (fp64) h->prec = 0;
  }
  ~ReportHold() {
    if (internal) h->seq_internal = false;
    h->prec = prec;
    h->f32_report_hold = report;
  }
};
int svihmm_get_precision(svihmm_ctx* h, int32_t* mode_out, int32_t* last_batch_f32_out) {
  if (!h) return fail("svihmm_get_precision: NULL handle");
  if (mode_out) *mode_out = h->prec;
  if (last_batch_f32_out) *last_batch_f32_out = f32_report(h);
  return 0;
}
int svihmm_sync(svihmm_ctx* h) {
  CK(set_device(h));
  HIPCK(hipStreamSynchronize(h->stream));
  if (h->stream2) HIPCK(hipStreamSynchronize(h->stream2));
  if (h->stream3) HIPCK(hipStreamSynchronize(h->stream3));
  return check_emission_status(h);
}

int svihmm_set_obs(svihmm_ctx* h, const double* obs, int64_t T, int32_t D,
                   const uint8_t* mask) {
  if (!h || !obs || T <= 0 || D <= 0) return fail("svihmm_set_obs: bad arguments");
  if (D > 4095) return fail("svihmm_set_obs: D too large");
  CK(set_device(h));
  h->lin_stale = true;
  ProfScope ps(h, KS_H2D);
  CK(ensure(h->obs, (size_t)T * D * sizeof(double)));
  HIPCK(hipMemcpyAsync(h->obs.p, obs, (size_t)T * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  h->have_mask = mask != nullptr;
  if (mask) {
    CK(ensure(h->mask, (size_t)T));
    HIPCK(hipMemcpyAsync(h->mask.p, mask, (size_t)T, hipMemcpyHostToDevice, h->stream));
  }
  h->T = T; h->D = D; h->gen_T = 0;
  drop_clamp(h);                       // (labels / allowed-state sets described the previous rows)
  h->post_kind = 0;                    // (a held posterior batch described the previous rows)
  h->seq_off.clear();                  // (a declaration of sequences described the previous rows)
  h->svi_active = false;               // a resident SVI state belonged to the previous sequence
  h->center_pending = false;
  std::vector<double> c;
  sample_center(h, obs, T, D, c);
  CK(reset_shift(h, c, 0, T));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- the handle's shift (see svihmm_ctx::shift) ---------------------------------------------
// A point inside the data: per column the mean of the finite entries of a strided sample of rows.
// Any vector works (the model is shift-equivariant); what matters is |x - c| being of the size of
// the data's spread, so that the emission GEMM's expanded quadratic form does not cancel.
static void sample_center(const svihmm_ctx* h, const double* obs, int64_t T, int D, std::vector<double>& c) {
  c.assign((size_t)D, 0.0);
  const_cast<svihmm_ctx*>(h)->center_deferred = false;
  if (h->variant[SVIHMM_VAR_CENTRING] == SVIHMM_CENTRING_OFF || !obs || T <= 0) return;      // (no automatic centring)
  // a Categorical table is the active emission: the column holds symbol indices, which the lookup
  // kernels truncate to int -- it stays exactly as uploaded (round-3 advisor finding: set_emission_cat
  // followed by set_obs centred the symbols)
  if (h->have_emission && fam_table(h->fam)) { const_cast<svihmm_ctx*>(h)->center_deferred = true; return; }
  int64_t nsamp = ((int64_t)4 << 20) / D;
  if (nsamp > 65536) nsamp = 65536;
  if (nsamp < 16) nsamp = 16;
  if (nsamp > T) nsamp = T;
  const int64_t stride = T / nsamp;
  std::vector<int64_t> cnt((size_t)D, 0);
  for (int64_t i = 0; i < nsamp; ++i) {
    const double* row = obs + (size_t)(i * stride) * D;
    for (int d = 0; d < D; ++d) {
      const double v = row[d];
      if (finite_val(v)) { c[d] += v; ++cnt[d]; }
    }
  }
  for (int d = 0; d < D; ++d) {
    c[d] = cnt[d] > 0 ? c[d] / (double)cnt[d] : 0.0;
    if (!finite_val(c[d])) c[d] = 0.0;
  }
}
// rows [row0, row0 + nrows) of the resident copy -= delta[D] (host vector)
static int shift_rows(svihmm_ctx* h, const double* delta, int64_t row0, int64_t nrows, int round_symbols) {
  const int D = h->D;
  bool any = false;
  for (int d = 0; d < D; ++d) any = any || delta[d] != 0.0;
  if (!any || nrows <= 0) return 0;
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, (size_t)D * sizeof(double), &pin, &slot));
  std::memcpy(pin, delta, (size_t)D * sizeof(double));
  void* dpin = nullptr;
  HIPCK(hipHostGetDevicePointer(&dpin, pin, 0));
  const int64_t n = nrows * (int64_t)D;
  double* base = (double*)h->obs.p + (size_t)row0 * D;
  // round_symbols: 0 plain shift, 1 symbols (every entry to the nearest integer), 2 counts (k_shift_obs: entries at an
  // integer snap to it, fractional ones keep their value)
  if (round_symbols == 2)
    hipLaunchKernelGGL(k_shift_obs<2>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, base, n, D,
                       (const double*)dpin);
  else if (round_symbols)
    hipLaunchKernelGGL(k_shift_obs<1>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, base, n, D,
                       (const double*)dpin);
  else
    hipLaunchKernelGGL(k_shift_obs<0>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, base, n, D,
                       (const double*)dpin);
  HIPCK(hipGetLastError());
  CK(pin_release(h, slot));
  return 0;
}
// record c as the handle's shift (host + device copy)
static int store_shift(svihmm_ctx* h, const std::vector<double>& c) {
  const int D = h->D;
  h->shift = c;
  h->shifted = false;
  for (int d = 0; d < D; ++d) h->shifted = h->shifted || c[d] != 0.0;
  ++h->shift_epoch;
  CK(ensure(h->shift_d, (size_t)D * sizeof(double)));
  return upload_blocks(h, h->shift_d.p, {{c.data(), (size_t)D}});
}
// The centre moved by delta[D]: device-side parameters kept in centred coordinates follow -- the
// means of the NIW / diagonal factors in h->niw (theta is rebuilt), the prior means of a running
// SVI loop.  What the caller uploaded keeps its meaning.
static int params_follow_centre(svihmm_ctx* h, const double* delta) {
  const int D = h->D;
  bool any = false;
  for (int d = 0; d < D; ++d) any = any || delta[d] != 0.0;
  const bool live = h->have_emission && fam_gaussian(h->fam) && h->eD == D && h->niw.p;   // (NIW or diagonal: means lead the block)
  const bool svi = h->svi_active && h->svi_D == D && fam_gaussian(h->svi_family);    // (symbol and count families: no means)
  if (!any || (!live && !svi)) return 0;
  CK(wait_side_streams(h));
  if (live) CK(drop_auto_status(h));      // this rebuild supersedes what an earlier automatic one reported
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, (size_t)D * sizeof(double), &pin, &slot));
  std::memcpy(pin, delta, (size_t)D * sizeof(double));
  void* dpin = nullptr;
  HIPCK(hipHostGetDevicePointer(&dpin, pin, 0));
  if (live) {
    const int n = h->eK * D;
    hipLaunchKernelGGL(k_shift_means, dim3((n + 255) / 256), dim3(256), 0, h->stream, (double*)h->niw.p, n, D,
                       (const double*)dpin);
  }
  if (svi) {
    const int n = h->svi_K * D;
    hipLaunchKernelGGL(k_shift_means, dim3((n + 255) / 256), dim3(256), 0, h->stream, (double*)h->svi_prior.p, n, D,
                       (const double*)dpin);
  }
  HIPCK(hipGetLastError());
  CK(pin_release(h, slot));
  if (live && h->fam == EF_DIAG) CK(launch_diag_to_theta(h, h->eK, D));
  else if (live) CK(launch_niw_to_theta(h, h->eK, D, svi ? svi_ptr(h, 4) : nullptr));
  if (live) h->status_auto = true;
  return 0;
}
// An explicit parameter upload supersedes whatever an automatic rebuild of theta reported (new
// observations uploaded under the previous model's factors may lie anywhere relative to them).
static int drop_auto_status(svihmm_ctx* h) {
  if (h->status_pending && h->status_auto) {
    HIPCK(hipStreamSynchronize(h->stream));
    if (h->pin_status) *h->pin_status = 0;
    h->status_pending = false;
  }
  h->status_auto = false;
  return 0;
}
// freshly written rows [row0, row0 + nrows) hold caller coordinates: c becomes the shift, rows move,
// parameters already on the device follow the change of centre
static int reset_shift(svihmm_ctx* h, const std::vector<double>& c, int64_t row0, int64_t nrows) {
  std::vector<double> delta(c);
  if ((int)h->shift.size() == h->D)
    for (int d = 0; d < h->D; ++d) delta[d] -= h->shift[d];
  CK(store_shift(h, c));
  CK(shift_rows(h, c.data(), row0, nrows, 0));
  return params_follow_centre(h, delta.data());
}

int svihmm_shift_obs(svihmm_ctx* h, const double* shift) {
  if (!h || !shift) return fail("svihmm_shift_obs: bad arguments");
  if (h->T <= 0 || !h->obs.p) return fail("svihmm_shift_obs: no resident observations");
  CK(set_device(h));
  h->lin_stale = true;
  const int D = h->D;
  for (int d = 0; d < D; ++d)
    if (!finite_val(shift[d])) return fail("svihmm_shift_obs: shift must be finite");
  CK(wait_side_streams(h));
  CK(shift_rows(h, shift, 0, h->T, 0));
  std::vector<double> c = h->shift;
  c.resize((size_t)D, 0.0);
  for (int d = 0; d < D; ++d) c[d] += shift[d];
  CK(store_shift(h, c));
  return params_follow_centre(h, shift);
}
int svihmm_get_shift(svihmm_ctx* h, double* shift_out) {
  if (!h || !shift_out) return fail("svihmm_get_shift: bad arguments");
  if (h->T <= 0) return fail("svihmm_get_shift: no resident observations");
  for (int d = 0; d < h->D; ++d) shift_out[d] = d < (int)h->shift.size() ? h->shift[d] : 0.0;
  return 0;
}

// Chunked upload for sequences that arrive in pieces (gen_synthetic.py:188-191 read_data_mmap
// yields [size, D] blocks of the on-disk float64 array): svihmm_alloc_obs sizes the resident
// copy, svihmm_set_obs_rows fills rows [row0, row0 + nrows).  Each call returns once its
// block is on the device (the caller may reuse the block).
int svihmm_alloc_obs(svihmm_ctx* h, int64_t T, int32_t D, int32_t with_mask) {
  if (!h || T <= 0 || D <= 0) return fail("svihmm_alloc_obs: bad arguments");
  if (D > 4095) return fail("svihmm_alloc_obs: D too large");
  CK(set_device(h));
  h->lin_stale = true;
  CK(ensure(h->obs, (size_t)T * D * sizeof(double)));
  h->have_mask = with_mask != 0;
  if (with_mask) {
    CK(ensure(h->mask, (size_t)T));
    HIPCK(hipMemsetAsync(h->mask.p, 0, (size_t)T, h->stream));
  }
  h->T = T; h->D = D; h->gen_T = 0;
  drop_clamp(h);
  h->post_kind = 0;
  h->seq_off.clear();
  h->svi_active = false;
  CK(reset_shift(h, std::vector<double>((size_t)D, 0.0), 0, 0));
  h->center_pending = true;            // the first block that arrives fixes the shift
  return 0;
}
int svihmm_set_obs_rows(svihmm_ctx* h, int64_t row0, int64_t nrows, const double* obs,
                        const uint8_t* mask) {
  if (!h || !obs || row0 < 0 || nrows <= 0) return fail("svihmm_set_obs_rows: bad arguments");
  if (h->T <= 0 || row0 + nrows > h->T) return fail("svihmm_set_obs_rows: rows outside the allocated sequence");
  if (mask && !h->have_mask) return fail("svihmm_set_obs_rows: sequence was allocated without a mask");
  CK(set_device(h));
  h->lin_stale = true;
  ProfScope ps(h, KS_H2D);
  const size_t D = (size_t)h->D;
  HIPCK(hipMemcpyAsync((double*)h->obs.p + (size_t)row0 * D, obs, (size_t)nrows * D * sizeof(double),
                       hipMemcpyHostToDevice, h->stream));
  if (mask)
    HIPCK(hipMemcpyAsync((uint8_t*)h->mask.p + row0, mask, (size_t)nrows, hipMemcpyHostToDevice, h->stream));
  if (h->center_pending) {
    h->center_pending = false;
    std::vector<double> c;
    sample_center(h, obs, nrows, h->D, c);
    CK(reset_shift(h, c, 0, 0));         // (rows written before this call would be undefined anyway)
  }
  CK(shift_rows(h, h->shift.data(), row0, nrows, 0));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

// Known states of the resident rows (include/svihmm.h).  Everything that can be wrong is found before the upload, so
// a refused call leaves the labels in force as they were.
int svihmm_set_labels(svihmm_ctx* h, const int32_t* labels) {
  const char* fn = "svihmm_set_labels";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!labels) { h->have_labels = false; h->lin_stale = true; return 0; }
  if (h->T <= 0 || !h->obs.p) return bad("no observations: call svihmm_set_obs first");
  int32_t mx = -1;
  int64_t mx_row = -1;
  for (int64_t t = 0; t < h->T; ++t) {
    if (labels[t] < -1)
      return bad("labels[" + std::to_string(t) + "] = " + std::to_string(labels[t]) +
                 " (-1 means free, a state index means known)");
    if (labels[t] > mx) { mx = labels[t]; mx_row = t; }
  }
  CK(set_device(h));
  CK(ensure(h->labels, (size_t)h->T * sizeof(int32_t)));
  CK(upload_staged(h, h->labels.p, labels, (size_t)h->T * sizeof(int32_t)));
  HIPCK(hipStreamSynchronize(h->stream));
  h->have_labels = true;
  h->have_sets = false;                // (labels and allowed-state sets are alternatives)
  h->label_max = mx; h->label_max_row = mx_row;
  h->lin_stale = true;                 // (lliks held were evaluated under the previous labels)
  return 0;
}

// Allowed-state sets of the resident rows (include/svihmm.h): one pass over the host array finds the first offending
// row before the upload, so a refused call leaves whatever was in force as it was.
int svihmm_set_state_sets(svihmm_ctx* h, const uint64_t* allowed, int32_t K) {
  const char* fn = "svihmm_set_state_sets";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!allowed) { h->have_sets = false; h->lin_stale = true; return 0; }
  if (h->T <= 0 || !h->obs.p) return bad("no observations: call svihmm_set_obs first");
  if (K < 1 || K > 256) return bad("K = " + std::to_string(K) + " is outside [1, 256]");
  const int W = (K + 63) / 64, tail = K - (W - 1) * 64;
  const uint64_t beyond = tail == 64 ? 0ull : ~0ull << tail;       // the last word's bits at or beyond K
  for (int64_t t = 0; t < h->T; ++t) {
    const uint64_t* row = allowed + t * W;
    if (row[W - 1] & beyond) {
      const int k = (W - 1) * 64 + __builtin_ctzll(row[W - 1] & beyond);
      return bad("row " + std::to_string(t) + " has bit " + std::to_string(k) + " set, at or beyond K = " +
                 std::to_string(K) + " (the padding bits of the last word must be zero)");
    }
    uint64_t any = 0;
    for (int j = 0; j < W; ++j) any |= row[j];
    if (!any) return bad("row " + std::to_string(t) + " allows no state (a free row has all K bits set)");
  }
  const size_t bytes = (size_t)h->T * W * sizeof(uint64_t);
  CK(set_device(h));
  CK(ensure(h->sets, bytes));
  CK(upload_staged(h, h->sets.p, allowed, bytes));
  HIPCK(hipStreamSynchronize(h->stream));
  h->have_sets = true;
  h->have_labels = false;              // (labels and allowed-state sets are alternatives)
  h->sets_K = K; h->sets_W = W;
  h->lin_stale = true;                 // (lliks held were evaluated under the previous clamp)
  return 0;
}

// SVIHMM_LTRAN_LINEAR_MIN: exp(-600) = 1e-261 is a normal double with 1e-47 of headroom for
// products with a scaled message; below it: k_fb_exact
int svihmm_set_globals(svihmm_ctx* h, int32_t K, const double* mod_init, const double* ltran) {
  if (!h || K <= 0 || !mod_init || !ltran) return fail("svihmm_set_globals: bad arguments");
  if (K > 1024) return fail("svihmm_set_globals: K > 1024 unsupported");
  CK(set_device(h));
  CK(wait_globals(h));               // a globals kernel of the SVI loop may still be writing them
  h->svi_globals_ready = false;
  h->lin_stale = true;
  const size_t kk = (size_t)K * K * sizeof(double);
  CK(ensure(h->mod_init, K * sizeof(double)));
  CK(ensure(h->ltran, kk));
  // zero rows behind each matrix: the wide-model sweeps stream whole row tiles of the transition
  // matrix up to the width they are instantiated for (128 rows for 64 < K <= 128, 256 beyond),
  // not just up to K rounded to a tile
  const int reach = K <= 64 ? (K + 15) / 16 * 16 : K <= 128 ? 128 : K <= 256 ? 256 : K;
  const size_t slack = (size_t)(reach - K + 16) * K * sizeof(double);
  CK(ensure(h->Aexp, kk + slack));
  CK(ensure(h->AexpT, kk + slack));
  if (h->slack_a != h->Aexp.p || h->slack_t != h->AexpT.p || h->slack_k != K) {   // once per (buffers, K)
    HIPCK(hipMemsetAsync((char*)h->Aexp.p + kk, 0, slack, h->stream));
    HIPCK(hipMemsetAsync((char*)h->AexpT.p + kk, 0, slack, h->stream));
    h->slack_a = h->Aexp.p; h->slack_t = h->AexpT.p; h->slack_k = K;
  }
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, kk + K * sizeof(double), &pin, &slot));
  std::memcpy(pin, ltran, kk);
  std::memcpy((char*)pin + kk, mod_init, K * sizeof(double));
  {
    ProfScope ps(h, KS_MISC);
    void* dpin = nullptr;
    HIPCK(hipHostGetDevicePointer(&dpin, pin, 0));
    hipLaunchKernelGGL(k_exp_transpose, dim3((K * K + 255) / 256), dim3(256), 0, h->stream,
                       (const double*)dpin, K, (double*)h->ltran.p, (double*)h->mod_init.p,
                       (double*)h->Aexp.p, (double*)h->AexpT.p);
  }
  HIPCK(hipGetLastError());
  CK(pin_release(h, slot));   // guards the slot until the kernel has read it
  h->K = K; h->have_globals = true;
  // dynamic range of the transition expectations (K^2 values, host side): exp(ltran) must stay a
  // normal double with headroom for the scaled recursions, a normal float for the fp32 mode
  double lmin = 0.0;
  bool finite = true;
  for (size_t i = 0; i < (size_t)K * K; ++i) {
    const double v = ltran[i];
    if (!finite_val(v)) finite = false;
    else if (v < lmin) lmin = v;
  }
  h->exact_log = !finite || lmin < SVIHMM_LTRAN_LINEAR_MIN;
  h->f32_ok = finite && lmin > SVIHMM_LTRAN_F32_MIN;
  return 0;
}

// acquire the next staging slot (waits only if the copy that last used it is still in flight,
// i.e. six uploads ago); pin_release() records the guard event after the copy is enqueued
static int pinned(svihmm_ctx* h, size_t bytes, void** out, int* slot_out) {
  svihmm_ctx::PinSlot& ps = h->pins[h->pin_next];
  *slot_out = h->pin_next;
  h->pin_next = (h->pin_next + 1) % 6;
  if (ps.busy) { HIPCK(hipEventSynchronize(ps.ev)); ps.busy = false; }
  if (bytes > ps.cap) {
    if (ps.p) hipHostFree(ps.p);
    ps.p = nullptr; ps.cap = 0;
    HIPCK(hipHostMalloc(&ps.p, bytes + 4096, hipHostMallocMapped));   // kernels pull from the slots
    ps.cap = bytes + 4096;
  }
  if (!ps.ev) HIPCK(hipEventCreateWithFlags(&ps.ev, hipEventDisableTiming));
  *out = ps.p;
  return 0;
}
static int pin_release(svihmm_ctx* h, int slot) {
  svihmm_ctx::PinSlot& ps = h->pins[slot];
  HIPCK(hipEventRecord(ps.ev, h->stream));
  ps.busy = true;
  return 0;
}
// call after a stream synchronisation: reports a failed NIW factorisation of the last
// svihmm_set_emission_niw (which itself returns without waiting for the device)
static int check_emission_status(svihmm_ctx* h) {
  if (!h->status_pending) return 0;
  h->status_pending = false;
  const int st = h->pin_status ? *h->pin_status : 0;
  if (h->pin_status) *h->pin_status = 0;   // sticky until read: reset only here (stream idle)
  if (st > NIW_STATUS_RANGE) {
    h->have_emission = false;
    return fail("svihmm_set_emission_niw: factor " + std::to_string(st - NIW_STATUS_RANGE - 1) +
                " lies too far from the centre of the resident observations for its spread "
                "((mu-c)' (nu/2 sigma^-1) (mu-c) > 1e9): the expanded quadratic form would lose more than "
                "5e-7 in the log-likelihoods -- svihmm_shift_obs moves the centre (svihmm_get_shift reads it)");
  }
  if (st != 0) {
    h->have_emission = false;
    return fail("svihmm_set_emission_niw: sigma_mf[" + std::to_string(st - 1) + "] is not positive definite");
  }
  return 0;
}

// ---- NIW -> theta on the device (k_niw_to_theta) -------------------------------------
static inline int feat_index(int a, int b, int D) {  // 0 <= a <= b <= D
  return a * (D + 1) - a * (a - 1) / 2 + (b - a);
}

// Features are products x~_a x~_b of the augmented row x~ = (x, 1); the table lists the (a, b) the
// emission family needs.  Full covariance: all a <= b, F = (D+1)(D+2)/2.  Diagonal family:
// x_a^2 (f = a), x_a (f = D + a), 1 (f = 2 D): F = 2 D + 1.  Emission and statistics GEMMs read
// the table, so the family only changes the table and the theta builder.
int upload_feature_table(svihmm_ctx* h, int D, int K, bool diag) {
  const int F = diag ? 2 * D + 1 : (D + 1) * (D + 2) / 2, Fp = (F + 15) / 16 * 16;
  const int Kp = padded_K(K);
  if (h->tabD == D && h->Fp == Fp && h->tab_diag == diag) { h->F = F; h->Kp = Kp; return 0; }
  std::vector<int> fab(Fp, (D + 1) | ((D + 1) << 16));  // padding -> zero slot
  if (diag) {
    for (int a = 0; a < D; ++a) { fab[a] = a | (a << 16); fab[D + a] = a | (D << 16); }
    fab[2 * D] = D | (D << 16);
  } else
  for (int a = 0; a <= D; ++a)
    for (int b = a; b <= D; ++b) fab[feat_index(a, b, D)] = a | (b << 16);
  CK(ensure(h->fab, fab.size() * sizeof(int)));
  HIPCK(hipMemcpyAsync(h->fab.p, fab.data(), fab.size() * sizeof(int), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  h->tabD = D; h->F = F; h->Fp = Fp; h->Kp = Kp; h->tab_diag = diag;
  return 0;
}


// means[K][D] in the caller's coordinates -> centred coordinates (and back), in place on the host
static void to_centred(const svihmm_ctx* h, double* mu, int K, int D) {
  if (!h->shifted || (int)h->shift.size() != D) return;
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) mu[(size_t)k * D + d] -= h->shift[d];
}
static void from_centred(const svihmm_ctx* h, double* mu, int K, int D) {
  if (!h->shifted || (int)h->shift.size() != D) return;
  for (int k = 0; k < K; ++k)
    for (int d = 0; d < D; ++d) mu[(size_t)k * D + d] += h->shift[d];
}
// A Categorical table was active when the resident copy was uploaded (or un-centred it): the copy
// holds caller coordinates.  A Gaussian family that arrives now gets the centring the upload skipped:
// column means of a strided row sample, taken on the device (k_col_mean), then the usual shift.
static int centre_deferred(svihmm_ctx* h) {
  if (!h->center_deferred) return 0;
  h->center_deferred = false;
  if (h->T <= 0 || !h->obs.p || h->shifted || h->variant[SVIHMM_VAR_CENTRING] == SVIHMM_CENTRING_OFF) return 0;
  const int D = h->D;
  int64_t nsamp = ((int64_t)4 << 20) / D;
  if (nsamp > 65536) nsamp = 65536;
  if (nsamp < 16) nsamp = 16;
  if (nsamp > h->T) nsamp = h->T;
  const int64_t stride = h->T / nsamp;
  CK(ensure(h->scratch, (size_t)D * sizeof(double)));
  hipLaunchKernelGGL(k_col_mean, dim3((unsigned)D), dim3(256), 0, h->stream, (const double*)h->obs.p, D, stride,
                     nsamp, (double*)h->scratch.p);
  HIPCK(hipGetLastError());
  std::vector<double> c((size_t)D, 0.0);
  CK(d2h_sync_small(h, c.data(), h->scratch.p, (size_t)D * sizeof(double)));
  return reset_shift(h, c, 0, h->T);
}

// ---- what every svihmm_set_emission_* does between its argument checks and its first ensure ---------------------
// The live device loop is of this family and this shape: the upload re-pushes the loop's own factors' table (the
// validation hooks of infer() -- full_predprob, adaptive L, growBuffer -- re-upload what they just read back) and the
// loop survives it.  W: the columns D, for EF_CAT the symbols V; V: the columns' symbol counts (EF_MCAT only).
static bool own_loop(const svihmm_ctx* h, EmisFamily fam, int K, int W, const int32_t* V = nullptr) {
  if (!h->svi_active || h->svi_family != fam || h->svi_K != K) return false;
  switch (fam) {
    case EF_NIW: case EF_DIAG: case EF_POIS: return h->svi_D == W;
    case EF_CAT: return h->V == W;
    case EF_MCAT: return h->svi_mcat_V == std::vector<int>(V, V + W);
    default: return false;             // (the resident loop does not know the family)
  }
}
// The emission is about to be rewritten, in this order ("putting a family in force"):
//   1. device, stale logs;
//   2. the centring the family wants (Gaussian: the one an upload under a table family deferred; table: none pending);
//   3. a live loop's deferred ELBO kernels, launched while the factors they read are still whole -- only then does a
//      loop that is not `own` end (it kept its factors in h->niw, which any family's arrival may rewrite or reallocate);
//   4. the stream behind the ELBO kernels in flight;  5. an automatic rebuild's status word dropped;
//   6. table families: the resident rows back in the caller's coordinates (uncentre: cat_uncentre's mode).
static int begin_emission_upload(svihmm_ctx* h, EmisFamily fam, int D, bool own, int uncentre = -1) {
  CK(set_device(h));
  h->lin_stale = true;
  if (fam_table(fam)) h->center_pending = false;
  else if (h->D == D) CK(centre_deferred(h));
  if (h->svi_active) CK(svi_flush_elbo(h));
  if (!own) h->svi_active = false;
  CK(wait_vlb(h));
  CK(drop_auto_status(h));
  if (fam_table(fam)) CK(cat_uncentre(h, uncentre));
  return 0;
}

int svihmm_set_emission_niw(svihmm_ctx* h, int32_t K, int32_t D, const double* mu,
                            const double* sigma, const double* kappa, const double* nu) {
  if (!h || K <= 0 || D <= 0 || !mu || !sigma || !kappa || !nu)
    return fail("svihmm_set_emission_niw: bad arguments");
  if (D > SVIHMM_NIW_MAX_D)   // (k_niw_to_theta_generic keeps two D x (D+1) matrices in LDS)
    return fail("svihmm_set_emission_niw: D > SVIHMM_NIW_MAX_D: evaluate the expected log-likelihoods on the "
                "host and pass them with svihmm_set_lliks / SVIHMM_USE_HOST_LLIKS");
  CK(begin_emission_upload(h, EF_NIW, D, own_loop(h, EF_NIW, K, D)));
  const size_t nmu = (size_t)K * D, nsg = (size_t)K * D * D;
  CK(ensure(h->niw, (nmu + nsg + 2 * (size_t)K) * sizeof(double) + 64));
  // (the resident observations are x - shift: so are the means)
  CK(upload_blocks(h, h->niw.p, {{mu, nmu}, {sigma, nsg}, {kappa, (size_t)K}, {nu, (size_t)K}}, K, D));
  return launch_niw_to_theta(h, K, D, nullptr);
}

int svihmm_set_emission_diag(svihmm_ctx* h, int32_t K, int32_t D, const double* mu, const double* nus,
                             const double* alphas, const double* betas) {
  if (!h || K <= 0 || D <= 0 || !mu || !nus || !alphas || !betas)
    return fail("svihmm_set_emission_diag: bad arguments");
  if (D > SVIHMM_DIAG_MAX_D)
    return fail("svihmm_set_emission_diag: D > SVIHMM_DIAG_MAX_D: evaluate the expected log-likelihoods on the "
                "host and pass them with svihmm_set_lliks / SVIHMM_USE_HOST_LLIKS");
  CK(begin_emission_upload(h, EF_DIAG, D, own_loop(h, EF_DIAG, K, D)));
  const size_t n = (size_t)K * D;
  CK(ensure(h->niw, 4 * n * sizeof(double) + 64));
  CK(upload_blocks(h, h->niw.p, {{mu, n}, {nus, n}, {alphas, n}, {betas, n}}, K, D));
  return launch_diag_to_theta(h, K, D);
}

// ---- ELBO terms of the NIW factors from the device-resident parameters --------------------
int svihmm_set_emission_prior(svihmm_ctx* h, int32_t K, int32_t D, const double* mu0, const double* sigma0) {
  if (!h || K <= 0 || D <= 0 || !mu0 || !sigma0) return fail("svihmm_set_emission_prior: bad arguments");
  CK(set_device(h));
  const size_t nmu = (size_t)K * D, nsg = (size_t)K * D * D;
  CK(ensure(h->prior, (nmu + nsg) * sizeof(double)));
  CK(upload_blocks(h, h->prior.p, {{mu0, nmu}, {sigma0, nsg}}, K, D));
  h->prior_K = K; h->prior_D = D;
  h->prior_mu0.assign(mu0, mu0 + nmu);     // re-centred when the handle's shift has moved since
  h->prior_epoch = h->shift_epoch;
  return 0;
}
int svihmm_niw_vlb_terms(svihmm_ctx* h, int32_t K, int32_t D, const double* mu, const double* sigma,
                         const double* kappa, const double* nu, double* out3K) {
  if (!h || K <= 0 || D <= 0 || !mu || !sigma || !kappa || !nu || !out3K)
    return fail("svihmm_niw_vlb_terms: bad arguments");
  if (h->prior_K != K || h->prior_D != D) return fail("svihmm_niw_vlb_terms: call svihmm_set_emission_prior first");
  if (D > SVIHMM_NIW_MAX_D) return fail("svihmm_niw_vlb_terms: D > SVIHMM_NIW_MAX_D");
  CK(set_device(h));
  CK(upload_feature_table(h, D, K));
  const int Fp = h->Fp, Kp = h->Kp;
  if (h->vlb_host_K < K) {
    if (h->vlb_host) hipHostFree(h->vlb_host);
    h->vlb_host = nullptr; h->vlb_host_K = 0;
    HIPCK(hipHostMalloc((void**)&h->vlb_host, (size_t)3 * K * sizeof(double), hipHostMallocMapped));
    h->vlb_host_K = K;
  }
  double* dout = nullptr;
  HIPCK(hipHostGetDevicePointer((void**)&dout, h->vlb_host, 0));
  // a private parameter / theta set: the E-step's own (h->niw, h->theta) stay untouched, so the
  // intermediates of the last E-step remain readable after the ELBO has been evaluated
  const size_t nmu = (size_t)K * D, nsg = (size_t)K * D * D, nin = nmu + nsg + 2 * (size_t)K;
  const size_t nth = (size_t)Fp * Kp;
  CK(ensure(h->vlb_aux, (nin + nth + K + 8) * sizeof(double)));
  double* dmu = (double*)h->vlb_aux.p;
  double* dsg = dmu + nmu;
  double* dka = dsg + nsg;
  double* dnu = dka + K;
  double* th2 = dnu + K;
  double* ld = th2 + nth;
  int* dstat = (int*)(ld + K);
  // (only differences mu - mu_0 enter; both travel centred)
  CK(upload_blocks(h, dmu, {{mu, nmu}, {sigma, nsg}, {kappa, (size_t)K}, {nu, (size_t)K}}, K, D));
  if (h->prior_epoch != h->shift_epoch) {
    CK(upload_blocks(h, h->prior.p, {{h->prior_mu0.data(), nmu}}, K, D));
    h->prior_epoch = h->shift_epoch;
  }
  const double* p0 = (const double*)h->prior.p;
  CK(launch_niw_vlb(h, K, D, dmu, dsg, dka, dnu, th2, dstat, ld, p0, dout));
  HIPCK(hipStreamSynchronize(h->stream));
  std::memcpy(out3K, h->vlb_host, (size_t)3 * K * sizeof(double));
  return 0;
}

// The resident column holds symbol indices: a centred copy (an upload cannot know the family that
// will read it; svihmm_shift_obs may have moved it) goes back to exact integers and stays uncentred.
// Called when the table is set and again in front of every lookup / count launch.
// counts: the family that reads the copy next is the Poisson one (-1: the family in force), whose fractional entries
// keep their value (k_shift_obs<2>); counts == 2: the real-valued one (svihmm_set_emission_pgauss), which takes the
// plain shift back (k_shift_obs<0>: the values return to rounding, not to the bit).
int cat_uncentre(svihmm_ctx* h, int counts) {
  if (h->T > 0) h->center_deferred = true;     // a Gaussian family that follows centres the copy again
  if (!h->shifted || h->T <= 0) return 0;
  std::vector<double> back(h->shift.size());
  for (size_t d = 0; d < back.size(); ++d) back[d] = -h->shift[d];
  if (counts < 0) counts = FAM_TRAITS[h->fam].uncentre;
  CK(shift_rows(h, back.data(), 0, h->T, counts == 2 ? 0 : counts ? 2 : 1));
  return store_shift(h, std::vector<double>((size_t)h->D, 0.0));
}
// feature table is also needed by the statistics kernels when only host lliks are used
int svihmm_set_emission_cat(svihmm_ctx* h, int32_t K, int32_t V, const double* logp) {
  if (!h || K <= 0 || V <= 0 || !logp) return fail("svihmm_set_emission_cat: bad arguments");
  CK(begin_emission_upload(h, EF_CAT, 1, own_loop(h, EF_CAT, K, V)));
  const size_t n = (size_t)K * V;
  CK(ensure(h->cat_table, n * sizeof(double)));
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, n * sizeof(double), &pin, &slot));
  double* hp = (double*)pin;
  for (int k = 0; k < K; ++k)              // transpose to [V][K]: a row's states are contiguous
    for (int v = 0; v < V; ++v) hp[(size_t)v * K + k] = logp[(size_t)k * V + v];
  HIPCK(hipMemcpyAsync(h->cat_table.p, hp, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CK(pin_release(h, slot));
  enter_table_family(h, EF_CAT, K, 1, V);
  return 0;
}
// What svihmm_set_emission_mcat and svihmm_svi_begin_mcat (`fn`) ask of K, D and the columns' symbol counts, in the
// order both have always asked it; *F_out = sum of V
static int check_mcat_shape(const char* fn, int K, int D, const int32_t* V, int* F_out) {
  const std::string p = std::string(fn) + ": ";
  if (K < 1 || K > 256) return fail(p + "K = " + std::to_string(K) + " outside [1, 256]");
  if (D < 1 || D > SVIHMM_MCAT_MAX_D)
    return fail(p + "D = " + std::to_string(D) + " outside [1, SVIHMM_MCAT_MAX_D = " + std::to_string(SVIHMM_MCAT_MAX_D) + "]");
  int64_t F = 0;
  for (int d = 0; d < D; ++d) {
    if (V[d] < 1)
      return fail(p + "V[" + std::to_string(d) + "] = " + std::to_string(V[d]) + " (every column needs at least one symbol)");
    F += V[d];
  }
  if (F > SVIHMM_MCAT_MAX_F)
    return fail(p + "F = sum of V = " + std::to_string(F) + " exceeds SVIHMM_MCAT_MAX_F = " + std::to_string(SVIHMM_MCAT_MAX_F));
  *F_out = (int)F;
  return 0;
}
// mcat_meta = [off_d D | V_d D | d(f) F | v(f) F] int32, built in a staging slot
static int upload_mcat_meta(svihmm_ctx* h, int D, int F, const int32_t* V) {
  const size_t nb = (2 * (size_t)D + 2 * (size_t)F) * sizeof(int);
  CK(ensure(h->mcat_meta, nb));
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, nb, &pin, &slot));
  int* mp = (int*)pin;
  for (int d = 0, o = 0; d < D; o += V[d], ++d) {
    mp[d] = o; mp[D + d] = V[d];
    for (int v = 0; v < V[d]; ++v) { mp[2 * D + o + v] = d; mp[2 * D + F + o + v] = v; }
  }
  HIPCK(hipMemcpyAsync(h->mcat_meta.p, pin, nb, hipMemcpyHostToDevice, h->stream));
  return pin_release(h, slot);
}
// D symbol columns, independent per state (kernels_mcat.h).  The family rides the Categorical branches of the host
// code (fam_table) with V = F features; only the lookup and the count launches differ (EF_MCAT).
int svihmm_set_emission_mcat(svihmm_ctx* h, int32_t K, int32_t D, const int32_t* V, const double* logp) {
  if (!h) return fail("svihmm_set_emission_mcat: handle is NULL");
  if (!V || !logp) return fail("svihmm_set_emission_mcat: V and logp must not be NULL");
  int F = 0;
  CK(check_mcat_shape("svihmm_set_emission_mcat", K, D, V, &F));
  const size_t n = (size_t)K * F;
  for (size_t i = 0; i < n; ++i)
    if (!finite_val(logp[i]))
      return fail("svihmm_set_emission_mcat: logp[" + std::to_string(i / F) + "][" + std::to_string(i % F) + "] is not finite");
  CK(begin_emission_upload(h, EF_MCAT, D, own_loop(h, EF_MCAT, K, D, V)));
  CK(ensure(h->cat_table, n * sizeof(double)));
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, n * sizeof(double), &pin, &slot));
  double* hp = (double*)pin;
  for (int k = 0; k < K; ++k)              // transpose to [F][K]: a feature's states are contiguous
    for (int f = 0; f < F; ++f) hp[(size_t)f * K + k] = logp[(size_t)k * F + f];
  HIPCK(hipMemcpyAsync(h->cat_table.p, hp, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CK(pin_release(h, slot));
  CK(upload_mcat_meta(h, D, F, V));
  enter_table_family(h, EF_MCAT, K, D, F);
  return 0;
}
// What svihmm_set_emission_poisson and svihmm_svi_begin_poisson (`fn`) ask of K, D, C and the logfact table, in the
// order both have always asked it; elog / erate [K][D]: the setter's tables, which it checks in front of logfact
static int check_poisson_shape(const char* fn, int K, int D, int C, const double* logfact, const double* elog = nullptr,
                               const double* erate = nullptr) {
  const std::string p = std::string(fn) + ": ";
  if (K < 1 || K > 256) return fail(p + "K = " + std::to_string(K) + " outside [1, 256]");
  if (D < 1 || D > SVIHMM_POISSON_MAX_D)
    return fail(p + "D = " + std::to_string(D) + " outside [1, SVIHMM_POISSON_MAX_D = " + std::to_string(SVIHMM_POISSON_MAX_D) + "]");
  if (C < 0 || C > SVIHMM_POISSON_MAX_COUNT)
    return fail(p + "C = " + std::to_string(C) + " outside [0, SVIHMM_POISSON_MAX_COUNT = " + std::to_string(SVIHMM_POISSON_MAX_COUNT) + "]");
  for (size_t i = 0; elog && i < (size_t)K * D; ++i) {
    const std::string at = "[" + std::to_string(i / D) + "][" + std::to_string(i % D) + "] is not finite";
    if (!finite_val(elog[i])) return fail(p + "elog" + at);
    if (!finite_val(erate[i])) return fail(p + "erate" + at);
  }
  for (int c = 0; c <= C; ++c)
    if (!finite_val(logfact[c])) return fail(p + "logfact[" + std::to_string(c) + "] is not finite");
  return 0;
}
// the logfact table changes only with C: the device copy stays while the caller's holds the same bits
static int upload_logfact(svihmm_ctx* h, const double* logfact, int C) {
  const size_t nlf = (size_t)C + 1;
  if (h->pois_lf_host.size() == nlf && std::memcmp(h->pois_lf_host.data(), logfact, nlf * sizeof(double)) == 0) return 0;
  CK(ensure(h->pois_logfact, nlf * sizeof(double)));
  h->pois_lf_host.clear();               // (stays empty if the upload below fails)
  CK(upload_blocks(h, h->pois_logfact.p, {{logfact, nlf}}));
  h->pois_lf_host.assign(logfact, logfact + nlf);
  return 0;
}
// D count columns, independent Poisson rates per state (kernels_poisson.h).  The family rides the Categorical branches
// of the host code (fam_table) with V = 2 D statistics rows [sx | n]; only the lookup and the statistics launches
// differ (EF_POIS).
int svihmm_set_emission_poisson(svihmm_ctx* h, int32_t K, int32_t D, const double* elog, const double* erate,
                                const double* logfact, int32_t C) {
  if (!h) return fail("svihmm_set_emission_poisson: handle is NULL");
  if (!elog || !erate || !logfact) return fail("svihmm_set_emission_poisson: elog, erate and logfact must not be NULL");
  CK(check_poisson_shape("svihmm_set_emission_poisson", K, D, C, logfact, elog, erate));
  CK(begin_emission_upload(h, EF_POIS, D, own_loop(h, EF_POIS, K, D), 1));
  const size_t n = (size_t)K * D;
  const size_t nt = 2 * (n + (size_t)K);     // [D + 1][K] pairs (elog, erate); row D, all +0.0, is what an absent column reads
  CK(ensure(h->cat_table, nt * sizeof(double)));
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, nt * sizeof(double), &pin, &slot));
  double* hp = (double*)pin;
  for (int k = 0; k < K; ++k) {            // transposed: a column's states are contiguous
    for (int d = 0; d < D; ++d) {
      hp[2 * ((size_t)d * K + k)] = elog[(size_t)k * D + d];
      hp[2 * ((size_t)d * K + k) + 1] = erate[(size_t)k * D + d];
    }
    hp[2 * ((size_t)D * K + k)] = hp[2 * ((size_t)D * K + k) + 1] = 0.0;
  }
  HIPCK(hipMemcpyAsync(h->cat_table.p, hp, nt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CK(pin_release(h, slot));
  CK(upload_logfact(h, logfact, C));
  h->pois_C = C;
  enter_table_family(h, EF_POIS, K, D, 2 * D);
  return 0;
}
// D real-valued columns with missing entries, independent Gaussians per state (kernels_pgauss.h).  The family rides the
// Categorical branches of the host code (fam_table) with V = 3 D statistics rows [sxx | sx | n]; only the lookup and
// the statistics launches differ (EF_PGAUSS).
int svihmm_set_emission_pgauss(svihmm_ctx* h, int32_t K, int32_t D, const double* mu, const double* hprec,
                               const double* cst, const double* origin) {
  const std::string fn = "svihmm_set_emission_pgauss: ";
  if (!h) return fail(fn + "handle is NULL");
  if (!mu || !hprec || !cst || !origin) return fail(fn + "mu, hprec, cst and origin must not be NULL");
  if (K < 1 || K > 256) return fail(fn + "K = " + std::to_string(K) + " outside [1, 256]");
  if (D < 1 || D > SVIHMM_PGAUSS_MAX_D)
    return fail(fn + "D = " + std::to_string(D) + " outside [1, SVIHMM_PGAUSS_MAX_D = " +
                std::to_string(SVIHMM_PGAUSS_MAX_D) + "]");
  auto inside =[](double v) { return v > -SVIHMM_PGAUSS_ABSENT && v < SVIHMM_PGAUSS_ABSENT; };
  const size_t n = (size_t)K * D;
  for (size_t i = 0; i < n; ++i) {
    const std::string at = "[" + std::to_string(i / D) + "][" + std::to_string(i % D) + "]";
    if (!finite_val(mu[i])) return fail(fn + "mu" + at + " is not finite");
    if (!finite_val(hprec[i])) return fail(fn + "hprec" + at + " is not finite");
    if (!finite_val(cst[i])) return fail(fn + "cst" + at + " is not finite");
    if (hprec[i] > 0.0) return fail(fn + "hprec" + at + " is positive (hprec = -0.5 alphas / betas)");
    if (!inside(mu[i])) return fail(fn + "|mu" + at + "| is at or above SVIHMM_PGAUSS_ABSENT");
  }
  for (int d = 0; d < D; ++d) {
    if (!finite_val(origin[d])) return fail(fn + "origin[" + std::to_string(d) + "] is not finite");
    if (!inside(origin[d])) return fail(fn + "|origin[" + std::to_string(d) + "]| is at or above SVIHMM_PGAUSS_ABSENT");
  }
  // (the resident SVI loop does not know this family: a running loop ends with this upload)
  CK(begin_emission_upload(h, EF_PGAUSS, D, own_loop(h, EF_PGAUSS, K, D), 2));
  const size_t nr = n + (size_t)K;           // [D + 1][K]; row D, all +0.0, is what an absent column reads
  const size_t nt = 3 * nr;                  // pairs (mu, hprec), then cst
  CK(ensure(h->cat_table, nt * sizeof(double)));
  CK(ensure(h->pg_origin, (size_t)D * sizeof(double)));
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, (nt + (size_t)D) * sizeof(double), &pin, &slot));
  double* hp = (double*)pin;
  for (int k = 0; k < K; ++k) {              // transposed: a column's states are contiguous
    for (int d = 0; d < D; ++d) {
      hp[2 * ((size_t)d * K + k)] = mu[(size_t)k * D + d];
      hp[2 * ((size_t)d * K + k) + 1] = hprec[(size_t)k * D + d];
      hp[2 * nr + (size_t)d * K + k] = cst[(size_t)k * D + d];
    }
    hp[2 * ((size_t)D * K + k)] = hp[2 * ((size_t)D * K + k) + 1] = hp[2 * nr + (size_t)D * K + k] = 0.0;
  }
  std::memcpy(hp + nt, origin, (size_t)D * sizeof(double));
  HIPCK(hipMemcpyAsync(h->cat_table.p, hp, nt * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(h->pg_origin.p, hp + nt, (size_t)D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  CK(pin_release(h, slot));
  enter_table_family(h, EF_PGAUSS, K, D, 3 * D);
  return 0;
}
int64_t svihmm_packed_len(svihmm_ctx* h) { return h ? (int64_t)packed_len(h) : 0; }

int ensure_feature_table(svihmm_ctx* h) {
  return upload_feature_table(h, h->D, h->K, h->fam == EF_DIAG);
}

int svihmm_set_lliks(svihmm_ctx* h, const double* lliks, int32_t B, int32_t Lm) {
  if (!h || !lliks || B <= 0 || Lm <= 0) return fail("svihmm_set_lliks: bad arguments");
  if (!h->have_globals) return fail("svihmm_set_lliks: call svihmm_set_globals first (K unknown)");
  CK(set_device(h));
  h->lin_stale = true;
  const size_t n = (size_t)B * Lm * h->K * sizeof(double);
  // (host-evaluated emitters do not use the factors an automatic theta rebuild may have complained about)
  CK(drop_auto_status(h));
  CK(ensure(h->ll, n));
  HIPCK(hipMemcpyAsync(h->ll.p, lliks, n, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  h->hostB = B; h->hostLm = Lm; h->have_host_ll = true;
  return 0;
}

// ---- launch helpers -----------------------------------------------------------------
// A declaration of sequences is in force (svihmm_set_sequences): every window [starts[b], starts[b] + Lm), already
// known to lie inside [0, T), must lie inside ONE of them.  `fn`: prefix of the message ("" for none).
static int check_window_sequences(const svihmm_ctx* h, const std::string& fn, const int64_t* starts, int B, int Lm) {
  if (h->seq_off.empty() || h->seq_internal) return 0;
  const std::vector<int64_t>& so = h->seq_off;
  for (int b = 0; b < B; ++b) {
    // the sequence that holds the window's first row: the last offset <= starts[b]
    const size_t s = (size_t)(std::upper_bound(so.begin(), so.end(), starts[b]) - so.begin()) - 1;
    if (starts[b] + Lm > so[s + 1])
      return fail(fn + "window " + std::to_string(b) + " (rows " + std::to_string(starts[b]) + " .. " +
                  std::to_string(starts[b] + Lm - 1) + ") holds rows of two sequences: sequence " + std::to_string(s) +
                  " ends at row " + std::to_string(so[s + 1] - 1) + " (svihmm_set_sequences)");
  }
  return 0;
}
static int check_windows(svihmm_ctx* h, const int64_t* starts, int B, int Lm, bool need_obs) {
  if (B <= 0 || Lm <= 0) return fail("bad window batch (B, Lm must be positive)");
  if (need_obs) {
    if (h->T <= 0) return fail("no observations: call svihmm_set_obs first");
    if (!starts) return fail("starts is NULL");
    for (int b = 0; b < B; ++b)
      if (starts[b] < 0 || starts[b] + Lm > h->T)
        return fail("window " + std::to_string(b) + " out of range");
    CK(check_window_sequences(h, "", starts, B, Lm));
  }
  return 0;
}

// small upload through a pinned slot, pulled by a kernel (see k_exp_transpose)
static int pull_small(svihmm_ctx* h, void* dst, const void* pin, size_t bytes) {
  const size_t n = bytes / 8;
  unsigned blocks = (unsigned)((n + 1023) / 1024);
  if (blocks > 512) blocks = 512;
  if (blocks < 1) blocks = 1;
  void* dpin = nullptr;
  HIPCK(hipHostGetDevicePointer(&dpin, const_cast<void*>(pin), 0));
  hipLaunchKernelGGL(k_pull, dim3(blocks), dim3(256), 0, h->stream, (const unsigned long long*)dpin,
                     (unsigned long long*)dst, n);
  HIPCK(hipGetLastError());
  return 0;
}

int ensure_starts_pulled(svihmm_ctx* h) {
  if (!h->starts_pending) return 0;
  void* dst = h->starts.p;
  const int64_t* src = h->starts_pending;
  h->starts_pending = nullptr;
  hipLaunchKernelGGL(k_pull, dim3(1), dim3(256), 0, h->stream, (const unsigned long long*)src,
                     (unsigned long long*)dst, (size_t)h->starts_pending_n);
  HIPCK(hipGetLastError());
  return 0;
}
static int upload_starts(svihmm_ctx* h, const int64_t* starts, int B) {
  CK(ensure(h->starts, (size_t)B * sizeof(int64_t)));
  h->starts_pending = nullptr;
  const size_t nb = (size_t)B * sizeof(int64_t);
  if (h->svi_upload_it >= 0 && nb <= (size_t)1 << 20) {
    svihmm_ctx::StartSlot& ss = h->svi_starts[h->svi_upload_it % 8];
    if (ss.used_it >= 0 && h->svi_flags && h->svi_ts && 2 * ss.used_it + 1 < h->svi_ts_cap) {
      // (eight iterations back: long complete -- its end stamp is there; bounded wait, then the stream itself)
      volatile unsigned long long* ts = &h->svi_ts[2 * ss.used_it + 1];
      int spins = 0;
      while (*ts == 0 && ++spins < 200000) { for (volatile int w = 0; w < 50; ++w) {} }
      if (*ts == 0) HIPCK(hipStreamSynchronize(h->stream));
    } else if (ss.used_it >= 0 && 2 * ss.used_it + 1 < (int)h->svi_ev.size())
      HIPCK(hipEventSynchronize(h->svi_ev[2 * ss.used_it + 1]));   // (eight iterations back: long complete)
    if (nb > ss.cap) {
      if (ss.p) hipHostFree(ss.p);
      ss.p = nullptr; ss.cap = 0;
      HIPCK(hipHostMalloc(&ss.p, nb + 4096, hipHostMallocMapped));
      ss.cap = nb + 4096;
    }
    std::memcpy(ss.p, starts, nb);
    // the pull is owed, not launched: the orbit-schedule emission kernel reads the slot itself and leaves the
    // device copy behind (launch_emission); every other consumer pays it first (ensure_starts_pulled)
    void* dpin = nullptr;
    HIPCK(hipHostGetDevicePointer(&dpin, ss.p, 0));
    h->starts_pending = (const int64_t*)dpin; h->starts_pending_n = B;
    ss.used_it = h->svi_upload_it;
  } else if (h->starts_sync_call && nb <= (size_t)1 << 20) {
    // (svihmm_estep_minibatch with a read-back: as in the SVI loop the pull is owed, not launched -- a k_pull launch
    //  and the slot's release event in front of the emission kernel are ~10 us of a 64-window step)
    if (h->starts_slot_inflight) { HIPCK(hipStreamSynchronize(h->stream)); h->starts_slot_inflight = false; }
    if (nb > h->starts_slot_cap) {
      if (h->starts_slot) hipHostFree(h->starts_slot);
      h->starts_slot = nullptr; h->starts_slot_cap = 0;
      HIPCK(hipHostMalloc(&h->starts_slot, nb + 4096, hipHostMallocMapped));
      h->starts_slot_cap = nb + 4096;
    }
    std::memcpy(h->starts_slot, starts, nb);
    void* dpin = nullptr;
    HIPCK(hipHostGetDevicePointer(&dpin, h->starts_slot, 0));
    h->starts_pending = (const int64_t*)dpin; h->starts_pending_n = B;
    h->starts_slot_inflight = true;
  } else if (nb <= (size_t)4 << 20) {   // through a pinned slot: no host-side wait for the stream
    void* pin = nullptr;
    int slot = 0;
    CK(pinned(h, nb, &pin, &slot));
    std::memcpy(pin, starts, nb);
    CK(pull_small(h, h->starts.p, pin, nb));
    CK(pin_release(h, slot));
  } else {
    HIPCK(hipMemcpyAsync(h->starts.p, starts, nb, hipMemcpyHostToDevice, h->stream));
  }
  return 0;
}



// Which sweep implementation a batch uses, as a code of the FB knob: SVIHMM_FB_WAVE wave-per-window (log domain;
// small batches, K > 64), SVIHMM_FB_LOG_MFMA log-domain MFMA (callers that want lalpha / lbeta back),
// SVIHMM_FB_SCALED scaled linear-domain MFMA (the E-step fast path; logs are materialised on demand).
static int pick_fb(const svihmm_ctx* h, int B, int Lm, bool want_logs) {
  int var = h->variant[SVIHMM_VAR_FB];
  if (h->K > 256 || h->exact_log) return SVIHMM_FB_WAVE;
  if (h->K > 64) {   // no log-domain MFMA sweep beyond 64 states: scaled (streamed B) or per-window
    if (var == SVIHMM_FB_LOG_MFMA) var = SVIHMM_FB_WAVE;
    // one long chain: blocked scan (its messages convert to logs row by row, see materialise);
    // large batches: scaled sweeps unless the logs themselves are wanted
    if (var == 0) var = (use_chain(h, B, Lm) || (B >= cu_scaled(h, 192) && !want_logs)) ? SVIHMM_FB_SCALED : SVIHMM_FB_WAVE;
    if (var == SVIHMM_FB_SCALED && !use_chain(h, B, Lm) && (size_t)16 * Lm * h->K * sizeof(double) >= ((size_t)1 << 32))
      var = SVIHMM_FB_WAVE;
    return var;
  }
  // no logs wanted: scaled sweeps at any batch size; logs of one long chain: blocked scan + conversion
  if (var == 0)
    var = want_logs ? (use_chain(h, B, Lm) ? SVIHMM_FB_SCALED : B >= cu_scaled(h, 192) ? SVIHMM_FB_LOG_MFMA : SVIHMM_FB_WAVE)
                    : SVIHMM_FB_SCALED;
  // the scaled sweeps address a workgroup's 16 windows with 32-bit byte offsets
  // (the wave-per-window kernel of small batches uses 64-bit row offsets)
  if (var == SVIHMM_FB_SCALED && !use_chain(h, B, Lm) &&
      !(B < lin_wave_max(h) && h->variant[SVIHMM_VAR_SWEEP_FAMILY] != SVIHMM_SWEEP_FAMILY_TILES) &&
      (size_t)16 * Lm * h->K * sizeof(double) >= ((size_t)1 << 32))
    var = SVIHMM_FB_LOG_MFMA;
  return var;
}

// messages + posterior for a window batch (mode from pick_fb, fixed before the emission ran)
// the SVI loop's globals kernel runs on a side stream: everything that reads Aexp / mod_init /
// var_init on the main stream waits for it here (no-op otherwise)
int wait_globals(svihmm_ctx* h) {
  if (h->globals_ev) {
    HIPCK(hipStreamWaitEvent(h->stream, h->globals_ev, 0));
    h->globals_ev = nullptr;
  }
  return 0;
}
// The SVI loop's side streams may still read what a host upload is about to rewrite: the ELBO
// kernels (stream3) read niw / theta / logdet / var_tran, the globals kernel (stream2) var_tran.
static int wait_side_streams(svihmm_ctx* h) {
  // (flags mode, inside the loop's E-step: the sweeps gate on the globals counter -- or take the event themselves,
  //  launch_fb_lin_range -- and the global step gates on the ELBO kernels' counter)
  if (h->svi_flags && h->in_svi_estep) return 0;
  CK(svi_flush_elbo(h));
  CK(wait_globals(h));
  return wait_vlb(h);
}
static int run_fb(svihmm_ctx* h, int B, int Lm, int var, bool want_lb, bool total) {
  h->m_nb = 0;
  // the sweeps need the globals kernel of the SVI loop's side stream; the loop's other cross-stream
  // wait (the previous iteration's ELBO kernels, before the global step rewrites what they read) is
  // taken at the same place: every stream-order event between two kernels of the iteration's chain
  // costs a few microseconds of dispatch, two in a row less than two apart
  CK(wait_side_streams(h));
  if (var == SVIHMM_FB_SCALED) {
    h->have_lb = true;   // materialised lazily
    return launch_fb_lin(h, B, Lm, total);
  }
  h->have_lb = (var != SVIHMM_FB_LOG_MFMA) || want_lb;
  if (h->svi_flags && h->in_svi_estep) CK(wait_globals(h));    // (the log-domain kernels take no gate)
  if (var == SVIHMM_FB_LOG_MFMA) return launch_fb_fused(h, B, Lm, want_lb, total);
  CK(launch_fb(h, B, Lm, 0, 2));
  return launch_posterior(h, B, Lm, total);
}


int d2h(svihmm_ctx* h, void* dst, const void* src, size_t bytes) {
  ProfScope ps(h, KS_D2H);
  HIPCK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, h->stream));
  return 0;
}
// small result readback: DMA into a pinned slot queued right behind the producing kernel,
// one stream synchronisation, host copy to the caller's (pageable) buffer.  A direct async
// copy to pageable memory makes the runtime wait for the stream on the host first (~0.1 ms
// of GPU idle per E-step in the kernel trace).
static int d2h_sync_small(svihmm_ctx* h, void* dst, const void* src, size_t bytes) {
  void* pin = nullptr;
  int slot = 0;
  CK(pinned(h, bytes, &pin, &slot));
  {
    ProfScope ps(h, KS_D2H);
    HIPCK(hipMemcpyAsync(pin, src, bytes, hipMemcpyDeviceToHost, h->stream));
  }
  HIPCK(hipStreamSynchronize(h->stream));
  std::memcpy(dst, pin, bytes);
  return 0;
}

int64_t svihmm_packed_size(int32_t K, int32_t D) {
  return (int64_t)K * K + (int64_t)K * D + K + (int64_t)K * D * D + 1;
}


// Step-major message layout (kernels_msg_layout.h): exactly the batches whose sweeps are k_sweeps_lin<4, true, 0> on
// double messages behind the row-tile orbit emission kernel -- the tiled fp64 epoch at K = 64.  Thresholds, from the
// dispatch: B >= lin_wave_max (4 CUs' worth of windows + 1: below it the wave-per-window / fused kernels run) and at
// least one 128-row emission workgroup per CU.  Everything else keeps row-major; SVIHMM_MSG_LAYOUT_ROW_MAJOR forces
// row-major here
// too (A/B runs, the bit-identity test).  (B + 18) Lm K < 2^31: the statistics GEMM's 32-bit message offsets.
bool step_major_ok(const svihmm_ctx* h, int B, int Lm, uint32_t flags, bool lin) {
  if (!lin || h->variant[SVIHMM_VAR_MSG_LAYOUT] == SVIHMM_MSG_LAYOUT_ROW_MAJOR || h->K != 64 || h->Kp != 64) return false;
  if ((flags & SVIHMM_USE_HOST_LLIKS) || fam_table(h->fam) || (h->prec == 1 && h->f32_ok)) return false;
  if (use_chain(h, B, Lm) || B < lin_wave_max(h)) return false;
  if ((int64_t)(B + 18) * Lm * h->K >= ((int64_t)1 << 31)) return false;
  return emission_row_tile_orbit(h, (int64_t)B * Lm);
}

// lin: the batch goes through the scaled linear-domain sweeps (pick_fb == SVIHMM_FB_SCALED)
int prepare_ll(svihmm_ctx* h, const int64_t* starts, int B, int Lm, uint32_t flags,
                      bool need_obs_for_stats, bool lin) {
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  const bool host_ll = flags & SVIHMM_USE_HOST_LLIKS;
  if (!host_ll) CK(check_clamp_fit(h));
  CK(check_windows(h, starts, B, Lm, !host_ll || need_obs_for_stats));
  if (starts) CK(upload_starts(h, starts, B));
  h->f32_report_hold = -1;
  h->cur_f32 = false;
  h->eh_float = false;
  h->step_major = false;
  h->seq_result = false;
  h->dec_result = 0;
  h->post_kind = 0;
  if (host_ll) {
    if (!h->have_host_ll || h->hostB != B || h->hostLm != Lm)
      return fail("SVIHMM_USE_HOST_LLIKS: no uploaded lliks of shape [B,Lm,K]");
    if (lin) CK(launch_scale_ll(h, B, Lm));
  } else {
    // K <= 64: the emission kernel owns whole rows and writes (Eh, kexp) itself; wider
    // models take the plain kernel plus one scaling pass
    // (a labelled batch -- svihmm_set_labels -- or one under allowed-state sets -- svihmm_set_state_sets -- as well: the
    //  clamp follows the plain kernel, there is no scaled output under a clamp; such a batch runs in fp64 and in the
    //  row-major layout)
    const bool labelled = clamp_in_force(h);
    const bool two_pass = lin && (h->Kp > 64 || fam_table(h->fam) || labelled);
    // fp32 mode: scaled messages stored as float + fp32 statistics GEMM, for what the mode
    // covers (NIW emission, K <= 64, window batches on the scaled sweeps; round 5: wide NIW models
    // up to K = 256, D = 64 in large batches, f32_wide_ok); everything else runs as fp64
    const bool wide32 = two_pass && !labelled && lin && h->prec == 1 && h->f32_ok && !use_chain(h, B, Lm) &&
                        f32_wide_ok(h, (int64_t)B * Lm);
    h->cur_f32 = lin && h->prec == 1 && h->f32_ok && (!two_pass || wide32) && !use_chain(h, B, Lm);
    h->step_major = !two_pass && !h->cur_f32 && step_major_ok(h, B, Lm, flags, lin);
    h->curB = B;
    CK(launch_emission(h, B, Lm, flags, lin && !two_pass));
    if (h->cur_f32 && !two_pass && h->f32_fused_req) {     // (float Eh is written; from here on the batch is an fp64 one)
      h->eh_float = true;
      h->cur_f32 = false;
    }
    // wide models: plain log-likelihoods + one scaling pass (fp32 mode: float, in place in h->ll, first rows
    // of the windows in h->ll0 -- the layout of the K <= 64 path, so eh_in_llE stays false)
    if (wide32) CK(launch_scale_ll_f32(h, B, Lm));
    else if (two_pass) CK(launch_scale_ll(h, B, Lm));
    h->have_host_ll = false;
  }
  h->eh_in_llE = lin && (host_ll || (h->Kp > 64 && !h->cur_f32) || fam_table(h->fam) || clamp_in_force(h));
  h->lin_mode = lin;
  h->lin_stale = false;
  h->q_valid = false;
  h->curB = B;
  h->last_host_ll = host_ll;
  h->last_flags = flags;
  h->m_nb = 0;
  return 0;
}

// device pointer of row `row0` of intermediate `what` (0 lliks, 1 lalpha, 2 lbeta, 3 var_x)
static int intermediate_ptr(svihmm_ctx* h, int what, int64_t row0, int64_t nrows, const double** out) {
  const int K = h->K, Lm = h->lastLm;
  Buf* src[] = {&h->ll, &h->la, &h->lb, &h->q};
  if (h->seq_result && h->seq_subset && what != 3)
    return fail("lliks / lalpha / lbeta are not available: svihmm_estep_sequence_subset keeps var_x of the listed "
                "rows only (what = 3); svihmm_forward_backward on a sequence's window returns its messages");
  if (h->seq_result && what != 3)
    return fail("lliks / lalpha / lbeta are not available: svihmm_estep_sequences keeps var_x only (what = 3); "
                "svihmm_forward_backward on a sequence's window returns its messages");
  if (h->dec_result && what != 0)
    return fail(std::string("lalpha / lbeta / var_x are not available: ") +
                (h->dec_result == 1 ? "svihmm_viterbi_sequences" : "svihmm_ffbs_sequences") +
                " keeps the lliks of all T rows only (what = 0)" +
                (h->dec_result == 2 ? "; lalpha is handed out through out_lalpha" : ""));
  if (!h->lin_mode || what == 3 || (what == 0 && h->eh_in_llE)) {
    if (what == 3) CK(ensure_q(h, h->lastB, Lm, h->stream));
    if (what == 2 && !h->have_lb) {
      // the fused log-domain backward sweep kept lbeta in registers (no SVIHMM_KEEP_LBETA):
      // one more backward sweep over the lliks still held, as long as they are current
      if (h->lin_stale)
        return fail("lbeta was not kept (SVIHMM_KEEP_LBETA) and the observations / globals / emission "
                    "parameters have changed since: read it before the next parameter upload");
      CK(wait_globals(h));
      CK(launch_fb(h, h->lastB, Lm, 1, 1));
      h->have_lb = true;
    }
    if (!src[what]->p) return fail("intermediate buffer not available");
    *out = (const double*)src[what]->p + (size_t)row0 * K;
    return 0;
  }
  const int b0 = (int)(row0 / Lm), b1 = (int)((row0 + nrows - 1) / Lm) + 1;
  CK(materialise(h, b0, b1 - b0));
  Buf* ms[] = {&h->m_ll, &h->m_la, &h->m_lb};
  *out = (const double*)ms[what]->p + ((size_t)row0 - (size_t)h->m_b0 * Lm) * K;
  return 0;
}

// copy `packed` into the host-visible mirror on the handle's stream
static int launch_mirror(svihmm_ctx* h) {
  const size_t n = (size_t)packed_len(h);
  if (n * sizeof(double) > h->mirror_cap) {
    if (h->mirror) hipHostFree(h->mirror);
    h->mirror = nullptr; h->mirror_cap = 0;
    HIPCK(hipHostMalloc((void**)&h->mirror, n * sizeof(double) + 256, hipHostMallocMapped));
    h->mirror_cap = n * sizeof(double) + 256;
  }
  double* dev = nullptr;
  HIPCK(hipHostGetDevicePointer((void**)&dev, h->mirror, 0));
  ProfScope ps(h, KS_D2H);
  if (h->shifted && fam_gaussian(h->fam))      // statistics leave in the caller's coordinates
    hipLaunchKernelGGL(k_packed_shift, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)h->packed.p, dev, (int)n, h->K, h->D, (const double*)h->shift_d.p, 1.0, h->fam == EF_DIAG ? 1 : 0);
  else
    hipLaunchKernelGGL(k_mirror, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                       (const double*)h->packed.p, dev, (int)n);
  HIPCK(hipGetLastError());
  h->mirror_valid = true;
  return 0;
}
static int read_packed_host(svihmm_ctx* h, double* out) {
  const size_t nb = (size_t)packed_len(h) * sizeof(double);
  if (!h->mirror_valid) CK(launch_mirror(h));
  HIPCK(hipStreamSynchronize(h->stream));
  std::memcpy(out, h->mirror, nb);
  return 0;
}
// Sum of the packed statistics over the ranks.  The buffer holds centred coordinates and every
// rank has its own shift: the sum is formed in the callers' common coordinates and brought back.
// packed_to_common: the statistics in the coordinates every rank shares (the callers'), as a device
// buffer (commtmp; `packed` itself where no shift applies); packed_from_common: the reduced buffer
// back into this handle's centred coordinates.  The RCCL all-reduce and the host-mediated exchange
// (svihmm_export_packed / svihmm_import_packed) run between the same two halves.
static bool common_needs_shift(const svihmm_ctx* h, bool always) {
  // (the knob: rehearsal at one rank)
  return h->shifted && fam_gaussian(h->fam) &&
         (always || h->nranks > 1 || h->variant[SVIHMM_VAR_ALLREDUCE_COORDS] == SVIHMM_ALLREDUCE_COORDS_ON);
}
static int packed_to_common(svihmm_ctx* h, bool always, double** buf_out) {
  const size_t n = (size_t)packed_len(h);
  if (!common_needs_shift(h, always)) { *buf_out = (double*)h->packed.p; return 0; }
  CK(ensure(h->commtmp, n * sizeof(double)));
  double* tmp = (double*)h->commtmp.p;
  hipLaunchKernelGGL(k_packed_shift, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                     (const double*)h->packed.p, tmp, (int)n, h->K, h->D, (const double*)h->shift_d.p, 1.0,
                     h->fam == EF_DIAG ? 1 : 0);
  HIPCK(hipGetLastError());
  *buf_out = tmp;
  return 0;
}
static int packed_from_common(svihmm_ctx* h, const double* buf) {
  if (buf == (const double*)h->packed.p) return 0;
  const size_t n = (size_t)packed_len(h);
  hipLaunchKernelGGL(k_packed_shift, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream, buf,
                     (double*)h->packed.p, (int)n, h->K, h->D, (const double*)h->shift_d.p, -1.0,
                     h->fam == EF_DIAG ? 1 : 0);
  HIPCK(hipGetLastError());
  return 0;
}
static int allreduce_packed_dev(svihmm_ctx* h) {
  double* buf = nullptr;
  CK(packed_to_common(h, false, &buf));
  NCCLCK(ncclAllReduce(buf, buf, (size_t)packed_len(h), ncclDouble, ncclSum, h->comm, h->stream));
  return packed_from_common(h, buf);
}

// ---- two-stream E-step pipeline -------------------------------------------------------------
// The scaled sweeps are latency-bound (one 4-wave workgroup per 16 windows, a serial chain
// of Lm steps that keeps the matrix pipe ~45 % busy) while emission and statistics are
// throughput-bound GEMMs.  For large batches the windows are split in two halves:
//   stream A:  emission(h1)  emission(h2)        statistics(h1)  statistics(h2)  finalize
//   stream B:               sweeps(h1)      sweeps(h2)
// so that the sweeps of one half share the CUs with a GEMM of the other half.  The emission
// kernel's LDS request is padded so that three of its workgroups plus one sweep workgroup fit
// a CU; the sweep kernels raise their wave priority.  Partials stay deterministic (fixed
// chunking per half, one finalize over all slots).
static bool use_pipeline(const svihmm_ctx* h, int B, int Lm, int fbvar, uint32_t flags) {
  const int v = h->variant[SVIHMM_VAR_PIPELINE];
  if (v == SVIHMM_PIPELINE_UNFUSED || fbvar != SVIHMM_FB_SCALED || (flags & SVIHMM_USE_HOST_LLIKS)) return false;
  if (h->Kp > 64 || h->D > 64 || fam_table(h->fam) || clamp_in_force(h)) return false;
  const int sv = h->variant[SVIHMM_VAR_STATS];
  if (sv != 0 && sv != SVIHMM_STATS_PIPELINED) return false;
  // opt-in only: on MI355X the sweeps' fp64 VALU work queues behind the GEMMs' MFMAs on a
  // shared SIMD and both sides lose more than the overlap wins (experiments)
  return v == SVIHMM_PIPELINE_TWO_STREAM && B >= 32;
}
static int estep_pipelined(svihmm_ctx* h, const int64_t* starts, int B, int Lm, int inner_off,
                           int inner_len, uint32_t flags) {
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  CK(check_windows(h, starts, B, Lm, true));
  CK(upload_starts(h, starts, B));
  if (!h->have_emission) return fail("no emission parameters: call svihmm_set_emission_niw");
  if (h->eD != h->D) return fail(emission_d_message(h));
  if (h->eK != h->K) return fail("emission K does not match globals K");
  if (!h->stream2) {
    HIPCK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
    for (int i = 0; i < 2; ++i) {
      HIPCK(hipEventCreateWithFlags(&h->ev_em[i], hipEventDisableTiming));
      HIPCK(hipEventCreateWithFlags(&h->ev_sw[i], hipEventDisableTiming));
    }
  }
  const int K = h->K;
  const int64_t n = (int64_t)B * Lm;
  // all buffers first: ensure() may reallocate
  CK(ensure(h->ll, (size_t)n * K * sizeof(double)));
  CK(ensure(h->kexp, (size_t)n * sizeof(double)));
  CK(ensure(h->ll0, (size_t)B * K * sizeof(double)));
  CK(ensure_fb_lin(h, B, Lm));
  int b0[2], nb[2];
  b0[0] = 0; nb[0] = ((B / 2 + 15) / 16) * 16; b0[1] = nb[0]; nb[1] = B - nb[0];
  StatsPlan plan[2] = {stats_plan(h, (int64_t)nb[0] * inner_len), stats_plan(h, (int64_t)nb[1] * inner_len)};
  CK(ensure_stats(h, plan[0].nchunk + plan[1].nchunk));
  h->have_host_ll = false;
  h->lin_mode = true; h->lin_stale = false; h->last_host_ll = false; h->eh_in_llE = false; h->last_flags = flags;
  h->cur_f32 = false; h->step_major = false; h->seq_result = false; h->dec_result = 0; h->post_kind = 0;
  h->q_valid = false; h->curB = B;
  h->m_nb = 0; h->have_lb = true;
  hipStream_t A = h->stream, Bs = h->stream2;
  // stream B must not start before earlier work of stream A (parameter uploads) is done
  HIPCK(hipEventRecord(h->ev_sw[1], A));
  HIPCK(hipStreamWaitEvent(Bs, h->ev_sw[1], 0));
  const size_t em_lds = 41 * 1024;   // 3 emission workgroups + 1 sweep workgroup per CU
  for (int c = 0; c < 2; ++c) {
    const size_t ro = (size_t)b0[c] * Lm;
    CK(launch_emission(h, nb[c], Lm, flags, true, (const int64_t*)h->starts.p + b0[c],
                       (double*)h->ll.p + ro * K, (double*)h->kexp.p + ro, A, em_lds,
                       (double*)h->ll0.p + (size_t)b0[c] * K));
    HIPCK(hipEventRecord(h->ev_em[c], A));
    HIPCK(hipStreamWaitEvent(Bs, h->ev_em[c], 0));
    CK(launch_fb_lin_range(h, b0[c], nb[c], Lm, Bs));
    HIPCK(hipEventRecord(h->ev_sw[c], Bs));
  }
  for (int c = 0; c < 2; ++c) {
    HIPCK(hipStreamWaitEvent(A, h->ev_sw[c], 0));
    CK(launch_stats_range(h, b0[c], nb[c], Lm, inner_off, inner_len, flags, plan[c],
                          c == 0 ? 0 : plan[0].nchunk, A));
  }
  CK(launch_stats_finalize(h, plan[0].nchunk + plan[1].nchunk, A));
  CK(launch_sum_lb(h, B, A));
  return 0;
}

int svihmm_loglik(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                  double* out_lliks) {
  if (!h || !out_lliks) return fail("svihmm_loglik: bad arguments");
  CK(set_device(h));
  CK(prepare_ll(h, starts, B, Lm, flags & ~SVIHMM_USE_HOST_LLIKS, false));
  CK(d2h(h, out_lliks, h->ll.p, (size_t)B * Lm * h->K * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  h->lastB = B; h->lastLm = Lm;
  return 0;
}

int svihmm_forward_backward(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm,
                            uint32_t flags, double* out_lalpha, double* out_lbeta,
                            double* out_var_x, double* out_local_lb) {
  if (!h) return fail("svihmm_forward_backward: NULL handle");
  CK(set_device(h));
  const int var = pick_fb(h, B, Lm, out_lalpha != nullptr || out_lbeta != nullptr);
  CK(prepare_ll(h, starts, B, Lm, flags, false, var == SVIHMM_FB_SCALED));
  CK(run_fb(h, B, Lm, var, out_lbeta != nullptr, false));
  h->lastB = B; h->lastLm = Lm;
  if (var == SVIHMM_FB_SCALED && (out_lalpha || out_lbeta)) CK(materialise(h, 0, B));   // forced variant
  if (var == SVIHMM_FB_SCALED && out_var_x) CK(ensure_q(h, B, Lm, h->stream));
  const size_t n = (size_t)B * Lm * h->K * sizeof(double);
  if (out_lalpha) CK(d2h(h, out_lalpha, var == SVIHMM_FB_SCALED ? h->m_la.p : h->la.p, n));
  if (out_lbeta) CK(d2h(h, out_lbeta, var == SVIHMM_FB_SCALED ? h->m_lb.p : h->lb.p, n));
  if (out_var_x) CK(d2h(h, out_var_x, h->q.p, n));
  if (out_local_lb) CK(d2h(h, out_local_lb, h->local_lb.p, (size_t)B * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  h->lastB = B; h->lastLm = Lm;
  note_posterior_batch(h, 1);
  return 0;
}

int svihmm_pred_logprob(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm,
                        uint32_t flags, double out2[2]) {
  if (!h || !starts || !out2) return fail("svihmm_pred_logprob: bad arguments");
  if (flags & SVIHMM_USE_HOST_LLIKS) return fail("svihmm_pred_logprob: NIW emission only");
  if (h->have_labels)
    return fail("svihmm_pred_logprob: labels are in force (svihmm_set_labels) and this call does not take them; "
                "svihmm_heldout_rows scores masked rows against a labelled E-step's posteriors");
  if (h->have_sets)
    return fail("svihmm_pred_logprob: allowed-state sets are in force (svihmm_set_state_sets) and this call does not "
                "take them; svihmm_heldout_rows scores masked rows against a constrained E-step's posteriors");
  if (h->have_emission && FAM_TRAITS[h->fam].noun)
    return fail(std::string("svihmm_pred_logprob: NIW emission only (") + FAM_TRAITS[h->fam].noun + " of " +
                FAM_TRAITS[h->fam].setter + " is not taken)");
  CK(set_device(h));
  if (!h->have_mask) { out2[0] = NAN; out2[1] = 0.0; return 0; }
  const int var = pick_fb(h, B, Lm, false);
  CK(prepare_ll(h, starts, B, Lm, flags, false, var == SVIHMM_FB_SCALED));
  CK(run_fb(h, B, Lm, var, false, false));
  h->lastB = B; h->lastLm = Lm;
  CK(ensure_q(h, B, Lm, h->stream));
  // emission term on the true observations (no masking), into the side buffer
  const int K = h->K;
  const int64_t n = (int64_t)B * Lm;
  CK(ensure(h->m_ll, (size_t)n * K * sizeof(double)));
  h->m_nb = 0;
  CK(launch_emission(h, B, Lm, flags & ~(uint32_t)SVIHMM_MASK_AS_NAN, false, nullptr, (double*)h->m_ll.p, nullptr, nullptr,
                     0, nullptr, false));
  const int nblk = (int)((n + PRED_ROWS_PER_BLOCK - 1) / PRED_ROWS_PER_BLOCK);
  CK(ensure(h->scratch, ((size_t)2 * nblk + 2) * sizeof(double)));
  double* part = (double*)h->scratch.p;
  {
    ProfScope ps(h, KS_MISC);
#define PL(KT) hipLaunchKernelGGL(k_pred_logprob<KT>, dim3(nblk), dim3(256), 0, h->stream, (const double*)h->q.p, \
                                  (const double*)h->m_ll.p, (const uint8_t*)h->mask.p,                            \
                                  (const int64_t*)h->starts.p, n, Lm, K, part)
    if (K <= 16) PL(1); else if (K <= 32) PL(2); else if (K <= 48) PL(3); else if (K <= 64) PL(4);
    else if (K <= 128) PL(8); else if (K <= 256) PL(16);
    else return fail("svihmm_pred_logprob: K > 256 not supported");
#undef PL
    hipLaunchKernelGGL(k_pred_final, dim3(1), dim3(64), 0, h->stream, (const double*)part, nblk, part + 2 * nblk);
    HIPCK(hipGetLastError());
  }
  CK(d2h(h, out2, part + 2 * nblk, 2 * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  return 0;
}

// emission -> sweeps -> statistics of a window batch into h->packed (B >= 1), asynchronous
static int estep_core(svihmm_ctx* h, const int64_t* starts, int B, int Lm, int inner_off, int inner_len,
                      uint32_t flags) {
  if (inner_off < 0 || inner_len <= 0 || inner_off + inner_len > Lm)
    return fail("svihmm_estep_minibatch_ex: inner segment out of range");
  const int var = pick_fb(h, B, Lm, false);
  if (use_pipeline(h, B, Lm, var, flags)) {
    CK(estep_pipelined(h, starts, B, Lm, inner_off, inner_len, flags));
  } else {
    // (the fused launch below can compute the emission tiles itself: launch_emission then does everything but launch)
    h->em_def.active = false;
    h->em_defer_req = var == SVIHMM_FB_SCALED && sweep_emission_ok(h, B, Lm, inner_off, inner_len, flags);
    h->f32_fused_req = var == SVIHMM_FB_SCALED && sweep_mixed_ok(h, B, Lm, inner_off, inner_len, flags);
    const int prc = prepare_ll(h, starts, B, Lm, flags, true, var == SVIHMM_FB_SCALED);
    h->em_defer_req = false;
    h->f32_fused_req = false;
    if (prc) { h->em_def.active = false; return prc; }
    const bool fused = var == SVIHMM_FB_SCALED && sweep_stats_ok(h, B, Lm, inner_off, inner_len, flags);
    if (h->eh_float && !fused) return fail("internal: float emission rows without the fused launch that reads them");
    if (!fused) CK(launch_emission_deferred(h));
    if (fused) {
      // minibatch-sized batches of the five-tile shapes: sweeps and statistics in one launch, the statistics'
      // stages behind the sweeps' published progress (tu_fused.hip)
      CK(wait_side_streams(h));
      CK(launch_sweep_stats(h, B, Lm, inner_off, inner_len, flags));
    } else {
      CK(run_fb(h, B, Lm, var, (flags & SVIHMM_KEEP_LBETA) != 0, true));
      CK(launch_stats(h, B, Lm, inner_off, inner_len, flags));
    }
    CK(flush_lb(h, h->stream));   // no-op when k_finalize carried the ELBO total
  }
  h->have_packed = true;
  h->mirror_valid = false;
  h->lastB = B; h->lastLm = Lm;
  note_posterior_batch(h, 1);
  return 0;
}

int svihmm_estep_minibatch(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm,
                           uint32_t flags, double* out_packed) {
  return svihmm_estep_minibatch_ex(h, starts, B, Lm, 0, Lm, flags, out_packed);
}

int svihmm_estep_minibatch_ex(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm,
                              int32_t inner_off, int32_t inner_len, uint32_t flags,
                              double* out_packed) {
  if (!h) return fail("svihmm_estep_minibatch: NULL handle");
  CK(set_device(h));
  if (B == 0) {  // empty shard of a multi-GPU minibatch: all-zero statistics
    if (!h->have_globals || h->D <= 0) return fail("svihmm_estep_minibatch: set obs/globals first");
    const size_t nb = (size_t)packed_len(h) * sizeof(double);
    CK(ensure(h->packed, nb));
    HIPCK(hipMemsetAsync(h->packed.p, 0, nb, h->stream));
    h->have_packed = true;
    h->mirror_valid = false;
    if (out_packed) {
      CK(d2h(h, out_packed, h->packed.p, nb));
      HIPCK(hipStreamSynchronize(h->stream));
    }
    return 0;
  }
  // (SVIHMM_CENTRING_PULL_STARTS: the k_pull route)
  h->starts_sync_call = out_packed != nullptr && h->variant[SVIHMM_VAR_CENTRING] != SVIHMM_CENTRING_PULL_STARTS;
  const int rc = estep_core(h, starts, B, Lm, inner_off, inner_len, flags);
  h->starts_sync_call = false;
  if (rc) return rc;
  CK(launch_mirror(h));
  if (out_packed) {
    CK(read_packed_host(h, out_packed));
    h->starts_slot_inflight = false;      // (the stream is idle: the slot's readers are done)
    CK(check_emission_status(h));
  }
  return 0;
}

// ---- a9 on posteriors the caller supplies (svihmm_suffstats) ---------------------------------
// host -> device through the pinned staging ring in pieces of 4 MB: the DMA of one piece runs while the host
// copies the next into another slot (a pageable source would make the runtime stage it synchronously itself)
static int upload_staged(svihmm_ctx* h, void* dst, const void* src, size_t bytes) {
  const size_t piece = (size_t)4 << 20;
  for (size_t o = 0; o < bytes; o += piece) {
    const size_t nb = bytes - o < piece ? bytes - o : piece;
    void* pin = nullptr;
    int slot = 0;
    CK(pinned(h, nb, &pin, &slot));
    std::memcpy(pin, (const char*)src + o, nb);
    {
      ProfScope ps(h, KS_H2D);
      HIPCK(hipMemcpyAsync((char*)dst + o, pin, nb, hipMemcpyHostToDevice, h->stream));
    }
    CK(pin_release(h, slot));
  }
  return 0;
}

// ---- argument checks of the entry points that take windows of the resident observations ------
// (svihmm_suffstats, svihmm_viterbi, svihmm_ffbs_windows; `fn`: the entry point's name.  Host work only: every one of
//  them is through with these before its first device call.  The older entry points keep check_windows / prepare_ll.)
// the model side: observations and an emission family of the globals' K and the observations' D
static int check_window_model(const svihmm_ctx* h, const char* fn) {
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (h->T <= 0 || !h->obs.p) return bad("no observations: call svihmm_set_obs first");
  if (!h->have_emission) return bad("no emission family: call svihmm_set_emission_niw / _diag / _cat first");
  if (h->K != h->eK)
    return bad("K of the globals (" + std::to_string(h->K) + ") differs from the emission family's K (" +
               std::to_string(h->eK) + ")");
  if (h->eD != h->D) return bad(emission_d_message(h));
  return 0;
}
// every window [starts[b], starts[b] + Lm) inside [0, T)
static int check_window_range(const svihmm_ctx* h, const char* fn, const int64_t* starts, int B, int Lm) {
  for (int b = 0; b < B; ++b)
    if (starts[b] < 0 || starts[b] + Lm > h->T)
      return fail(std::string(fn) + ": window " + std::to_string(b) + " reaches outside [0, T)");
  return check_window_sequences(h, std::string(fn) + ": ", starts, B, Lm);
}
// a decoder's window batch (B, Lm positive): host lliks of exactly its shape, or the model side and the windows
static int check_window_call(const svihmm_ctx* h, const char* fn, const int64_t* starts, int B, int Lm, uint32_t flags) {
  if (flags & SVIHMM_USE_HOST_LLIKS) {
    if (!h->have_host_ll || h->hostB != B || h->hostLm != Lm)
      return fail(std::string(fn) + ": SVIHMM_USE_HOST_LLIKS without uploaded lliks of shape [B, Lm, K] (svihmm_set_lliks)");
    return 0;
  }
  CK(check_window_model(h, fn));
  if (!starts) return fail(std::string(fn) + ": starts is NULL");
  return check_window_range(h, fn, starts, B, Lm);
}

int svihmm_suffstats(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                     const double* var_x, double* out_packed) {
  if (!h) return fail("svihmm_suffstats: NULL handle");
  CK(check_window_model(h, "svihmm_suffstats"));
  if (B < 1 || Lm < 1) return fail("svihmm_suffstats: B and Lm must be positive");
  if (!starts || !var_x) return fail("svihmm_suffstats: starts / var_x is NULL");
  CK(check_window_range(h, "svihmm_suffstats", starts, B, Lm));
  CK(set_device(h));
  CK(wait_side_streams(h));
  const int K = h->K;
  const size_t nq = (size_t)B * Lm * K * sizeof(double);
  // buffers of their own: the last E-step's q / starts (read back lazily: read_intermediate, state_argmax,
  // the kept last window of the SVI loop) stay as they are
  CK(ensure(h->user_q, nq));
  CK(ensure(h->user_starts, (size_t)B * sizeof(int64_t)));
  CK(upload_staged(h, h->user_starts.p, starts, (size_t)B * sizeof(int64_t)));
  CK(upload_staged(h, h->user_q.p, var_x, nq));
  // fp64 statistics whatever the precision mode: the fp32-format kernels are never planned for this batch
  // (cur_f32 is what the last E-step ran in: svihmm_get_precision reports it unchanged afterwards)
  const bool cur_f32 = h->cur_f32;
  h->cur_f32 = false;
  const int rc = launch_stats_posteriors(h, (const double*)h->user_q.p, (const int64_t*)h->user_starts.p, B, Lm,
                                         flags & SVIHMM_TRANS_WRAP);
  h->cur_f32 = cur_f32;
  if (rc) return rc;
  h->have_packed = true;
  h->mirror_valid = false;
  CK(launch_mirror(h));
  if (out_packed) CK(read_packed_host(h, out_packed));
  return 0;
}

// ---- several sequences of unequal length on one handle (include/svihmm.h) ---------------------
int svihmm_set_sequences(svihmm_ctx* h, const int64_t* seq_off, int32_t N) {
  const char* fn = "svihmm_set_sequences";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (N < 0) return bad("N must not be negative");
  if (N == 0) { h->seq_off.clear(); return 0; }
  if (h->T <= 0 || !h->obs.p) return bad("no observations: call svihmm_set_obs first");
  if (!seq_off) return bad("seq_off is NULL");
  if (seq_off[0] != 0) return bad("seq_off[0] must be 0");
  for (int s = 0; s < N; ++s)
    if (seq_off[s + 1] <= seq_off[s])
      return bad("offsets must be strictly increasing (seq_off[" + std::to_string(s + 1) + "] = " +
                 std::to_string(seq_off[s + 1]) + " after " + std::to_string(seq_off[s]) + ")");
  if (seq_off[N] != h->T)
    return bad("seq_off[N] = " + std::to_string(seq_off[N]) + " must equal T = " + std::to_string(h->T));
  CK(set_device(h));
  const size_t nb = ((size_t)N + 1) * sizeof(int64_t);
  CK(ensure(h->seq_off_d, nb));
  CK(upload_staged(h, h->seq_off_d.p, seq_off, nb));
  h->seq_off.assign(seq_off, seq_off + N + 1);
  return 0;
}

// emission -> sweeps -> statistics of all declared sequences into h->packed, h->seq_out (local_lb[N] | q0[K]) and the
// concatenated posteriors, asynchronous.  Long sequences (use_chain) one after the other through the whole-chain
// scan, which writes the handle's ll / la / lb / q from row 0: their posteriors and local_lb are copied out before
// the next starts.  All others in one ragged launch over the lliks of the smallest row range that covers them.
static int estep_sequences_core(svihmm_ctx* h, uint32_t flags, bool subset = false) {
  const int N = (int)h->seq_off.size() - 1, K = h->K;
  const int64_t T = h->T;
  const std::vector<int64_t>& so = h->seq_off;
  const uint32_t efl = flags & SVIHMM_MASK_AS_NAN;
  std::vector<int32_t> ragged, longs;
  for (int s = 0; s < N; ++s) (use_chain(h, 1, (int)(so[s + 1] - so[s])) ? longs : ragged).push_back(s);
  // longest first: the launch's tail is short (ties in ascending s)
  std::stable_sort(ragged.begin(), ragged.end(),
                   [&so](int32_t a, int32_t b) { return so[a + 1] - so[a] > so[b + 1] - so[b]; });
  CK(ensure(h->seq_q, (size_t)T * K * sizeof(double)));
  CK(ensure(h->seq_out, ((size_t)N + K) * sizeof(double)));
  double* seq_q = (double*)h->seq_q.p;
  double* seq_lb = (double*)h->seq_out.p;
  double* q0 = seq_lb + N;
  const int64_t* sod = (const int64_t*)h->seq_off_d.p;
  if (!ragged.empty()) {
    int64_t r0 = T, r1 = 0;
    for (int32_t s : ragged) { r0 = std::min(r0, so[s]); r1 = std::max(r1, so[s + 1]); }
    CK(ensure(h->seq_ord, ragged.size() * sizeof(int32_t)));
    CK(upload_staged(h, h->seq_ord.p, ragged.data(), ragged.size() * sizeof(int32_t)));
    CK(prepare_ll(h, &r0, 1, (int)(r1 - r0), efl, false, false));
    CK(launch_fb_sequences(h, (int)ragged.size(), (const int32_t*)h->seq_ord.p, sod, r0, r1 - r0,
                           (int)(so[ragged[0] + 1] - so[ragged[0]]), (const double*)h->ll.p, seq_q, seq_lb));
  }
  for (int32_t s : longs) {
    const int len = (int)(so[s + 1] - so[s]);
    CK(prepare_ll(h, &so[s], 1, len, efl, false, true));
    h->m_nb = 0;
    CK(launch_fb_lin(h, 1, len, false));
    CK(ensure_q(h, 1, len, h->stream));
    HIPCK(hipMemcpyAsync(seq_q + (size_t)so[s] * K, h->q.p, (size_t)len * K * sizeof(double), hipMemcpyDeviceToDevice,
                         h->stream));
    HIPCK(hipMemcpyAsync(seq_lb + s, h->local_lb.p, sizeof(double), hipMemcpyDeviceToDevice, h->stream));
  }
  // statistics: the concatenated posteriors as ONE window of T rows without wrap, then the N boundaries
  CK(ensure(h->user_starts, sizeof(int64_t)));
  HIPCK(hipMemsetAsync(h->user_starts.p, 0, sizeof(int64_t), h->stream));
  CK(launch_stats_posteriors(h, seq_q, (const int64_t*)h->user_starts.p, 1, (int)T, 0));
  CK(launch_seq_finish(h, N, sod, (flags & SVIHMM_TRANS_WRAP) != 0, seq_q, seq_lb, q0));
  // what is readable afterwards: var_x of all T rows as one [1, T, K] batch
  std::swap(h->q, h->seq_q);
  h->lin_mode = false; h->q_valid = true; h->lin_stale = true; h->m_nb = 0; h->have_lb = false;
  h->lastB = 1; h->lastLm = (int)T;
  h->seq_result = true;
  h->seq_subset = subset;
  h->last_host_ll = false;
  note_posterior_batch(h, subset ? 3 : 2);
  return 0;
}

// estep_sequences_core always in fp64, the precision mode's report about the last E-step batch held (as
// svihmm_grow_windows), then the packed result's host-visible mirror
static int estep_sequences_fp64(svihmm_ctx* h, uint32_t flags, bool subset, bool mirror = true) {
  int rc;
  {
    ReportHold hold(h, true, true);
    rc = estep_sequences_core(h, flags, subset);
  }
  h->cur_f32 = false; h->eh_float = false;
  if (rc) return rc;
  h->have_packed = true;
  h->mirror_valid = false;
  // (the resident SVI loop reads nothing back: svihmm_read_packed fills the mirror when somebody asks)
  return mirror ? launch_mirror(h) : 0;
}

// What svihmm_estep_sequences and svihmm_estep_sequence_subset share, found before any device work:
// what can be wrong with the model ...
static int check_estep_sequences(const svihmm_ctx* h, const char* fn, uint32_t flags) {
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (flags & SVIHMM_USE_HOST_LLIKS) return bad("SVIHMM_USE_HOST_LLIKS is not supported (host lliks carry no sequence offsets)");
  if (!h->have_globals) return bad("no globals: call svihmm_set_globals first");
  CK(check_window_model(h, fn));
  if (h->K > 256) return bad("K = " + std::to_string(h->K) + " > 256 not supported");
  return 0;
}
// ... the statistics pass addressing the call's R rows as one window (launch_stats_posteriors' limit; `rows`: their
// name in the message) ...
static int check_stats_rows(const svihmm_ctx* h, const char* fn, int64_t R, const std::string& rows) {
  const int64_t rpc = fam_table(h->fam) ? 0 : stats_plan(h, R, h->variant[SVIHMM_VAR_STATS_CHUNKS]).rpc;
  if (R > 0x7fffffff || (R + rpc) * (int64_t)(fam_table(h->fam) ? 1 : h->Kp) >= ((int64_t)1 << 31))
    return fail(std::string(fn) + ": " + rows + " are too many for the statistics GEMM's 32-bit row offsets");
  return 0;
}
// ... and the results of the M sequences the E-step ran over
static int read_estep_sequences(svihmm_ctx* h, int M, double* out_packed, double* out_seq_lb, double* out_q0) {
  if (out_seq_lb) CK(d2h(h, out_seq_lb, h->seq_out.p, (size_t)M * sizeof(double)));
  if (out_q0) CK(d2h(h, out_q0, (const double*)h->seq_out.p + M, (size_t)h->K * sizeof(double)));
  if (out_packed) CK(read_packed_host(h, out_packed));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  return 0;
}

int svihmm_estep_sequences(svihmm_ctx* h, uint32_t flags, double* out_packed, double* out_seq_lb, double* out_q0) {
  const char* fn = "svihmm_estep_sequences";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (h->seq_off.empty()) return bad("no sequences declared: call svihmm_set_sequences first");
  CK(check_estep_sequences(h, fn, flags));
  CK(check_stats_rows(h, fn, h->T, "T = " + std::to_string(h->T) + " rows"));
  CK(set_device(h));
  CK(wait_side_streams(h));
  CK(estep_sequences_fp64(h, flags, false));
  return read_estep_sequences(h, (int)h->seq_off.size() - 1, out_packed, out_seq_lb, out_q0);
}

// ---- a minibatch of whole sequences (svihmm_estep_sequence_subset) ------------------------------
// For the call's duration the handle's resident rows ARE the gathered copy: obs / mask / T / the declaration and its
// device offsets stand for the R listed rows laid end to end, so estep_sequences_core and everything below it
// (emission, ragged sweeps / chain scan, the statistics GEMM as one window, k_seq_fix) run unchanged and touch R
// rows only.  The destructor puts the handle's own back on every return path.
struct SubsetView {
  svihmm_ctx* h; int64_t T; std::vector<int64_t> seq_off;
  SubsetView(svihmm_ctx* h_, int64_t R, std::vector<int64_t>& compact) : h(h_), T(h_->T) {
    std::swap(h->obs, h->sub_obs); std::swap(h->mask, h->sub_mask); std::swap(h->seq_off_d, h->sub_tab);
    std::swap(h->labels, h->sub_labels); std::swap(h->sets, h->sub_sets);
    seq_off.swap(h->seq_off);
    h->seq_off.swap(compact);
    h->T = R;
  }
  ~SubsetView() {
    std::swap(h->obs, h->sub_obs); std::swap(h->mask, h->sub_mask); std::swap(h->seq_off_d, h->sub_tab);
    std::swap(h->labels, h->sub_labels); std::swap(h->sets, h->sub_sets);
    h->seq_off.swap(seq_off);
    h->T = T;
  }
};

// The host half of a subset call, before any device work: the listed sequences checked, dst_off [M + 1] | src_off [M]
// (the compact copy's offsets -- its declaration -- and where each occurrence comes from), the model and the
// statistics pass's limits.  `fn`: the entry point's name in the messages.
struct SubsetPlan { std::vector<int64_t> tab; int64_t R = 0, maxlen = 0; };
static int subset_plan(const svihmm_ctx* h, const char* fn, const int32_t* idx, int32_t M, uint32_t flags, SubsetPlan& p) {
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (h->seq_off.empty()) return bad("no sequences declared: call svihmm_set_sequences first");
  if (!idx) return bad("idx is NULL");
  if (M < 1) return bad("M = " + std::to_string(M) + ": at least one sequence must be listed");
  const int N = (int)h->seq_off.size() - 1;
  const std::vector<int64_t>& so = h->seq_off;
  p.tab.assign((size_t)2 * M + 1, 0);
  int64_t R = 0, maxlen = 0;
  for (int m = 0; m < M; ++m) {
    const int32_t s = idx[m];
    if (s < 0 || s >= N)
      return bad("idx[" + std::to_string(m) + "] = " + std::to_string(s) + " is outside [0, N = " + std::to_string(N) + ")");
    p.tab[m] = R;
    p.tab[(size_t)M + 1 + m] = so[s];
    R += so[s + 1] - so[s];
    maxlen = std::max(maxlen, so[s + 1] - so[s]);
  }
  p.tab[M] = R;
  p.R = R; p.maxlen = maxlen;
  CK(check_estep_sequences(h, fn, flags));
  CK(check_stats_rows(h, fn, R, "R = " + std::to_string(R) + " listed rows"));
  return 0;
}
// The device half, enqueue only: gather, then the E-step of the compact copy into h->packed, h->seq_out
// (local_lb[M] | q0[K]) and the posteriors of the R rows.  `in_loop`: svihmm_svi_iteration_sequences -- stream order
// carries the loop's dependencies (no wait for its side stream here), and the statistics' host-visible mirror is
// left to whoever reads them.
static int subset_enqueue(svihmm_ctx* h, const SubsetPlan& p, int M, uint32_t flags, bool in_loop) {
  const int D = h->D;
  const int64_t R = p.R;
  CK(set_device(h));
  if (!in_loop) CK(wait_side_streams(h));
  // the resident copy's lazily applied state first: symbol indices go back to exact integers before they are copied
  // (the lookup kernels would do that to the rows in place; a Gaussian family's centre is the handle's, and the copy
  // holds the same centred values)
  if (fam_table(h->fam)) CK(cat_uncentre(h));
  CK(ensure(h->sub_obs, (size_t)R * D * sizeof(double)));
  if (h->have_mask) CK(ensure(h->sub_mask, (size_t)R));
  CK(ensure(h->sub_tab, p.tab.size() * sizeof(int64_t)));
  CK(upload_staged(h, h->sub_tab.p, p.tab.data(), p.tab.size() * sizeof(int64_t)));
  if (h->have_labels) CK(ensure(h->sub_labels, (size_t)R * sizeof(int32_t)));
  if (h->have_sets) CK(ensure(h->sub_sets, (size_t)R * h->sets_W * sizeof(uint64_t)));
  CK(launch_seq_gather(h, M, (const int64_t*)h->sub_tab.p, (int)p.maxlen, (double*)h->sub_obs.p, (uint8_t*)h->sub_mask.p,
                       (int32_t*)h->sub_labels.p, (uint64_t*)h->sub_sets.p));
  std::vector<int64_t> compact(p.tab.begin(), p.tab.begin() + M + 1);
  {
    SubsetView view(h, R, compact);
    CK(estep_sequences_fp64(h, flags, true, !in_loop));
  }
  return 0;
}

int svihmm_estep_sequence_subset(svihmm_ctx* h, const int32_t* idx, int32_t M, uint32_t flags, double* out_packed,
                                 double* out_seq_lb, double* out_q0) {
  const char* fn = "svihmm_estep_sequence_subset";
  if (!h) return fail(std::string(fn) + ": NULL handle");
  SubsetPlan p;
  CK(subset_plan(h, fn, idx, M, flags, p));
  CK(subset_enqueue(h, p, M, flags, false));
  return read_estep_sequences(h, M, out_packed, out_seq_lb, out_q0);
}

// ---- device-resident SVI loop (hmmsgd_metaobs.py:347-445) ------------------------------------
// layout of h->svi_state: var_tran K*K | prior_tran K*K | var_init K | vlb K | logdet K | prior_logpart K | rowterm K |
// var_init' K (the stationary vector is double-buffered: the next iteration's is computed ahead) | lb block 16 |
// ada_G K*K | prior_init K.  Sequence minibatches (svihmm_svi_sequences): var_init is the learned factor, first slot only
static double* svi_ptr(svihmm_ctx* h, int which) {
  const size_t K = h->svi_K, kk = K * K;
  double* b = (double*)h->svi_state.p;
  switch (which) {
    case 0: return b;                    // var_tran
    case 1: return b + kk;               // prior_tran
    case 2: return b + 2 * kk;           // var_init
    case 3: return b + 2 * kk + K;       // vlb
    case 4: return b + 2 * kk + 2 * K;   // logdet
    case 5: return b + 2 * kk + 3 * K;   // prior_logpart
    case 6: return b + 2 * kk + 4 * K;   // rowterm (Dirichlet terms of the transition rows)
    case 7: return b + 2 * kk + 5 * K;   // second var_init slot
    case 8: return b + 2 * kk + 6 * K;   // lb of the last two iterations (read by the side-stream ELBO kernel)
    case 10: return b + 3 * kk + 6 * K + 16;   // prior_init K (svihmm_svi_sequences)
    case 11: return b + 2 * kk + 6 * K + 2;    // the initial factor's ELBO term (svihmm_svi_sequences; in the lb block)
    default: return b + 2 * kk + 6 * K + 16;   // ada_G K*K (AdaGrad: accumulated squared natural parameters)
  }
}
#ifndef SVI_GW
#define SVI_GW 8      // wavefronts of the k_svi_globals workgroups
#endif
// counters of the loop's device-side dependencies (host.h): [0] global-step workgroups, [1] globals-kernel
// workgroups, [2] theta-builder workgroups, [3] ELBO side-chain workgroups; the gates' status word is slot 1 of the
// mapped status block (slot 0: the theta builders')
static unsigned* svi_cnt(svihmm_ctx* h, int which) { return (unsigned*)h->svi_sync.p + 16 * which; }
static int* svi_gate_status(svihmm_ctx* h) {
  int* d = nullptr;
  if (h->pin_status && hipHostGetDevicePointer((void**)&d, h->pin_status, 0) == hipSuccess) return d + 1;
  return nullptr;
}
static unsigned long long* svi_stamp_dev(svihmm_ctx* h, int idx) { return h->svi_ts_dev ? h->svi_ts_dev + idx : nullptr; }
// What every gate of the loop carries (flags mode): the status word in mapped host memory, the loop's dead flag
// (counter slot 7) and the bound of its wait.  Counter slots: [0] global-step workgroups, [1] globals-kernel
// workgroups, [2] theta-builder workgroups, [3] ELBO side chain, [4] sweep launches that signalled their start,
// [5] the poison word (SviSync::poison), [6] the concurrency probe's flag, [7] dead.
static SviSync svi_sy(svihmm_ctx* h) {
  SviSync sy = {};
  if (h->svi_flags) { sy.status = h->svi_status_dev; sy.dead = svi_cnt(h, 7); sy.ticks = h->svi_ticks; }
  return sy;
}
// Bound of a gate's wait.  A gate waits for work submitted earlier in host order, and the in-order side streams keep
// it from starting more than one iteration ahead of what it waits for: 64 measured iteration periods (at least 50 ms)
// once the device stamps of a finished iteration are there, 2 s before that, plus 20 us per row of the batch in
// flight (adaptive windows / buffers grow between two measurements); never more than SVI_SYNC_TICKS (60 s).
static unsigned long long svi_gate_ticks(const svihmm_ctx* h, int64_t rows) {
  const double khz = h->wall_clock_khz > 0.0 ? h->wall_clock_khz : 100000.0;
  double t = h->svi_period_ticks ? std::fmax(64.0 * (double)h->svi_period_ticks, 50.0 * khz) : 2000.0 * khz;
  t += 0.02 * (double)rows * khz;
  return t < (double)SVI_SYNC_TICKS ? (unsigned long long)t : SVI_SYNC_TICKS;
}
static int svi_launch_gate(svihmm_ctx* h, hipStream_t st, int which, unsigned long long tgt) {
  if (tgt == 0) return 0;
  SviSync sy = svi_sy(h);
  sy.gate = svi_cnt(h, which); sy.gate_tgt = (unsigned)tgt;
  hipLaunchKernelGGL(k_svi_gate, dim3(1), dim3(64), 0, st, sy);
  HIPCK(hipGetLastError());
  return 0;
}
// One-time probe per handle (see k_svi_probe_wait), for each of the loop's two side streams against the main one:
// the waiter goes first and the setter is launched only once the waiter reports that it is running, so the outcome
// does not depend on which queue a serialising tool serves first.  ~30 us per stream where kernels overlap, 2 ms
// where they do not.
static int svi_probe_concurrency(svihmm_ctx* h) {
  if (h->svi_concurrent >= 0) return 0;
  if (!h->stream2) HIPCK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
  if (!h->stream3) HIPCK(hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking));
  unsigned* pin = reinterpret_cast<unsigned*>(h->pin_status);      // words 2, 3: started / result (mapped)
  unsigned* dpin = nullptr;
  HIPCK(hipHostGetDevicePointer((void**)&dpin, pin, 0));
  unsigned* flag = svi_cnt(h, 6);
  volatile unsigned* vp = pin;
  int ok = 1;
  hipStream_t side[2] = {h->stream2, h->stream3};
  for (int i = 0; i < 2 && ok; ++i) {
    vp[2] = 0; vp[3] = 2;
    HIPCK(hipMemset(flag, 0, sizeof(unsigned)));
    hipLaunchKernelGGL(k_svi_probe_wait, dim3(1), dim3(64), 0, side[i], (const unsigned*)flag, dpin + 2, dpin + 3,
                       200000ull);
    HIPCK(hipGetLastError());
    for (int spin = 0; spin < 2000000 && vp[2] == 0; ++spin) { for (volatile int w = 0; w < 20; ++w) {} }
    hipLaunchKernelGGL(k_svi_probe_set, dim3(1), dim3(64), 0, h->stream, flag);
    HIPCK(hipGetLastError());
    HIPCK(hipStreamSynchronize(side[i]));
    HIPCK(hipStreamSynchronize(h->stream));
    ok = vp[3] == 1 ? 1 : 0;
  }
  h->svi_concurrent = ok;
  return 0;
}
// mod_init / ltran / exp(ltran) and its transpose for the loop's K, the padding rows behind the two matrices zeroed on
// stream `st` when the buffers are new
static int svi_globals_buffers(svihmm_ctx* h, hipStream_t st, bool zero_now) {
  const int K = h->svi_K;
  const size_t kk = (size_t)K * K * sizeof(double);
  CK(ensure(h->mod_init, K * sizeof(double)));
  CK(ensure(h->ltran, kk));
  const int reach = K <= 64 ? (K + 15) / 16 * 16 : K <= 128 ? 128 : K <= 256 ? 256 : K;
  const size_t slack = (size_t)(reach - K + 16) * K * sizeof(double);
  CK(ensure(h->Aexp, kk + slack));
  CK(ensure(h->AexpT, kk + slack));
  if (zero_now && (h->slack_a != h->Aexp.p || h->slack_t != h->AexpT.p || h->slack_k != K)) {
    HIPCK(hipMemsetAsync((char*)h->Aexp.p + kk, 0, slack, st));
    HIPCK(hipMemsetAsync((char*)h->AexpT.p + kk, 0, slack, st));
    h->slack_a = h->Aexp.p; h->slack_t = h->AexpT.p; h->slack_k = K;
  }
  return 0;
}
static int svi_globals(svihmm_ctx* h, int slot, int for_it) {
  const int K = h->svi_K;
  double* vi_out = svi_ptr(h, slot ? 7 : 2);
  CK(svi_globals_buffers(h, nullptr, false));
  // The globals kernel depends on var_tran only, i.e. on the previous global step: it is launched
  // on a side stream right after that step and runs beside the rest of the iteration (theta, ELBO
  // kernels) and the next iteration's uploads and emission GEMM; the sweeps wait for it
  // (wait_globals).  ~100 us off the critical path of a 64-window iteration.
  if (!h->stream2) HIPCK(hipStreamCreateWithFlags(&h->stream2, hipStreamNonBlocking));
  if (!h->svi_ea) {
    HIPCK(hipEventCreateWithFlags(&h->svi_ea, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&h->svi_eb, hipEventDisableTiming));
  }
  hipStream_t s2 = h->stream2;
  // (a globals kernel that finds the loop dead does not run: the iteration its output is for is poisoned)
  SviSync gsy = svi_sy(h);
  if (h->svi_flags) {
    gsy.arrive = svi_cnt(h, 1); h->tgt_glob += (unsigned)(K + 1);
    gsy.poison = svi_cnt(h, 5); gsy.poison_val = SVI_POISON_BASE - (unsigned)(for_it < 0 ? 0 : for_it);
  }
  if (h->svi_flags && h->tgt_step > 0) {
    // no event on the main stream: the side stream waits for the global steps launched so far in a one-wave gate
    CK(svi_launch_gate(h, s2, 0, h->tgt_step));
  } else {         // (svi_begin: behind the uploads of the main stream)
    HIPCK(hipEventRecord(h->svi_ea, h->stream));
    HIPCK(hipStreamWaitEvent(s2, h->svi_ea, 0));
  }
  CK(svi_globals_buffers(h, s2, true));       // (the padding rows, behind the wait above)
  const size_t work = 2 * (size_t)K * (K | 1) * sizeof(double);
  const int use_lds = work + 9 * 1024 <= 150 * 1024;
  if (!use_lds) CK(ensure(h->svi_work, work));
  {
    ProfScope ps(h, KS_MISC, s2);
    if (use_lds) {
      if (work > 48 * 1024)
        hipFuncSetAttribute((const void*)k_svi_globals<true, SVI_GW>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)work);
      hipLaunchKernelGGL((k_svi_globals<true, SVI_GW>), dim3(K + 1), dim3(64 * SVI_GW), work, s2, (const double*)svi_ptr(h, 0), K,
                         (double*)nullptr, (double*)h->ltran.p, (double*)h->Aexp.p, (double*)h->AexpT.p,
                         vi_out, (double*)h->mod_init.p, gsy);
    } else {
      hipLaunchKernelGGL((k_svi_globals<false, SVI_GW>), dim3(K + 1), dim3(64 * SVI_GW), 0, s2, (const double*)svi_ptr(h, 0), K,
                         (double*)h->svi_work.p, (double*)h->ltran.p, (double*)h->Aexp.p, (double*)h->AexpT.p,
                         vi_out, (double*)h->mod_init.p, gsy);
    }
    HIPCK(hipGetLastError());
  }
  HIPCK(hipEventRecord(h->svi_eb, s2));
  h->globals_ev = h->svi_eb;
  h->svi_globals_ready = true; h->svi_globals_slot = slot;
  h->K = K; h->have_globals = true; h->lin_stale = true;
  // (a host svihmm_set_globals between two iterations -- select_L, pred_logprob_full -- decides
  //  these per upload; the loop's own globals are back in the range svi_begin verified)
  h->exact_log = false; h->f32_ok = h->svi_f32_ok;
  return 0;
}
// theta + log det for the factors now in h->niw (main stream: the next emission GEMM needs theta);
// their ELBO term vlb[] and, with elbo_it >= 0, elbo_vec[elbo_it] on the side stream -- only the
// ELBO trace needs them, so they stay off the critical path of the iteration chain.
static int svi_launch_elbo(svihmm_ctx* h, int elbo_it, int lb_slot, bool behind_sweeps, hipEvent_t after_theta);
// columns the loop's simple step / ELBO kernels run over
static int svi_step_width(const svihmm_ctx* h) { return FAM_TRAITS[h->svi_family].svi_width_D ? h->svi_D : h->V; }
// what the step and ELBO kernels take for the loop on sequence minibatches (all nullptr: the window loop); M: the
// minibatch's size -- q0 lies behind the M local bounds in h->seq_out
static SviSeqStep svi_seq_args(svihmm_ctx* h, int M) {
  if (!h->svi_seq) return SviSeqStep{nullptr, nullptr, nullptr, nullptr};
  return SviSeqStep{M > 0 ? (const double*)h->seq_out.p + M : (const double*)nullptr, (const double*)svi_ptr(h, 10),
                    svi_ptr(h, 2), svi_ptr(h, 11)};
}
static int svi_refresh_emission(svihmm_ctx* h, int elbo_it, int lb_slot, hipEvent_t after_theta = nullptr,
                                bool defer_elbo = false, const SviStepArgs* step = nullptr) {
  const int K = h->svi_K, D = h->svi_D;
  const EmisFamily fam = h->svi_family;
  if (!h->stream3) HIPCK(hipStreamCreateWithFlags(&h->stream3, hipStreamNonBlocking));
  if (!h->svi_ec) {
    HIPCK(hipEventCreateWithFlags(&h->svi_ec, hipEventDisableTiming));
    HIPCK(hipEventCreateWithFlags(&h->svi_ed, hipEventDisableTiming));
  }
  // flags mode: the builder's K workgroups arrive on the theta counter (the ELBO kernels' gate) and workgroup 0
  // stamps the end of the iteration
  SviSync tsy = {};
  if (h->svi_flags) {
    tsy.arrive = svi_cnt(h, 2);
    h->tgt_theta += (unsigned)K;
    if (elbo_it >= 0) { tsy.stamp = svi_stamp_dev(h, 2 * elbo_it + 1); tsy.stamp_at = (unsigned)h->tgt_theta; }
  }
  h->theta_sy = tsy;
  if (fam == EF_NIW) CK(launch_niw_to_theta(h, K, D, svi_ptr(h, 4), step));
  else if (fam == EF_DIAG) CK(launch_diag_to_theta(h, K, D));
  else {
    // E log theta[v][k] = psi(alpha_kv) - psi(sum_v alpha_kv) (what hmmbase._push_emission uploads); per column for
    // EF_MCAT; the pairs (psi(a) - log b, a / b) for EF_POIS
    ProfScope ps(h, KS_MISC);
    if (fam == EF_CAT)
      hipLaunchKernelGGL(k_cat_table, dim3(K), dim3(64), 0, h->stream, (const double*)h->niw.p, K, h->V,
                         (double*)h->cat_table.p, tsy);
    else if (fam == EF_MCAT)
      hipLaunchKernelGGL(k_mcat_table, dim3(K), dim3(256), 0, h->stream, (const double*)h->niw.p, K, D, h->V,
                         (const int*)h->mcat_meta.p, (double*)h->cat_table.p, tsy);
    else
      hipLaunchKernelGGL(k_pois_table, dim3(K), dim3(64), 0, h->stream, (const double*)h->niw.p, K, D,
                         (double2*)h->cat_table.p, tsy);
    HIPCK(hipGetLastError());
    enter_table_family(h, fam, K, D, h->V);
  }
  h->theta_sy = SviSync{};
  h->lin_stale = true;
#ifdef SVIHMM_MEASURE
  if (h->variant[SVIHMM_VAR_SVI_LOOP] == SVIHMM_SVI_LOOP_NO_ELBO) return 0;    // measurement only: no ELBO kernels at all
#endif
  if (h->svi_flags && defer_elbo && elbo_it >= 0) {
    // launched by the next svihmm_svi_iteration behind its sweeps (svi_launch_elbo), or by whoever needs them first
    h->elbo_pending = true; h->elbo_pend_it = elbo_it; h->elbo_pend_slot = lb_slot;
    return 0;
  }
  return svi_launch_elbo(h, elbo_it, lb_slot, false, after_theta);
}
// The ELBO terms of the factors now in h->niw / theta (side stream).  `behind_sweeps`: additionally gated on the
// start of the sweep launch that carries counter 4.
static int svi_launch_elbo(svihmm_ctx* h, int elbo_it, int lb_slot, bool behind_sweeps, hipEvent_t after_theta) {
  const int K = h->svi_K, D = h->svi_D;
  const EmisFamily fam = h->svi_family;
  hipStream_t s2 = h->stream3;
  // (the ELBO kernels follow their gate kernels in stream order: when a gate gave up they find the loop dead and
  //  leave the iteration's entry NaN -- svi_recover computes it again where the state still allows)
  SviSync vsy = svi_sy(h);
  if (h->svi_flags) {
    CK(svi_launch_gate(h, s2, 2, h->tgt_theta));
    if (behind_sweeps) CK(svi_launch_gate(h, s2, 4, h->tgt_early));
    vsy.arrive = svi_cnt(h, 3);
    h->tgt_side += (unsigned)(2 * K);       // (the ELBO total rides in the last-arriving workgroup: kernels_svi.h)
  } else {
    // (the iteration's end-of-iteration timing event doubles as the fork point of the ELBO kernels)
    hipEvent_t fork = after_theta ? after_theta : h->svi_ec;
    HIPCK(hipEventRecord(fork, h->stream));
    HIPCK(hipStreamWaitEvent(s2, fork, 0));
  }
  {
    ProfScope ps(h, KS_MISC, s2);
    double* delbo = nullptr;
    if (elbo_it >= 0) HIPCK(hipHostGetDevicePointer((void**)&delbo, h->svi_elbo, 0));
    const bool tail = h->svi_flags && elbo_it >= 0;
    const SviElboTail et = {tail ? delbo + elbo_it : (double*)nullptr, (const double*)svi_ptr(h, 8) + lb_slot,
                            h->svi_prior_const, (unsigned)h->tgt_side};
    // sequence minibatches (stream events only, no tail): one more workgroup for the learned initial-state factor's
    // term, its prior constant beside the rows'
    const SviSeqStep sq = svi_seq_args(h, 0);
    const unsigned nvlb = (unsigned)(2 * K) + (h->svi_seq ? 1u : 0u);
    const double prior_const = h->svi_seq ? h->svi_prior_const + h->svi_prior_const_init : h->svi_prior_const;
    if (fam == EF_NIW)
      hipLaunchKernelGGL(k_svi_vlb, dim3(nvlb), dim3(64), 0, s2, (const double*)h->theta.p,
                         (const int*)h->fab.p, h->F, D, h->Kp, (const double*)h->niw.p,
                         (const double*)svi_ptr(h, 4), (const double*)h->svi_prior.p,
                         (const double*)svi_ptr(h, 5), h->svi_zsign, K, svi_ptr(h, 3),
                         (const double*)svi_ptr(h, 1), (const double*)svi_ptr(h, 0), svi_ptr(h, 6), vsy, et, sq);
    else
      hipLaunchKernelGGL(k_svi_vlb_simple, dim3(nvlb), dim3(64), 0, s2, (int)fam, (const double*)h->niw.p,
                         (const double*)h->svi_prior.p, K, svi_step_width(h), svi_ptr(h, 3),
                         (const double*)svi_ptr(h, 1), (const double*)svi_ptr(h, 0), svi_ptr(h, 6),
                         (const int*)(fam == EF_MCAT ? h->mcat_meta.p : nullptr), D, vsy, et, sq);
    if (elbo_it >= 0 && !tail) {      // (stream-event choreography: no arrival counter to tell the last workgroup by)
      hipLaunchKernelGGL(k_svi_elbo, dim3(1), dim3(64), 0, s2, K, (const double*)svi_ptr(h, 3),
                         (const double*)svi_ptr(h, 6), prior_const, (const double*)svi_ptr(h, 8) + lb_slot,
                         delbo + elbo_it, vsy, (const double*)sq.term);
    }
    HIPCK(hipGetLastError());
  }
  HIPCK(hipEventRecord(h->svi_ed, s2));
  h->vlb_pending = true;
  return 0;
}
// deferred ELBO kernels, now and ungated: somebody is about to wait for the side stream or to rewrite what they read
int svi_flush_elbo(svihmm_ctx* h) {
  if (!h->elbo_pending) return 0;
  h->elbo_pending = false;
  return svi_launch_elbo(h, h->elbo_pend_it, h->elbo_pend_slot, false, nullptr);
}

// What the families' begin calls share: range check of the transition factor, the resident
// state (var_tran | prior_tran | ...), the ELBO / event rings.  The caller uploads its prior / factor
// blocks between svi_begin_common and svi_begin_finish.
static int svi_begin_common(svihmm_ctx* h, int K, int D, const double* prior_tran, const double* var_tran,
                            int maxit, EmisFamily family) {
  if (K > 1024) return fail("svihmm_svi_begin: K > 1024 unsupported");
  if (h->D != D) return fail("svihmm_svi_begin: D does not match the resident observations");
  // from here on the previous loop's state is being overwritten: a begin that fails half way must not
  // leave it marked as live (svi_begin_finish sets the flag again once everything is in place)
  h->svi_active = false;
  h->svi_adagrad = false;
  h->svi_seq = false; h->svi_prior_const_init = 0.0;
  CK(set_device(h));
  CK(wait_side_streams(h));
  CK(drop_auto_status(h));
  if (fam_gaussian(family)) CK(centre_deferred(h));       // (symbol and count families: the copy stays uncentred)
  const size_t kk = (size_t)K * K;
  {
    // The global step is var_tran <- (1 - rho) var_tran + rho (1 + bA (A_raw + nwin (prior_tran - 1)))
    // with bA nwin ~ T / 2L >> 1 (quirk Q2): only for prior_tran >= 1 is every later entry bounded
    // below by min(var_tran, 1), so that psi(v) - psi(row sum) stays inside the range of the
    // linear-domain recursions for the whole loop (the row sums are < 1e12: psi < 28).  Sparser
    // priors can drive entries towards zero or below mid-loop; the host loop, which picks the
    // recursion per upload, serves those.
    double vmin = INFINITY, pmin = INFINITY;
    for (size_t i = 0; i < kk; ++i) { vmin = std::fmin(vmin, var_tran[i]); pmin = std::fmin(pmin, prior_tran[i]); }
    if (!(vmin >= SVIHMM_SVI_MIN_PSEUDOCOUNT) || !(pmin >= 1.0))
      return fail("svihmm_svi_begin: prior_tran below 1 or var_tran below SVIHMM_SVI_MIN_PSEUDOCOUNT may need the "
                  "log-domain recursion mid-loop: run the loop through svihmm_set_globals + svihmm_estep_minibatch");
    h->svi_f32_ok = vmin > 0.05;      // psi(0.05) - 28 > SVIHMM_LTRAN_F32_MIN
    h->svi_vmin = vmin;
    h->exact_log = false;
    h->f32_ok = h->svi_f32_ok;
  }
  h->svi_K = K; h->svi_D = D; h->svi_maxit = maxit; h->svi_family = family;
  {   // sum_i [lgamma(sum_j p_ij + eps) - sum_j lgamma(p_ij + eps)]: the prior-only part of the rows' energy
    double pc = 0.0;
    for (int i = 0; i < K; ++i) {
      double rsum = 0.0, lg = 0.0;
      for (int j = 0; j < K; ++j) { const double p = prior_tran[(size_t)i * K + j]; rsum += p; lg += std::lgamma(p + 1e-9); }
      pc += std::lgamma(rsum + 1e-9) - lg;
    }
    h->svi_prior_const = pc;
  }
  CK(ensure(h->svi_state, (3 * kk + 7 * (size_t)K + 16) * sizeof(double)));
  h->svi_adagrad = false;
  CK(upload_blocks(h, svi_ptr(h, 0), {{var_tran, kk}, {prior_tran, kk}}));
  if (h->svi_elbo_cap < maxit) {
    if (h->svi_elbo) hipHostFree(h->svi_elbo);
    h->svi_elbo = nullptr; h->svi_elbo_cap = 0;
    HIPCK(hipHostMalloc((void**)&h->svi_elbo, (size_t)maxit * sizeof(double) + 64, hipHostMallocMapped));
    h->svi_elbo_cap = maxit;
  }
  for (int i = 0; i < maxit; ++i) h->svi_elbo[i] = NAN;
  // device-side dependencies (SVI_LOOP = SVIHMM_SVI_LOOP_EVENTS: the stream-event choreography of rounds 2-4 instead)
  h->svi_flags = h->variant[SVIHMM_VAR_SVI_LOOP] != SVIHMM_SVI_LOOP_EVENTS;
  h->tgt_step = h->tgt_glob = h->tgt_theta = h->tgt_side = h->tgt_early = 0;
  h->elbo_pending = false;
  h->svi_period_ticks = 0; h->svi_cur_it = -1; h->svi_replaying = false; h->svi_recoveries = 0;
  for (auto& e : h->svi_log) e.it = -1;
  h->svi_it_events.assign(maxit, (char)0);
  if (h->svi_flags) {
    // (begin is cold: the counters are zeroed with every stream idle, so no gate of this loop can see a
    //  previous loop's counts)
    CK(ensure(h->svi_sync, 8 * 64));
    HIPCK(hipStreamSynchronize(h->stream));
    HIPCK(hipMemset(h->svi_sync.p, 0, 8 * 64));
    if (h->svi_ts_cap < 2 * maxit) {
      if (h->svi_ts) hipHostFree(h->svi_ts);
      h->svi_ts = nullptr; h->svi_ts_dev = nullptr; h->svi_ts_cap = 0;
      HIPCK(hipHostMalloc((void**)&h->svi_ts, (size_t)2 * maxit * sizeof(unsigned long long) + 64, hipHostMallocMapped));
      h->svi_ts_cap = 2 * maxit;
      HIPCK(hipHostGetDevicePointer((void**)&h->svi_ts_dev, h->svi_ts, 0));
    }
    std::memset(h->svi_ts, 0, (size_t)2 * maxit * sizeof(unsigned long long));
    if (!h->pin_status) {
      HIPCK(hipHostMalloc((void**)&h->pin_status, 64, hipHostMallocMapped));
      std::memset(h->pin_status, 0, 64);
    }
    h->pin_status[1] = 0;
    h->svi_status_dev = svi_gate_status(h);
    // a device that runs one kernel at a time (a counter-collecting profiler, serialised launches) cannot carry
    // spinning gates: stream events there
    CK(svi_probe_concurrency(h));
    if (h->svi_concurrent != 1) h->svi_flags = false;
    if (h->wall_clock_khz <= 0.0) {
      int khz = 0;
      if (hipDeviceGetAttribute(&khz, hipDeviceAttributeWallClockRate, h->device) != hipSuccess || khz <= 0) khz = 100000;
      h->wall_clock_khz = (double)khz;
    }
    h->svi_ticks = svi_gate_ticks(h, 0);
  }
  // (event choreography only: the counter loop times its iterations with device stamps)
  while (!h->svi_flags && (int)h->svi_ev.size() < 2 * maxit) {      // [2 it]: first launch of iteration it, [2 it + 1]: its last
    hipEvent_t e;
    HIPCK(hipEventCreate(&e));
    h->svi_ev.push_back(e);
  }
  h->svi_ev_begin.assign(maxit, 0);
  h->svi_last_it = -1;
  return 0;
}
static int svi_begin_finish(svihmm_ctx* h) {
  HIPCK(hipStreamSynchronize(h->stream));          // (the rings below are keyed to this loop's events)
  for (auto& ss : h->svi_starts) ss.used_it = -1;
  CK(svi_refresh_emission(h, -1, 0));   // theta / table of the initial factors (their vlb is not used)
  // (the slot svihmm_svi_read_state / _read_factors hand out: before the first iteration it is the one the
  //  globals below write -- it used to be 1, and a read right after begin returned the never-written second slot)
  h->svi_vi_cur = 0;
  CK(svi_globals(h, 0, 0));          // globals of iteration 0
  h->svi_active = true;
  return 0;
}

int svihmm_svi_begin(svihmm_ctx* h, int32_t K, int32_t D, const double* prior_tran, const double* var_tran,
                     const double* mu0, const double* sigma0, const double* kappa0, const double* nu0,
                     const double* prior_logpart, const double* mu, const double* sigma,
                     const double* kappa, const double* nu, int32_t maxit, double zsign) {
  if (!h || K <= 0 || D <= 0 || !prior_tran || !var_tran || !mu0 || !sigma0 || !kappa0 || !nu0 ||
      !prior_logpart || !mu || !sigma || !kappa || !nu || maxit <= 0)
    return fail("svihmm_svi_begin: bad arguments");
  CK(svi_begin_common(h, K, D, prior_tran, var_tran, maxit, EF_NIW));
  h->svi_zsign = zsign;
  const size_t nmu = (size_t)K * D, nsg = (size_t)K * D * D;
  const size_t nin = nmu + nsg + 2 * (size_t)K;
  CK(ensure(h->svi_prior, (nin + 8) * sizeof(double)));
  CK(ensure(h->niw, nin * sizeof(double) + 64));
  // (the loop's state lives in the resident copy's coordinates: both blocks' means travel centred)
  const size_t k = (size_t)K;
  CK(upload_blocks(h, svi_ptr(h, 5), {{prior_logpart, k}}));
  CK(upload_blocks(h, h->svi_prior.p, {{mu0, nmu}, {sigma0, nsg}, {kappa0, k}, {nu0, k}}, K, D));
  CK(upload_blocks(h, h->niw.p, {{mu, nmu}, {sigma, nsg}, {kappa, k}, {nu, k}}, K, D));
  return svi_begin_finish(h);
}

// Diagonal family (distributions.DiagonalGaussian: per dimension a normal-inverse-gamma factor):
// blocks [mu | nus | alphas | betas], each [K][D]; the same loop with the family's natural-parameter
// blend (hmmsgd_metaobs.py:1050-1069 in [nu mu, nu, 2 beta + nu mu^2, 2 alpha]), theta from
// k_diag_to_theta, ELBO term -KL(q || prior) per dimension.
int svihmm_svi_begin_diag(svihmm_ctx* h, int32_t K, int32_t D, const double* prior_tran, const double* var_tran,
                          const double* prior_blk, const double* factor_blk, int32_t maxit) {
  if (!h || K <= 0 || D <= 0 || !prior_tran || !var_tran || !prior_blk || !factor_blk || maxit <= 0)
    return fail("svihmm_svi_begin_diag: bad arguments");
  if (D > SVIHMM_DIAG_MAX_D) return fail("svihmm_svi_begin_diag: D > SVIHMM_DIAG_MAX_D");
  const size_t n4 = 4 * (size_t)K * D;
  for (size_t i = (size_t)K * D; i < n4; ++i)       // (validated before any state is touched)
    if (!(prior_blk[i] > 0.0) || !(factor_blk[i] > 0.0)) return fail("svihmm_svi_begin_diag: nus, alphas, betas must be positive");
  CK(svi_begin_common(h, K, D, prior_tran, var_tran, maxit, EF_DIAG));
  CK(ensure(h->svi_prior, (n4 + 8) * sizeof(double)));
  CK(ensure(h->niw, n4 * sizeof(double) + 64));
  CK(upload_blocks(h, h->svi_prior.p, {{prior_blk, n4}}, K, D));
  CK(upload_blocks(h, h->niw.p, {{factor_blk, n4}}, K, D));
  return svi_begin_finish(h);
}

// Categorical family (hmmsgd_metaobs.py:907-926, 1071-1084): Dirichlet factors alpha[K][V] over one
// integer-valued observation column; the table E log theta is rebuilt on the device every iteration.
int svihmm_svi_begin_cat(svihmm_ctx* h, int32_t K, int32_t V, const double* prior_tran, const double* var_tran,
                         const double* alpha0, const double* alpha, int32_t maxit) {
  if (!h || K <= 0 || V <= 0 || !prior_tran || !var_tran || !alpha0 || !alpha || maxit <= 0)
    return fail("svihmm_svi_begin_cat: bad arguments");
  if (h->D != 1) return fail("svihmm_svi_begin_cat: the resident observations must be one symbol column (D = 1)");
  const size_t n = (size_t)K * V;
  for (size_t i = 0; i < n; ++i)
    if (!(alpha0[i] > 0.0) || !(alpha[i] > 0.0)) return fail("svihmm_svi_begin_cat: Dirichlet parameters must be positive");
  CK(svi_begin_common(h, K, 1, prior_tran, var_tran, maxit, EF_CAT));
  h->V = V;
  CK(cat_uncentre(h));
  CK(ensure(h->svi_prior, (n + 8) * sizeof(double)));
  CK(ensure(h->niw, n * sizeof(double) + 64));
  CK(ensure(h->cat_table, n * sizeof(double)));
  CK(upload_blocks(h, h->svi_prior.p, {{alpha0, n}}));
  CK(upload_blocks(h, h->niw.p, {{alpha, n}}));
  return svi_begin_finish(h);
}

// Multi-column Categorical family (distributions.ProductCategorical): D Dirichlet factors per state over the D symbol
// columns, alpha0 / alpha [K][F] with the feature offsets of svihmm_set_emission_mcat.  Column by column the step and
// the ELBO term of svihmm_svi_begin_cat; the [F][K] table is rebuilt by k_mcat_table every iteration.
int svihmm_svi_begin_mcat(svihmm_ctx* h, int32_t K, int32_t D, const int32_t* V, const double* prior_tran,
                          const double* var_tran, const double* alpha0, const double* alpha, int32_t maxit) {
  if (!h || !V || !prior_tran || !var_tran || !alpha0 || !alpha || maxit <= 0)
    return fail("svihmm_svi_begin_mcat: bad arguments");
  int F = 0;
  CK(check_mcat_shape("svihmm_svi_begin_mcat", K, D, V, &F));
  if (h->D != D)
    return fail("svihmm_svi_begin_mcat: the family has D = " + std::to_string(D) + " symbol columns, the resident observations have " +
                std::to_string(h->D));
  const size_t n = (size_t)K * F;
  for (size_t i = 0; i < n; ++i)       // (validated before any state is touched)
    if (!(alpha0[i] > 0.0) || !(alpha[i] > 0.0)) return fail("svihmm_svi_begin_mcat: Dirichlet parameters must be positive");
  CK(svi_begin_common(h, K, D, prior_tran, var_tran, maxit, EF_MCAT));
  h->V = F;
  h->svi_mcat_V.assign(V, V + D);
  CK(cat_uncentre(h, 0));
  CK(ensure(h->svi_prior, (n + 8) * sizeof(double)));
  CK(ensure(h->niw, n * sizeof(double) + 64));
  CK(ensure(h->cat_table, n * sizeof(double)));
  CK(upload_mcat_meta(h, D, F, V));
  CK(upload_blocks(h, h->svi_prior.p, {{alpha0, n}}));
  CK(upload_blocks(h, h->niw.p, {{alpha, n}}));
  return svi_begin_finish(h);
}

// Poisson family (distributions.ProductPoisson): Gamma factors (shape a, rate b) per state and count column, blocks
// [a | b], each [K][D].  The (E log lambda, E lambda) pairs are rebuilt by k_pois_table every iteration; the logfact
// table is uploaded here, once.
int svihmm_svi_begin_poisson(svihmm_ctx* h, int32_t K, int32_t D, const double* prior_tran, const double* var_tran,
                             const double* prior_blk, const double* factor_blk, const double* logfact, int32_t C,
                             int32_t maxit) {
  if (!h || !prior_tran || !var_tran || !prior_blk || !factor_blk || !logfact || maxit <= 0)
    return fail("svihmm_svi_begin_poisson: bad arguments");
  CK(check_poisson_shape("svihmm_svi_begin_poisson", K, D, C, logfact));
  if (h->D != D)
    return fail("svihmm_svi_begin_poisson: the family has D = " + std::to_string(D) + " count columns, the resident observations have " +
                std::to_string(h->D));
  const size_t n2 = 2 * (size_t)K * D;
  for (size_t i = 0; i < n2; ++i)      // (validated before any state is touched)
    if (!(prior_blk[i] > 0.0) || !(factor_blk[i] > 0.0)) return fail("svihmm_svi_begin_poisson: Gamma parameters must be positive");
  CK(svi_begin_common(h, K, D, prior_tran, var_tran, maxit, EF_POIS));
  h->V = 2 * D;
  h->pois_C = C;
  CK(cat_uncentre(h, 1));
  CK(ensure(h->svi_prior, (n2 + 8) * sizeof(double)));
  CK(ensure(h->niw, n2 * sizeof(double) + 64));
  CK(ensure(h->cat_table, (n2 + 2 * (size_t)K) * sizeof(double)));
  CK(upload_logfact(h, logfact, C));
  CK(upload_blocks(h, h->svi_prior.p, {{prior_blk, n2}}));
  CK(upload_blocks(h, h->niw.p, {{factor_blk, n2}}));
  return svi_begin_finish(h);
}

static int svi_iteration_impl(svihmm_ctx* h, int32_t it, const int64_t* starts, int32_t B, int32_t nwin_total,
                              int32_t Lm, int32_t inner_off, int32_t inner_len, uint32_t flags, double rho,
                              double bfactA, double bfactE);
// elements per state of the element-wise global step: D (diagonal, Poisson: one thread per (k, d)), V (Categorical),
// F (multi-column Categorical: h->V holds it)
// Leave the counters in the middle of a loop and carry on with the stream-event choreography (round 6).  Two
// callers: a gate of the loop gave up (the status word is set: a tool that serialises kernels attached after
// svihmm_svi_begin's probe, another process time-slicing the device, a partition too small for the loop's
// kernels side by side), or the host decides to (`clean`: SVIHMM_SVI_LOOP_LOSE_CONCURRENCY).  When a gate gave up the loop is
// dead on the device: every later gate returned at once, the E-steps whose inputs were missing poisoned their
// iteration and the global steps from that iteration on did not run (device_helpers.h) -- the loop's state is the
// one after iteration p - 1, whole.  The iterations from p on are replayed from the host's log (the host runs at
// most eight iterations ahead: the window-start ring), the last applied iteration's ELBO entry is formed again
// if its kernels were caught by the shutdown.  The event loop computes bit for bit what the counter loop does
// (tests/test_gpu_classes.py::test_svi_loop_on_counters_equals_the_stream_event_loop).
// every stream idle: counters, targets and the status word cleared, the iteration events there -- from here on the loop
// runs on stream order and events
static int svi_leave_counters(svihmm_ctx* h) {
  HIPCK(hipMemset(h->svi_sync.p, 0, 8 * 64));
  h->pin_status[1] = 0;
  h->tgt_step = h->tgt_glob = h->tgt_theta = h->tgt_side = h->tgt_early = 0;
  h->elbo_pending = false; h->vlb_pending = false; h->globals_ev = nullptr;
  h->svi_flags = false;
  while ((int)h->svi_ev.size() < 2 * h->svi_maxit) {
    hipEvent_t e;
    HIPCK(hipEventCreate(&e));
    h->svi_ev.push_back(e);
  }
  return 0;
}
static int svi_recover(svihmm_ctx* h, bool clean) {
  if (!h->svi_flags) return 0;
  if (clean) CK(svi_flush_elbo(h));
  HIPCK(hipStreamSynchronize(h->stream));
  if (h->stream2) HIPCK(hipStreamSynchronize(h->stream2));
  if (h->stream3) HIPCK(hipStreamSynchronize(h->stream3));
  unsigned poison = 0;
  HIPCK(hipMemcpy(&poison, svi_cnt(h, 5), sizeof(unsigned), hipMemcpyDeviceToHost));
  const int submitted = h->svi_last_it;                     // last iteration handed to the device
  const int p = poison ? (int)(SVI_POISON_BASE - poison) : submitted + 1;   // first iteration that did not reach the state
  CK(svi_leave_counters(h));
  ++h->svi_recoveries;
  if (p > submitted + 1 || p < 0) return fail("SVI loop: inconsistent poison word after a gate gave up");
  // the ELBO entry of the last iteration that did reach the state: its kernels may have found the loop dead
  if (p >= 1 && std::isnan(h->svi_elbo[p - 1])) CK(svi_launch_elbo(h, p - 1, (p - 1) & 1, false, nullptr));
  if (p > submitted) return 0;                              // nothing was lost: the next iteration's globals are in place
  // replay iterations p .. submitted
  for (int j = p; j <= submitted; ++j)
    if (h->svi_log[j % 16].it != j) return fail("SVI loop: iteration " + std::to_string(j) + " is no longer in the replay log");
  h->svi_globals_ready = false;                             // (the globals on the device stem from a skipped kernel)
  h->svi_last_it = p - 1;
  h->svi_vmin = h->svi_log[p % 16].vmin_before;
  h->svi_f32_ok = h->svi_log[p % 16].f32_ok_before;
  h->svi_replaying = true;
  int rc = 0;
  for (int j = p; j <= submitted && rc == 0; ++j) {
    const SviLogEntry& e = h->svi_log[j % 16];
    rc = svi_iteration_impl(h, e.it, e.starts.data(), e.B, e.nwin, e.Lm, e.off, e.len, e.flags, e.rho, e.bA, e.bE);
  }
  h->svi_replaying = false;
  return rc;
}
int svihmm_svi_recoveries(svihmm_ctx* h, int32_t* out) {
  if (!h || !out) return fail("svihmm_svi_recoveries: bad arguments");
  *out = h->svi_recoveries;
  return 0;
}

int svihmm_svi_iteration(svihmm_ctx* h, int32_t it, const int64_t* starts, int32_t B, int32_t nwin_total,
                         int32_t Lm, int32_t inner_off, int32_t inner_len, uint32_t flags, double rho,
                         double bfactA, double bfactE) {
  if (h && h->have_labels)
    return fail("svihmm_svi_iteration: labels are in force (svihmm_set_labels) and the resident SVI loop does not "
                "take them; remove them with svihmm_set_labels(h, NULL) or step on the host from "
                "svihmm_estep_minibatch's statistics");
  if (h && h->have_sets)
    return fail("svihmm_svi_iteration: allowed-state sets are in force (svihmm_set_state_sets) and the resident SVI "
                "loop does not take them; remove them with svihmm_set_state_sets(h, NULL, 0) or step on the host from "
                "svihmm_estep_minibatch's statistics");
  if (h && !h->svi_active && h->have_emission && FAM_TRAITS[h->fam].noun) {
    const FamTraits& t = FAM_TRAITS[h->fam];
    const std::string head = std::string("svihmm_svi_iteration: the resident SVI loop does not take ") + t.noun;
    if (t.svi_begin)
      return fail(head + " from " + t.setter + " alone: the family enters the loop through " + t.svi_begin);
    return fail(head + " of " + t.setter + "; step the globals on the host from svihmm_estep_minibatch's statistics");
  }
  if (!h || !h->svi_active) return fail("svihmm_svi_iteration: call svihmm_svi_begin first");
  if (h->svi_seq)
    return fail("svihmm_svi_iteration: the loop steps on minibatches of whole sequences since svihmm_svi_sequences: "
                "call svihmm_svi_iteration_sequences");
  if (it < 0 || it >= h->svi_maxit) return fail("svihmm_svi_iteration: iteration index out of range");
  if (B < 0 || (B > 0 && !starts) || nwin_total < B) return fail("svihmm_svi_iteration: bad window batch");
  if (flags & SVIHMM_USE_HOST_LLIKS) return fail("svihmm_svi_iteration: device-side emission families only");
  CK(set_device(h));
  if (h->svi_flags) {
    // a gate of the loop gave up since the last call (mapped status word: a plain host read)
    if (h->pin_status && *(volatile int*)&h->pin_status[1] != 0) CK(svi_recover(h, false));
    // (debug: "concurrency lost" between two iterations)
    else if (h->variant[SVIHMM_VAR_SVI_LOOP] == SVIHMM_SVI_LOOP_LOSE_CONCURRENCY && it == 3) CK(svi_recover(h, true));
  }
  if (h->svi_flags) {
    // the iteration period, from the device stamps of an iteration that is certainly complete (eight back)
    const int j = it - 8;
    if (j >= 0 && (int)h->svi_ev_begin.size() > j && h->svi_ts) {
      const unsigned long long t0 = h->svi_ts[h->svi_ev_begin[j]], t1 = h->svi_ts[2 * j + 1];
      if (t0 && t1 > t0 && t1 - t0 > h->svi_period_ticks) h->svi_period_ticks = t1 - t0;
    }
    h->svi_ticks = svi_gate_ticks(h, (int64_t)B * Lm);
  }
  {
    SviLogEntry& e = h->svi_log[it % 16];
    e.it = it; e.B = B; e.nwin = nwin_total; e.Lm = Lm; e.off = inner_off; e.len = inner_len; e.flags = flags;
    e.rho = rho; e.bA = bfactA; e.bE = bfactE; e.vmin_before = h->svi_vmin; e.f32_ok_before = h->svi_f32_ok;
    e.starts.assign(starts, starts + (B > 0 ? B : 0));
  }
  return svi_iteration_impl(h, it, starts, B, nwin_total, Lm, inner_off, inner_len, flags, rho, bfactA, bfactE);
}
static int svi_iteration_impl(svihmm_ctx* h, int32_t it, const int64_t* starts, int32_t B, int32_t nwin_total,
                              int32_t Lm, int32_t inner_off, int32_t inner_len, uint32_t flags, double rho,
                              double bfactA, double bfactE) {
  const int K = h->svi_K, D = h->svi_D;
  h->svi_cur_it = it;
  if ((int)h->svi_it_events.size() < h->svi_maxit) h->svi_it_events.resize(h->svi_maxit, (char)0);
  h->svi_it_events[it] = h->svi_flags ? (char)0 : (char)1;
  // start of the iteration: when the previous iteration is still running, the stream would execute
  // this marker right behind that iteration's end marker -- the end marker serves as both
  if ((int)h->svi_ev_begin.size() < h->svi_maxit) h->svi_ev_begin.resize(h->svi_maxit, 0);
  h->svi_ev_begin[it] = 2 * it;
  if (h->svi_flags) {
    // (stamps instead of events: the previous iteration's end stamp -- written by its theta builder into mapped
    //  host memory -- is still 0 while that iteration runs)
    if (it > 0 && h->svi_last_it == it - 1 && *(volatile unsigned long long*)&h->svi_ts[2 * it - 1] == 0)
      h->svi_ev_begin[it] = 2 * it - 1;
    else {
      hipLaunchKernelGGL(k_svi_stamp, dim3(1), dim3(64), 0, h->stream, svi_stamp_dev(h, 2 * it));
      HIPCK(hipGetLastError());
    }
  } else if (it > 0 && h->svi_last_it == it - 1 && hipEventQuery(h->svi_ev[2 * it - 1]) == hipErrorNotReady)
    h->svi_ev_begin[it] = 2 * it - 1;
  else
    HIPCK(hipEventRecord(h->svi_ev[2 * it], h->stream));
  (void)hipGetLastError();            // (hipErrorNotReady is not an error here)
  h->svi_last_it = it;
  if (!h->svi_globals_ready) CK(svi_globals(h, h->svi_vi_cur ^ 1, it));   // (a host set_globals came in between)
  h->svi_vi_cur = h->svi_globals_slot;
  h->svi_globals_ready = false;       // consumed by this iteration's sweeps
  const bool keep = (flags & SVIHMM_SVI_KEEP_WINDOW) != 0;
  flags &= ~(uint32_t)SVIHMM_SVI_KEEP_WINDOW;
  if (B > 0) {
    h->svi_upload_it = it;
    h->in_svi_estep = true;
    h->sweep_signalled = false;
    const int rc = estep_core(h, starts, B, Lm, inner_off, inner_len, flags);
    h->in_svi_estep = false;
    h->svi_upload_it = -1;
    // the previous iteration's ELBO kernels: behind this iteration's sweeps when their launch signals its start
    if (rc == 0 && h->elbo_pending) {
      h->elbo_pending = false;
      CK(svi_launch_elbo(h, h->elbo_pend_it, h->elbo_pend_slot, h->sweep_signalled, nullptr));
    }
    if (rc) return rc;
    // the last window's log-domain rows are rebuilt on demand from the CURRENT parameters:
    // do it now, before the global step replaces them
    if (keep && h->lin_mode) CK(materialise(h, B - 1, 1));
  } else {   // empty shard of a multi-GPU minibatch: all-zero statistics
    const size_t nb = (size_t)packed_len(h) * sizeof(double);
    CK(ensure(h->packed, nb));
    HIPCK(hipMemsetAsync(h->packed.p, 0, nb, h->stream));
    h->have_packed = true; h->mirror_valid = false;
  }
  if (h->comm) {
    ProfScope ps(h, KS_ALLREDUCE);
    CK(allreduce_packed_dev(h));
  }
  const bool flushed_now = h->elbo_pending;
  CK(svi_flush_elbo(h));   // (an empty shard, or an E-step that failed over to an ungated path)
  CK(wait_globals(h));     // (an empty shard ran no sweeps; a gated sweep kernel has cleared the event)
  // the previous iteration's ELBO kernels (their own stream) read var_tran / theta / logdet,
  // which this global step and the NIW kernel after it rewrite (normally long finished): flags mode gates the
  // step kernel on their counter, the event mode waits for their event
  // (NIW factors of 17 .. 32 dimensions: the step rides in the theta builder's launch -- k_svi_step_theta32s)
  const bool merged = h->svi_family == EF_NIW && step_theta_ok(h, K, D);
  const unsigned ntran = merged ? (unsigned)((K * K + 63) / 64) : (unsigned)((K * K + 255) / 256);
  const unsigned step_grid = h->svi_family == EF_NIW ? (unsigned)K + ntran
                                                : (unsigned)(((size_t)K * svi_step_width(h) + 255) / 256) + ntran;
  SviSync ssy = svi_sy(h);
  if (h->svi_flags) {
    ssy.gate = svi_cnt(h, 3); ssy.gate_tgt = (unsigned)h->tgt_side; ssy.arrive = svi_cnt(h, 0);
    ssy.poison = svi_cnt(h, 5);
    if (h->tgt_side == 0) ssy.gate = nullptr;
    // A gated grid must leave room for what it waits for.  The step's workgroups all spin in their gate: a grid
    // that can hold half the device's wave slots (K beyond ~600), or ELBO kernels that were enqueued only just now
    // (svi_flush_elbo above: they may not be resident yet), could keep those kernels off the device -- the stream
    // waits for their event instead (recorded in both modes, svi_launch_elbo).
    const bool big = (size_t)step_grid * (merged ? 1 : 4) > (size_t)h->ncu * h->waves_per_cu / 2;
    if (ssy.gate && (big || flushed_now) && h->vlb_pending) {
      HIPCK(hipStreamWaitEvent(h->stream, h->svi_ed, 0));
      ssy.gate = nullptr;
    }
  } else CK(wait_vlb(h));
  double* adag = h->svi_adagrad ? svi_ptr(h, 9) : (double*)nullptr;
  SviStepArgs sargs = {(const double*)h->packed.p, (const double*)svi_ptr(h, 1), svi_ptr(h, 0), (const double*)h->svi_prior.p,
                       rho, bfactA, bfactE, (double)nwin_total, svi_ptr(h, 8) + (it & 1), adag, ssy,
                       SviSeqStep{nullptr, nullptr, nullptr, nullptr}};
  if (merged) {
    if (h->svi_flags) h->tgt_step += ntran;          // (the merged kernel's transition workgroups: see k_svi_step_theta32s)
  } else {
    ProfScope ps(h, KS_MISC);
    if (h->svi_family == EF_NIW)
      hipLaunchKernelGGL(k_svi_global_step, dim3((unsigned)K + ntran), dim3(256), (size_t)3 * D * sizeof(double), h->stream,
                         (const double*)h->packed.p, (const double*)svi_ptr(h, 1), svi_ptr(h, 0),
                         (double*)h->niw.p, (const double*)h->svi_prior.p, K, D, rho, bfactA, bfactE,
                         (double)nwin_total, svi_ptr(h, 8) + (it & 1), adag, ssy, sargs.sq);
    else {
      const int W = svi_step_width(h);
      const unsigned nem = (unsigned)(((size_t)K * W + 255) / 256);
      hipLaunchKernelGGL(k_svi_global_step_simple, dim3(nem + ntran), dim3(256), 0, h->stream, (int)h->svi_family,
                         (const double*)h->packed.p, (const double*)svi_ptr(h, 1), svi_ptr(h, 0),
                         (double*)h->niw.p, (const double*)h->svi_prior.p, K, W, rho, bfactA, bfactE,
                         (double)nwin_total, svi_ptr(h, 8) + (it & 1), adag, (int)nem, ssy, sargs.sq);
    }
    HIPCK(hipGetLastError());
    if (h->svi_flags) h->tgt_step += step_grid;
  }
  // the next iteration's globals, ahead of time, forked right behind the global step (its own event:
  // forked behind theta together with the ELBO kernels it competes with the next emission GEMM,
  // ends after that GEMM, and a stream wait that really has to block wakes up ~20 us late -- measured
  // 0.272 against 0.25 ms per iteration)
  // Lower bound of var_tran after this step, kept on the host: the plain step is
  // v <- (1 - rho) v + rho (1 + bA (A_raw + nwin (prior_tran - 1))) with prior_tran >= 1 and A_raw >= 0,
  // so every entry is >= (1 - rho) bound + rho.  A loop that started below the fp32 mode's range for
  // E[log A] (a class's default initial var_tran of 1/K) enters it after its first steps (rho_0 = 1 for
  // tau = 1) instead of running fp64 to the end.  AdaGrad's element-wise weights give no such bound.
  if (!h->svi_adagrad && rho >= 0.0 && rho <= 1.0) {
    h->svi_vmin = (1.0 - rho) * h->svi_vmin + rho;
    h->svi_f32_ok = h->svi_vmin > 0.05;
  }
  if (merged) {
    // step + theta in one launch FIRST: the globals kernel's gate must wait for work submitted earlier in host order
    CK(svi_refresh_emission(h, it, it & 1, h->svi_flags ? (hipEvent_t) nullptr : h->svi_ev[2 * it + 1], it + 1 < h->svi_maxit, &sargs));
    if (it + 1 < h->svi_maxit) CK(svi_globals(h, h->svi_vi_cur ^ 1, it + 1));
    return 0;
  }
  if (it + 1 < h->svi_maxit) CK(svi_globals(h, h->svi_vi_cur ^ 1, it + 1));
  CK(svi_refresh_emission(h, it, it & 1, h->svi_flags ? (hipEvent_t) nullptr : h->svi_ev[2 * it + 1], it + 1 < h->svi_maxit));
  return 0;
}

// AdaGrad (hmmsgd_metaobs.py:179-183, 1036-1040): the K x K matrix of accumulated squared natural
// parameters of the transition factor joins the resident state; NULL switches the branch off.
int svihmm_svi_set_adagrad(svihmm_ctx* h, const double* ada_G) {
  if (!h || !h->svi_active) return fail("svihmm_svi_set_adagrad: call svihmm_svi_begin first");
  CK(set_device(h));
  if (!ada_G) { h->svi_adagrad = false; return 0; }
  if (h->svi_seq) return fail("svihmm_svi_set_adagrad: AdaGrad is not supported on minibatches of whole sequences (svihmm_svi_sequences)");
  const size_t kk = (size_t)h->svi_K * h->svi_K;
  // ada_G >= 1: the reference starts it at ones and only adds squares (hmmsgd_metaobs.py:179-183,
  // :1036-1040), and the step's weights 1 / ada_G^.25 must stay <= 1 -- a larger weight would let
  // var_tran leave the range svi_begin_common checked for the linear-domain recursions
  for (size_t i = 0; i < kk; ++i)
    if (!(ada_G[i] >= 1.0 && ada_G[i] < 1.7e308)) return fail("svihmm_svi_set_adagrad: ada_G must be finite and >= 1");
  CK(upload_blocks(h, svi_ptr(h, 9), {{ada_G, kk}}));
  h->svi_adagrad = true;               // (only once the accumulator is on its way)
  return 0;
}
int svihmm_svi_read_adagrad(svihmm_ctx* h, double* ada_G_out) {
  if (!h || !h->svi_active || !ada_G_out) return fail("svihmm_svi_read_adagrad: bad arguments");
  if (!h->svi_adagrad) return fail("svihmm_svi_read_adagrad: the loop runs without AdaGrad");
  CK(set_device(h));
  return d2h_sync_small(h, ada_G_out, svi_ptr(h, 9), (size_t)h->svi_K * h->svi_K * sizeof(double));
}

// Everything the loop has in flight is complete and has reached the loop's state: pending ELBO kernels launched,
// all three streams idle and -- when a gate of the loop gave up on the way -- the lost iterations replayed on stream
// events (svi_recover).  Every read of the loop's results starts here.
static int svi_settle(svihmm_ctx* h) {
  CK(svi_flush_elbo(h));
  for (int pass = 0; pass < 2; ++pass) {
    HIPCK(hipStreamSynchronize(h->stream));
    if (h->stream2) HIPCK(hipStreamSynchronize(h->stream2));
    if (h->stream3) HIPCK(hipStreamSynchronize(h->stream3));
    if (!(h->svi_flags && h->pin_status && h->pin_status[1] != 0)) break;
    CK(svi_recover(h, false));
  }
  return 0;
}
// ---- the loop on minibatches of whole declared sequences (include/svihmm.h) ----------------------
// svihmm_svi_sequences: prior_init / var_init join the resident state, the loop leaves the counters for stream order
// and events (what svi_recover(clean) does mid-loop, without counting as a recovery) and from here on steps through
// svihmm_svi_iteration_sequences.
int svihmm_svi_sequences(svihmm_ctx* h, const double* prior_init, const double* var_init) {
  const char* fn = "svihmm_svi_sequences";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!h->svi_active) return bad("no loop: call one of svihmm_svi_begin, _begin_diag, _begin_cat, _begin_mcat, _begin_poisson first");
  if (h->seq_off.empty()) return bad("no sequences declared: call svihmm_set_sequences first");
  if (!prior_init) return bad("prior_init is NULL");
  if (!var_init) return bad("var_init is NULL");
  const int K = h->svi_K;
  // every later var_init is a convex combination of var_init and prior_init + bf q0 (q0 >= 0): none falls below the
  // smaller of the two -- svi_begin_common's argument for var_tran
  for (int k = 0; k < K; ++k) {
    if (!(prior_init[k] >= SVIHMM_SVI_MIN_PSEUDOCOUNT && prior_init[k] < 1.7e308))
      return bad("prior_init[" + std::to_string(k) + "] = " + std::to_string(prior_init[k]) +
                 " is not finite or lies below SVIHMM_SVI_MIN_PSEUDOCOUNT");
    if (!(var_init[k] >= SVIHMM_SVI_MIN_PSEUDOCOUNT && var_init[k] < 1.7e308))
      return bad("var_init[" + std::to_string(k) + "] = " + std::to_string(var_init[k]) +
                 " is not finite or lies below SVIHMM_SVI_MIN_PSEUDOCOUNT");
  }
  if (h->svi_adagrad) return bad("an AdaGrad accumulator is set (svihmm_svi_set_adagrad): not supported on minibatches of whole sequences");
  if (h->comm) return bad("a communicator is attached: multi-GPU minibatches of whole sequences are not supported");
  CK(set_device(h));
  // everything in flight first: begin's globals kernel writes the stationary vector into the slot var_init takes
  CK(svi_settle(h));
  if (h->svi_flags) CK(svi_leave_counters(h));
  CK(upload_blocks(h, svi_ptr(h, 2), {{var_init, (size_t)K}}));
  CK(upload_blocks(h, svi_ptr(h, 10), {{prior_init, (size_t)K}}));
  {   // lgamma(sum_k p_k + eps) - sum_k lgamma(p_k + eps): the prior-only part of the initial factor's energy
    double sum = 0.0, lg = 0.0;
    for (int k = 0; k < K; ++k) { sum += prior_init[k]; lg += std::lgamma(prior_init[k] + 1e-9); }
    h->svi_prior_const_init = std::lgamma(sum + 1e-9) - lg;
  }
  h->svi_seq = true;
  h->svi_vi_cur = 0;
  h->svi_globals_ready = false; h->globals_ev = nullptr;     // (each iteration forms its own globals, in stream order)
  return 0;
}

// G1 of a sequence iteration, main stream: short without the elimination, and the E-step behind it needs no event
static int svi_globals_sequences(svihmm_ctx* h) {
  const int K = h->svi_K;
  CK(svi_globals_buffers(h, h->stream, true));
  {
    ProfScope ps(h, KS_MISC);
    hipLaunchKernelGGL((k_svi_globals_seq<SVI_GW>), dim3(K + 1), dim3(64 * SVI_GW), 0, h->stream,
                       (const double*)svi_ptr(h, 0), (const double*)svi_ptr(h, 2), K, (double*)h->ltran.p,
                       (double*)h->Aexp.p, (double*)h->AexpT.p, (double*)h->mod_init.p);
    HIPCK(hipGetLastError());
  }
  h->globals_ev = nullptr;
  h->K = K; h->have_globals = true; h->lin_stale = true;
  h->exact_log = false; h->f32_ok = h->svi_f32_ok;
  return 0;
}

int svihmm_svi_iteration_sequences(svihmm_ctx* h, int32_t it, const int32_t* idx, int32_t M, uint32_t flags, double rho,
                                   double bfact) {
  const char* fn = "svihmm_svi_iteration_sequences";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (h->have_labels)
    return fail("svihmm_svi_iteration_sequences: labels are in force (svihmm_set_labels) and the resident SVI loop does not "
                "take them; remove them with svihmm_set_labels(h, NULL) or step on the host from "
                "svihmm_estep_sequence_subset's statistics");
  if (h->have_sets)
    return fail("svihmm_svi_iteration_sequences: allowed-state sets are in force (svihmm_set_state_sets) and the "
                "resident SVI loop does not take them; remove them with svihmm_set_state_sets(h, NULL, 0) or step on "
                "the host from svihmm_estep_sequence_subset's statistics");
  if (!h->svi_active) return bad("no loop: call one of svihmm_svi_begin* and svihmm_svi_sequences first");
  if (!h->svi_seq) return bad("the loop steps on windows: call svihmm_svi_sequences first");
  if (it < 0 || it >= h->svi_maxit)
    return bad("it = " + std::to_string(it) + " is outside [0, maxit = " + std::to_string(h->svi_maxit) + ")");
  if (flags & SVIHMM_SVI_KEEP_WINDOW) return bad("SVIHMM_SVI_KEEP_WINDOW is not supported (the iteration has no windows)");
  if (!(std::fabs(rho) < 1.7e308)) return bad("rho is not finite");
  if (!(std::fabs(bfact) < 1.7e308)) return bad("bfact is not finite");
  // (the globals are the loop's own: formed below from the resident factors)
  h->K = h->svi_K; h->have_globals = true;
  SubsetPlan p;
  CK(subset_plan(h, fn, idx, M, flags, p));
  CK(set_device(h));
  const int K = h->svi_K, D = h->svi_D;
  h->svi_cur_it = it;
  if ((int)h->svi_it_events.size() < h->svi_maxit) h->svi_it_events.resize(h->svi_maxit, (char)0);
  h->svi_it_events[it] = (char)1;
  // start of the iteration: the previous iteration's end marker while that iteration still runs (svi_iteration_impl)
  if ((int)h->svi_ev_begin.size() < h->svi_maxit) h->svi_ev_begin.resize(h->svi_maxit, 0);
  h->svi_ev_begin[it] = 2 * it;
  if (it > 0 && h->svi_last_it == it - 1 && hipEventQuery(h->svi_ev[2 * it - 1]) == hipErrorNotReady)
    h->svi_ev_begin[it] = 2 * it - 1;
  else
    HIPCK(hipEventRecord(h->svi_ev[2 * it], h->stream));
  (void)hipGetLastError();            // (hipErrorNotReady is not an error here)
  h->svi_last_it = it;
  CK(svi_globals_sequences(h));
  CK(subset_enqueue(h, p, M, flags, true));
  // the previous iteration's ELBO kernels (their own stream) read var_tran / var_init / theta / logdet, which the step
  // and the theta builder rewrite: the stream waits for their event
  CK(wait_vlb(h));
  const bool merged = h->svi_family == EF_NIW && step_theta_ok(h, K, D);
  const unsigned ntran = (unsigned)((K * K + 255) / 256);
  const SviSeqStep sq = svi_seq_args(h, M);
  double* lb_keep = svi_ptr(h, 8) + (it & 1);
  SviStepArgs sargs = {(const double*)h->packed.p, (const double*)svi_ptr(h, 1), svi_ptr(h, 0), (const double*)h->svi_prior.p,
                       rho, bfact, bfact, 1.0, lb_keep, (double*)nullptr, SviSync{}, sq};
  if (!merged) {
    ProfScope ps(h, KS_MISC);
    if (h->svi_family == EF_NIW)
      hipLaunchKernelGGL(k_svi_global_step, dim3((unsigned)K + ntran), dim3(256), (size_t)3 * D * sizeof(double), h->stream,
                         sargs.packed, sargs.prior_tran, sargs.var_tran, (double*)h->niw.p, sargs.prior, K, D, rho, bfact,
                         bfact, 1.0, lb_keep, (double*)nullptr, SviSync{}, sq);
    else {
      const int W = svi_step_width(h);
      const unsigned nem = (unsigned)(((size_t)K * W + 255) / 256);
      hipLaunchKernelGGL(k_svi_global_step_simple, dim3(nem + ntran), dim3(256), 0, h->stream, (int)h->svi_family,
                         sargs.packed, sargs.prior_tran, sargs.var_tran, (double*)h->niw.p, sargs.prior, K, W, rho, bfact,
                         bfact, 1.0, lb_keep, (double*)nullptr, (int)nem, SviSync{}, sq);
    }
    HIPCK(hipGetLastError());
  }
  // lower bound of var_tran after the step: (1 - rho) v + rho (prior_tran + bf A_raw) >= (1 - rho) bound + rho
  if (rho >= 0.0 && rho <= 1.0) {
    h->svi_vmin = (1.0 - rho) * h->svi_vmin + rho;
    h->svi_f32_ok = h->svi_vmin > 0.05;
  }
  // theta / table of the new factors (with the step in the same launch where the window loop merges them), then the
  // ELBO kernels on their own stream behind the iteration's end marker
  return svi_refresh_emission(h, it, it & 1, h->svi_ev[2 * it + 1], false, merged ? &sargs : nullptr);
}

int svihmm_svi_read_elbo(svihmm_ctx* h, int32_t n, double* out_elbo, double* out_ms) {
  if (!h || !h->svi_active || n < 0 || n > h->svi_maxit) return fail("svihmm_svi_read_elbo: bad arguments");
  CK(set_device(h));
  CK(svi_settle(h));
  CK(check_emission_status(h));
  for (int i = 0; i < n; ++i) {
    if (out_elbo) out_elbo[i] = h->svi_elbo[i];
    // (per iteration: a loop that left the counters mid-way timed its later iterations with events)
    if (out_ms && !((int)h->svi_it_events.size() > i && h->svi_it_events[i])) {
      // device wall-clock stamps: begin (k_svi_stamp, or the previous iteration's end) to the theta builder's end
      const int bi = (int)h->svi_ev_begin.size() > i ? h->svi_ev_begin[i] : 2 * i;
      const unsigned long long t0 = h->svi_ts[bi], t1 = h->svi_ts[2 * i + 1];
      out_ms[i] = (t0 && t1 && t1 >= t0) ? (double)(t1 - t0) / h->wall_clock_khz : NAN;
    } else if (out_ms) {
      float ms = 0.f;
      out_ms[i] = hipEventElapsedTime(&ms, h->svi_ev[(int)h->svi_ev_begin.size() > i ? h->svi_ev_begin[i] : 2 * i], h->svi_ev[2 * i + 1]) == hipSuccess ? (double)ms : NAN;
    }
  }
  return 0;
}

int svihmm_svi_read_state(svihmm_ctx* h, double* var_tran, double* var_init, double* mu, double* sigma,
                          double* kappa, double* nu) {
  if (!h || !h->svi_active) return fail("svihmm_svi_read_state: no SVI state on the device");
  if (h->svi_family != EF_NIW) return fail("svihmm_svi_read_state: NIW layout; this loop's family reads through svihmm_svi_read_factors");
  CK(set_device(h));
  CK(svi_settle(h));
  const size_t K = h->svi_K, D = h->svi_D, nmu = K * D, nsg = K * D * D;
  const double* nw = (const double*)h->niw.p;
  if (var_tran) CK(d2h(h, var_tran, svi_ptr(h, 0), K * K * 8));
  CK(wait_globals(h));
  if (var_init) CK(d2h(h, var_init, svi_ptr(h, h->svi_vi_cur ? 7 : 2), K * 8));
  if (mu) CK(d2h(h, mu, nw, nmu * 8));
  if (sigma) CK(d2h(h, sigma, nw + nmu, nsg * 8));
  if (kappa) CK(d2h(h, kappa, nw + nmu + nsg, K * 8));
  if (nu) CK(d2h(h, nu, nw + nmu + nsg + K, K * 8));
  HIPCK(hipStreamSynchronize(h->stream));
  if (h->stream3) HIPCK(hipStreamSynchronize(h->stream3));   // ELBO kernels still reading niw / theta
  h->vlb_pending = false;
  if (mu) from_centred(h, mu, (int)K, (int)D);
  CK(check_emission_status(h));
  return 0;
}

// The loop's state in the family's own block layout: NIW [mu | sigma | kappa | nu], diagonal
// [mu | nus | alphas | betas] (each [K][D]), Categorical alpha[K][V], multi-column Categorical alpha[K][F], Poisson
// [a | b] (each [K][D]); means in the caller's coordinates.
int svihmm_svi_read_factors(svihmm_ctx* h, double* var_tran, double* var_init, double* factors_out) {
  if (!h || !h->svi_active) return fail("svihmm_svi_read_factors: no SVI state on the device");
  CK(set_device(h));
  CK(svi_settle(h));
  const size_t K = h->svi_K, D = h->svi_D;
  const size_t n = h->svi_family == EF_NIW ? K * D + K * D * D + 2 * K : h->svi_family == EF_DIAG ? 4 * K * D : K * (size_t)h->V;
  if (var_tran) CK(d2h(h, var_tran, svi_ptr(h, 0), K * K * 8));
  CK(wait_globals(h));
  if (var_init) CK(d2h(h, var_init, svi_ptr(h, h->svi_vi_cur ? 7 : 2), K * 8));
  if (factors_out) CK(d2h(h, factors_out, h->niw.p, n * 8));
  HIPCK(hipStreamSynchronize(h->stream));
  if (h->stream3) HIPCK(hipStreamSynchronize(h->stream3));   // ELBO kernels still reading the factors
  h->vlb_pending = false;
  if (factors_out && fam_gaussian(h->svi_family)) from_centred(h, factors_out, (int)K, (int)D);
  CK(check_emission_status(h));
  return 0;
}

// The globals the recursions currently hold (log domain): what svihmm_set_globals uploaded last, or
// what the device-resident loop's last iteration computed from var_tran (the reference leaves that
// iteration's psi-expectations on the object: hmmsgd_metaobs.py:502-504).
int svihmm_read_globals(svihmm_ctx* h, double* mod_init_out, double* ltran_out) {
  if (!h || (!mod_init_out && !ltran_out)) return fail("svihmm_read_globals: bad arguments");
  if (!h->have_globals) return fail("svihmm_read_globals: no globals on the device");
  CK(set_device(h));
  CK(wait_globals(h));
  const size_t K = h->K;
  if (mod_init_out) CK(d2h(h, mod_init_out, h->mod_init.p, K * 8));
  if (ltran_out) CK(d2h(h, ltran_out, h->ltran.p, K * K * 8));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

int svihmm_read_packed(svihmm_ctx* h, double* out_packed) {
  if (!h || !out_packed) return fail("svihmm_read_packed: bad arguments");
  if (!h->have_packed) return fail("svihmm_read_packed: no statistics computed yet");
  CK(set_device(h));
  CK(read_packed_host(h, out_packed));
  CK(check_emission_status(h));
  return 0;
}

int svihmm_read_intermediate(svihmm_ctx* h, int32_t what, double* out) {
  if (!h || !out) return fail("svihmm_read_intermediate: bad arguments");
  if (h->lastB <= 0) return fail("svihmm_read_intermediate: nothing computed yet");
  CK(set_device(h));
  if (what < 0 || what > 3) return fail("svihmm_read_intermediate: bad selector");
  const int64_t rows = (int64_t)h->lastB * h->lastLm;
  const double* src = nullptr;
  CK(intermediate_ptr(h, what, 0, rows, &src));
  CK(d2h(h, out, src, (size_t)rows * h->K * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

int svihmm_read_rows(svihmm_ctx* h, int32_t what, int64_t row0, int64_t nrows, double* out) {
  if (!h || !out || row0 < 0 || nrows <= 0) return fail("svihmm_read_rows: bad arguments");
  if (h->lastB <= 0) return fail("svihmm_read_rows: nothing computed yet");
  if (what < 0 || what > 3) return fail("svihmm_read_rows: bad selector");
  if (row0 + nrows > (int64_t)h->lastB * h->lastLm) return fail("svihmm_read_rows: out of range");
  CK(set_device(h));
  const double* src = nullptr;
  CK(intermediate_ptr(h, what, row0, nrows, &src));
  CK(d2h(h, out, src, (size_t)nrows * h->K * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- held-out log-probability against the posterior batch held (kernels_heldout.h) -------------
// Everything that can be wrong with a call is found before any device work.  The batch held: what the last
// E-step-type call left (post_kind; prepare_ll drops it, so a decoder, svihmm_loglik or svihmm_grow_windows since
// then means "none"), with the K it was computed with.
static int heldout_batch(const svihmm_ctx* h, const char* fn, int64_t* nrows_out) {
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (h->post_kind == 0 || h->lastB <= 0 || h->dec_result)
    return bad("no posterior batch held: call svihmm_forward_backward, svihmm_estep_minibatch(_ex), "
               "svihmm_estep_sequences or svihmm_estep_sequence_subset first (a decoder, svihmm_loglik or "
               "svihmm_grow_windows call since the last of them has dropped its batch)");
  if (h->K != h->post_K)
    return bad("the globals' K (" + std::to_string(h->K) + ") is not the K of the posterior batch held (" +
               std::to_string(h->post_K) + "): run the E-step again");
  if (h->K > 256) return bad("K = " + std::to_string(h->K) + " > 256 not supported");
  *nrows_out = (int64_t)h->lastB * h->lastLm;
  return 0;
}
// for the call's duration the handle's resident rows are the gathered copy svihmm_estep_sequence_subset left
// (its own rows and mask bytes, R of them): what launch_emission reads
struct GatheredRows {
  svihmm_ctx* h; int64_t T; bool on;
  GatheredRows(svihmm_ctx* h_, bool on_, int64_t R) : h(h_), T(h_->T), on(on_) {
    if (on) { std::swap(h->obs, h->sub_obs); std::swap(h->mask, h->sub_mask); h->T = R; }
  }
  ~GatheredRows() {
    if (on) { std::swap(h->obs, h->sub_obs); std::swap(h->mask, h->sub_mask); h->T = T; }
  }
};
// the partials' sum and the results back: out2 = {mean, count}, out_lp[n] when asked for
static int heldout_finish(svihmm_ctx* h, int nblk, double* part, const double* dlp, int64_t n, double out2[2], double* out_lp) {
  hipLaunchKernelGGL(k_pred_final, dim3(1), dim3(64), 0, h->stream, (const double*)part, nblk, part + 2 * nblk);
  HIPCK(hipGetLastError());
  CK(d2h(h, out2, part + 2 * nblk, 2 * sizeof(double)));
  if (out_lp) CK(d2h(h, out_lp, dlp, (size_t)n * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}
#define HELDOUT_KT(L)                                                                                 \
  do {                                                                                                \
    if (K <= 16) L(1); else if (K <= 32) L(2); else if (K <= 48) L(3); else if (K <= 64) L(4);        \
    else if (K <= 128) L(8); else L(16);                                                              \
  } while (0)

int svihmm_heldout_rows(svihmm_ctx* h, double out2[2], double* out_lp) {
  const char* fn = "svihmm_heldout_rows";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!out2) return bad("out2 is NULL");
  int64_t n = 0;
  CK(heldout_batch(h, fn, &n));
  if (h->last_host_ll)
    return bad("the posterior batch held ran on host lliks (SVIHMM_USE_HOST_LLIKS): it has no true observation to score");
  if (!h->have_emission)
    return bad("no emission family: call svihmm_set_emission_niw / _diag / _cat / _mcat / _poisson / _pgauss first");
  if (emission_family_id(h) != h->post_fam)
    return bad("the emission family is not the one the posterior batch held was computed with: run the E-step again");
  if (h->eK != h->K)
    return bad("K of the globals (" + std::to_string(h->K) + ") differs from the emission family's K (" +
               std::to_string(h->eK) + ")");
  if (h->eD != h->D) return bad(emission_d_message(h));
  if (!h->have_mask) {               // nothing can be masked: no launch
    out2[0] = NAN; out2[1] = 0.0;
    if (out_lp) for (int64_t g = 0; g < n; ++g) out_lp[g] = NAN;
    return 0;
  }
  CK(set_device(h));
  CK(wait_side_streams(h));
  const int K = h->K;
  const double* q = nullptr;
  CK(intermediate_ptr(h, 3, 0, n, &q));
  const int nblk = (int)((n + HELDOUT_PER_BLOCK - 1) / HELDOUT_PER_BLOCK);
  // heldout: [ zero (the identity map's window start), 16 bytes | out_lp n | partials 2 nblk + 2 ]
  CK(ensure(h->heldout, 16 + ((size_t)n + 2 * (size_t)nblk + 2) * sizeof(double)));
  CK(ensure(h->m_ll, (size_t)n * K * sizeof(double)));
  h->m_nb = 0;
  const int64_t* zero = (const int64_t*)h->heldout.p;
  double* dlp = (double*)((char*)h->heldout.p + 16);
  double* part = dlp + n;
  HIPCK(hipMemsetAsync(h->heldout.p, 0, 16, h->stream));
  {
    // the family's llik of the batch rows' true values (no masking), always fp64, into the side buffer; a window
    // batch through its own starts, the two sequence kinds as one window over the rows from 0
    GatheredRows view(h, h->post_kind == 3, n);
    const bool windows = h->post_kind == 1;
    if (windows) CK(ensure_starts_pulled(h));
    const bool cur_f32 = h->cur_f32;
    h->cur_f32 = false;
    const uint32_t fl = windows ? h->last_flags & ~(uint32_t)(SVIHMM_MASK_AS_NAN | SVIHMM_USE_HOST_LLIKS) : 0u;
    const int rc = launch_emission(h, windows ? h->lastB : 1, windows ? h->lastLm : (int)n, fl, false,
                                   windows ? nullptr : zero, (double*)h->m_ll.p, nullptr, nullptr, 0, nullptr,
                                   false);      // (the family's own llik of the true rows: no label clamp)
    h->cur_f32 = cur_f32;
    if (rc) return rc;
    ProfScope ps(h, KS_MISC);
#define HR(KT) hipLaunchKernelGGL(k_heldout_rows<KT>, dim3(nblk), dim3(256), 0, h->stream, q, (const double*)h->m_ll.p, \
                                  (const uint8_t*)h->mask.p, windows ? (const int64_t*)h->starts.p : (const int64_t*)nullptr, \
                                  n, h->lastLm, K, out_lp ? dlp : (double*)nullptr, part)
    HELDOUT_KT(HR);
#undef HR
    HIPCK(hipGetLastError());
  }
  CK(heldout_finish(h, nblk, part, dlp, n, out2, out_lp));
  return check_emission_status(h);
}

int svihmm_heldout_entries(svihmm_ctx* h, int64_t n, const int64_t* row, const int32_t* col, const double* val,
                           double out2[2], double* out_lp) {
  const char* fn = "svihmm_heldout_entries";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!out2) return bad("out2 is NULL");
  if (n < 0) return bad("n = " + std::to_string(n) + " must not be negative");
  if (n > 0 && (!row || !col || !val)) return bad("row, col and val must be given when n > 0");
  int64_t nrows = 0;
  CK(heldout_batch(h, fn, &nrows));
  if (!h->have_emission || !fam_entrywise(h->fam))
    return bad("entry-wise scores are defined for the families that skip single entries: besides the Gaussian tracks "
               "of svihmm_set_emission_pgauss, the multi-column Categorical and the Poisson family only "
               "(svihmm_set_emission_mcat / svihmm_set_emission_poisson); svihmm_heldout_rows takes every family");
  if (h->eK != h->K)
    return bad("K of the globals (" + std::to_string(h->K) + ") differs from the emission family's K (" +
               std::to_string(h->eK) + ")");
  const int K = h->K, D = h->eD;
  for (int64_t e = 0; e < n; ++e) {
    if (row[e] < 0 || row[e] >= nrows)
      return bad("row[" + std::to_string(e) + "] = " + std::to_string(row[e]) + " is outside [0, nrows = " +
                 std::to_string(nrows) + ")");
    if (col[e] < 0 || col[e] >= D)
      return bad("col[" + std::to_string(e) + "] = " + std::to_string(col[e]) + " is outside [0, D = " +
                 std::to_string(D) + ")");
  }
  if (n == 0) { out2[0] = NAN; out2[1] = 0.0; return 0; }
  CK(set_device(h));
  CK(wait_side_streams(h));
  const double* q = nullptr;
  CK(intermediate_ptr(h, 3, 0, nrows, &q));
  const int64_t nblk64 = (n + HELDOUT_PER_BLOCK - 1) / HELDOUT_PER_BLOCK;
  if (nblk64 > 0x3fffffff) return bad("n = " + std::to_string(n) + " entries are too many for one launch");
  const int nblk = (int)nblk64;
  // heldout: [ zero, 16 bytes | out_lp n | partials 2 nblk + 2 | row n int64 | val n | col n int32 ]
  CK(ensure(h->heldout, 16 + (3 * (size_t)n + 2 * (size_t)nblk + 2) * sizeof(double) + (size_t)n * sizeof(int32_t)));
  double* dlp = (double*)((char*)h->heldout.p + 16);
  double* part = dlp + n;
  int64_t* drow = (int64_t*)(part + 2 * (size_t)nblk + 2);
  double* dval = (double*)(drow + n);
  int32_t* dcol = (int32_t*)(dval + n);
  CK(upload_staged(h, drow, row, (size_t)n * sizeof(int64_t)));
  CK(upload_staged(h, dval, val, (size_t)n * sizeof(double)));
  CK(upload_staged(h, dcol, col, (size_t)n * sizeof(int32_t)));
  {
    ProfScope ps(h, KS_MISC);
#define HE(KT)                                                                                                         \
  do {                                                                                                                 \
    if (h->fam == EF_PGAUSS)                                                                                           \
      hipLaunchKernelGGL((k_heldout_entries<KT, 2>), dim3(nblk), dim3(256), 0, h->stream, q, (const int64_t*)drow,     \
                         (const int32_t*)dcol, (const double*)dval, n, K, D, (const double*)h->cat_table.p,            \
                         (const int*)nullptr, (const double*)nullptr, 0, out_lp ? dlp : (double*)nullptr, part);       \
    else if (h->fam == EF_POIS)                                                                                        \
      hipLaunchKernelGGL((k_heldout_entries<KT, 1>), dim3(nblk), dim3(256), 0, h->stream, q, (const int64_t*)drow,     \
                         (const int32_t*)dcol, (const double*)dval, n, K, D, (const double*)h->cat_table.p,            \
                         (const int*)nullptr, (const double*)h->pois_logfact.p, h->pois_C,                             \
                         out_lp ? dlp : (double*)nullptr, part);                                                       \
    else                                                                                                               \
      hipLaunchKernelGGL((k_heldout_entries<KT, 0>), dim3(nblk), dim3(256), 0, h->stream, q, (const int64_t*)drow,     \
                         (const int32_t*)dcol, (const double*)dval, n, K, D, (const double*)h->cat_table.p,            \
                         (const int*)h->mcat_meta.p, (const double*)nullptr, 0, out_lp ? dlp : (double*)nullptr, part);\
  } while (0)
    HELDOUT_KT(HE);
#undef HE
    HIPCK(hipGetLastError());
  }
  return heldout_finish(h, nblk, part, dlp, n, out2, out_lp);
}
#undef HELDOUT_KT

// ---- posterior expectations of per-state tables against the posterior batch held (kernels_expect.h) ----------
// heldout_batch's contract: no E-step, always fp64, K <= 256; everything that can be wrong is found before any device
// work.  The emission family is not asked for and the resident rows are not read: a batch on host lliks is taken.
// (var_x is handed out as doubles whatever mode computed the batch -- intermediate_ptr(h, 3): ensure_q writes fp64
//  rows in the fp32 mode too -- so no batch has to be refused for its precision.)
static int expect_table_check(const char* fn, int K, int F, const double* table) {
  for (int k = 0; k < K; ++k)
    for (int f = 0; f < F; ++f)
      if (!std::isfinite(table[(size_t)k * F + f]))
        return fail(std::string(fn) + ": table[" + std::to_string(k) + "][" + std::to_string(f) + "] is not finite");
  return 0;
}
// rows of one pass of the dense call: the device copy of the result is at most this large, a call on more rows
// runs the kernel pass by pass (a row's bits do not depend on where it sits in a launch)
#define EXPECT_OUT_BYTES ((size_t)256 << 20)

int svihmm_posterior_expect(svihmm_ctx* h, int32_t F, const double* table, double* out) {
  const char* fn = "svihmm_posterior_expect";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!table) return bad("table is NULL");
  if (!out) return bad("out is NULL");
  if (F < 1 || F > SVIHMM_MCAT_MAX_F)
    return bad("F = " + std::to_string(F) + " is outside [1, " + std::to_string(SVIHMM_MCAT_MAX_F) + "]");
  int64_t nrows = 0;
  CK(heldout_batch(h, fn, &nrows));
  const int K = h->K;
  CK(expect_table_check(fn, K, F, table));
  CK(set_device(h));
  CK(wait_side_streams(h));
  const double* q = nullptr;
  CK(intermediate_ptr(h, 3, 0, nrows, &q));
  // the widest feature group (16 NT features) whose staged slice leaves room for two workgroups on a CU
  const int Kpad = (K + EXPECT_KC - 1) / EXPECT_KC * EXPECT_KC;
  const auto lds_of = [Kpad](int nt) { return (size_t)Kpad * (16 * nt + EXPECT_LD_PAD) * sizeof(double); };
  int NT = F > 32 ? 4 : F > 16 ? 2 : 1;
  while (NT > 1 && lds_of(NT) > (size_t)72 << 10) NT >>= 1;
  const size_t lds = lds_of(NT);
  const int VEC = K % 4 == 0 ? 4 : K % 2 == 0 ? 2 : 1;
  const int64_t pass_rows = std::max<int64_t>(EXPECT_ROWS, (int64_t)(EXPECT_OUT_BYTES / ((size_t)F * sizeof(double))) /
                                                             EXPECT_ROWS * EXPECT_ROWS);
  const size_t tb = ((size_t)K * F * sizeof(double) + 255) & ~(size_t)255;
  // heldout: [ table K F (to 256 bytes) | result of one pass ]
  CK(ensure(h->heldout, tb + (size_t)std::min(nrows, pass_rows) * F * sizeof(double)));
  double* dtab = (double*)h->heldout.p;
  double* dout = (double*)((char*)h->heldout.p + tb);
  CK(upload_staged(h, dtab, table, (size_t)K * F * sizeof(double)));
  // workgroups a CU holds at once: the registers allow 3 (NT = 4: 150 VGPRs) or 4 waves per SIMD, the LDS the rest
  const int wgs_per_cu = (int)std::min<size_t>(NT == 4 ? 3 : 4, ((size_t)160 << 10) / lds);
  for (int64_t r0 = 0; r0 < nrows; r0 += pass_rows) {
    const int64_t nr = std::min(pass_rows, nrows - r0);
    const int64_t wg_tiles = (nr + 4 * EXPECT_ROWS - 1) / (4 * EXPECT_ROWS);
    const dim3 grid((unsigned)std::min<int64_t>(wg_tiles, (int64_t)std::max(h->ncu, 1) * wgs_per_cu),
                    (unsigned)((F + 16 * NT - 1) / (16 * NT)));
    {
      ProfScope ps(h, KS_MISC);
#define PE(NTV, VV)                                                                                                 \
  do {                                                                                                              \
    if (lds > ((size_t)64 << 10))                                                                                   \
      HIPCK(hipFuncSetAttribute((const void*)k_posterior_expect<NTV, VV>, hipFuncAttributeMaxDynamicSharedMemorySize, \
                                (int)lds));                                                                         \
    hipLaunchKernelGGL((k_posterior_expect<NTV, VV>), grid, dim3(256), lds, h->stream, q + (size_t)r0 * K,          \
                       (const double*)dtab, nr, K, (int)F, dout);                                                   \
  } while (0)
#define PEV(NTV) do { if (VEC == 4) PE(NTV, 4); else if (VEC == 2) PE(NTV, 2); else PE(NTV, 1); } while (0)
      if (NT == 4) PEV(4); else if (NT == 2) PEV(2); else PEV(1);
#undef PEV
#undef PE
      HIPCK(hipGetLastError());
    }
    CK(d2h(h, out + (size_t)r0 * F, dout, (size_t)nr * F * sizeof(double)));
    if (r0 + pass_rows < nrows) HIPCK(hipStreamSynchronize(h->stream));   // (the next pass rewrites the device copy)
  }
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

int svihmm_posterior_expect_entries(svihmm_ctx* h, int32_t F, const double* table, int64_t n, const int64_t* row,
                                    const int32_t* col, double* out) {
  const char* fn = "svihmm_posterior_expect_entries";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (!table) return bad("table is NULL");
  if (!out) return bad("out is NULL");
  if (F < 1 || F > SVIHMM_MCAT_MAX_F)
    return bad("F = " + std::to_string(F) + " is outside [1, " + std::to_string(SVIHMM_MCAT_MAX_F) + "]");
  if (n < 0) return bad("n = " + std::to_string(n) + " must not be negative");
  if (n > 0 && (!row || !col)) return bad("row and col must be given when n > 0");
  int64_t nrows = 0;
  CK(heldout_batch(h, fn, &nrows));
  for (int64_t e = 0; e < n; ++e) {
    if (row[e] < 0 || row[e] >= nrows)
      return bad("row[" + std::to_string(e) + "] = " + std::to_string(row[e]) + " is outside [0, nrows = " +
                 std::to_string(nrows) + ")");
    if (col[e] < 0 || col[e] >= F)
      return bad("col[" + std::to_string(e) + "] = " + std::to_string(col[e]) + " is outside [0, F = " +
                 std::to_string(F) + ")");
  }
  const int K = h->K;
  CK(expect_table_check(fn, K, F, table));
  if (n == 0) return 0;
  const int64_t nblk = (n + 255) / 256;
  if (nblk > 0x3fffffff) return bad("n = " + std::to_string(n) + " entries are too many for one launch");
  CK(set_device(h));
  CK(wait_side_streams(h));
  const double* q = nullptr;
  CK(intermediate_ptr(h, 3, 0, nrows, &q));
  const size_t tb = ((size_t)K * F * sizeof(double) + 255) & ~(size_t)255;
  // heldout: [ table K F (to 256 bytes) | out n | row n int64 | col n int32 ]
  CK(ensure(h->heldout, tb + 2 * (size_t)n * sizeof(double) + (size_t)n * sizeof(int32_t)));
  double* dtab = (double*)h->heldout.p;
  double* dout = (double*)((char*)h->heldout.p + tb);
  int64_t* drow = (int64_t*)(dout + n);
  int32_t* dcol = (int32_t*)(drow + n);
  CK(upload_staged(h, dtab, table, (size_t)K * F * sizeof(double)));
  CK(upload_staged(h, drow, row, (size_t)n * sizeof(int64_t)));
  CK(upload_staged(h, dcol, col, (size_t)n * sizeof(int32_t)));
  {
    ProfScope ps(h, KS_MISC);
    hipLaunchKernelGGL(k_posterior_expect_entries, dim3((unsigned)nblk), dim3(256), 0, h->stream, q,
                       (const int64_t*)drow, (const int32_t*)dcol, (const double*)dtab, n, K, (int)F, dout);
    HIPCK(hipGetLastError());
  }
  CK(d2h(h, out, dout, (size_t)n * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

int svihmm_state_argmax(svihmm_ctx* h, const int32_t* true_sts, int32_t* out_z,
                        int64_t* out_conf) {
  if (!h || (!out_z && !out_conf)) return fail("svihmm_state_argmax: bad arguments");
  if (out_conf && !true_sts) return fail("svihmm_state_argmax: the count matrix needs true_sts");
  if (h->lastB <= 0) return fail("svihmm_state_argmax: nothing computed yet");
  CK(set_device(h));
  const int K = h->K;
  const int64_t n = (int64_t)h->lastB * h->lastLm;
  const double* q = nullptr;
  CK(intermediate_ptr(h, 3, 0, n, &q));
  const size_t zb = ((size_t)n * sizeof(int32_t) + 15) & ~(size_t)15;
  const size_t cb = (size_t)K * K * sizeof(unsigned long long);
  CK(ensure(h->scratch, 2 * zb + cb));
  int32_t* dz = (int32_t*)h->scratch.p;
  int32_t* dtrue = (int32_t*)((char*)h->scratch.p + zb);
  unsigned long long* dconf = (unsigned long long*)((char*)h->scratch.p + 2 * zb);
  if (true_sts) {
    HIPCK(hipMemcpyAsync(dtrue, true_sts, (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
    HIPCK(hipMemsetAsync(dconf, 0, cb, h->stream));
  }
  {
    ProfScope ps(h, KS_MISC);
    const int nblk = (int)((n + ARGMAX_ROWS_PER_BLOCK - 1) / ARGMAX_ROWS_PER_BLOCK);
    const size_t lds = (true_sts && K <= 64) ? (size_t)K * K * sizeof(unsigned int) : 0;
    hipLaunchKernelGGL(k_state_argmax, dim3(nblk), dim3(256), lds, h->stream, q, n, K,
                       (const int32_t*)(true_sts ? dtrue : nullptr), dz, dconf);
    HIPCK(hipGetLastError());
  }
  if (out_z) CK(d2h(h, out_z, dz, (size_t)n * sizeof(int32_t)));
  if (out_conf) CK(d2h(h, out_conf, dconf, cb));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}


// ---- Viterbi / MAP state paths (kernels_viterbi.h) -------------------------------------------
// Everything that can be wrong with the call is found here, before any device work; the lliks are then
// produced exactly as svihmm_loglik produces them (prepare_ll) and decoded by launch_viterbi.
int svihmm_viterbi(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                   int32_t* out_z, double* out_score) {
  if (!h) return fail("svihmm_viterbi: NULL handle");
  if (!out_z && !out_score) return fail("svihmm_viterbi: neither out_z nor out_score given");
  if (!h->have_globals) return fail("svihmm_viterbi: no globals: call svihmm_set_globals first");
  if (h->K > 256)
    return fail("svihmm_viterbi: K = " + std::to_string(h->K) + " > 256 not supported (one-byte back-pointers)");
  if (B < 1 || Lm < 1) return fail("svihmm_viterbi: B and Lm must be positive");
  CK(check_window_call(h, "svihmm_viterbi", starts, B, Lm, flags));
  CK(set_device(h));
  CK(wait_side_streams(h));
  CK(prepare_ll(h, starts, B, Lm, flags & (SVIHMM_MASK_AS_NAN | SVIHMM_USE_HOST_LLIKS), false));
  h->lastB = B; h->lastLm = Lm;
  int32_t* dz = nullptr;
  double* dscore = nullptr;
  CK(launch_viterbi(h, B, Lm, (const double*)h->ll.p, out_z != nullptr, &dz, &dscore));
  if (out_z) CK(d2h(h, out_z, dz, (size_t)B * Lm * sizeof(int32_t)));
  if (out_score) CK(d2h(h, out_score, dscore, (size_t)B * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  return 0;
}


// ---- FFBS for window batches x draws (kernels_ffbs_windows.h) ---------------------------------
// Everything that can be wrong with the call is found here, before any device work; the filter and the draws
// are launch_ffbs_windows' (tu_recursion.hip).
// logA[k][z_next]: -inf is probability zero; every column needs one finite entry to draw from
static int check_logA(const char* fn, const double* logA, int K) {
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  for (int j = 0; j < K; ++j) {
    bool any = false;
    for (int k = 0; k < K; ++k) {
      const double v = logA[(size_t)k * K + j];
      if (v != v || v == INFINITY) return bad("logA[" + std::to_string(k) + "][" + std::to_string(j) + "] is NaN or +inf");
      any = any || v > -INFINITY;
    }
    if (!any) return bad("column " + std::to_string(j) + " of logA has no finite entry");
  }
  return 0;
}
int svihmm_ffbs_windows(svihmm_ctx* h, const int64_t* starts, int32_t B, int32_t Lm, uint32_t flags,
                        const double* logA, int32_t S, const double* uniforms, uint64_t seed,
                        int32_t* out_z, double* out_lalpha) {
  if (!h) return fail("svihmm_ffbs_windows: NULL handle");
  if (!logA || !out_z) return fail("svihmm_ffbs_windows: logA and out_z must be given");
  if (S < 1 || B < 1 || Lm < 1) return fail("svihmm_ffbs_windows: S, B and Lm must be positive");
  if ((int64_t)S * B >= ((int64_t)1 << 31)) return fail("svihmm_ffbs_windows: S * B too large");
  if (!h->have_globals) return fail("svihmm_ffbs_windows: no globals: call svihmm_set_globals first");
  const int K = h->K;
  if (K > 256) return fail("svihmm_ffbs_windows: K = " + std::to_string(K) + " > 256 not supported");
  CK(check_window_call(h, "svihmm_ffbs_windows", starts, B, Lm, flags));
  CK(check_logA("svihmm_ffbs_windows", logA, K));
  CK(set_device(h));
  CK(wait_side_streams(h));
  int32_t* dz = nullptr;
  const double* dla = nullptr;
  {
    ReportHold hold(h, false, false);
    CK(launch_ffbs_windows(h, starts, B, Lm, flags & (SVIHMM_MASK_AS_NAN | SVIHMM_USE_HOST_LLIKS), logA, S, uniforms,
                           seed, out_lalpha != nullptr, &dz, &dla));
  }
  CK(d2h(h, out_z, dz, (size_t)S * B * Lm * sizeof(int32_t)));
  if (out_lalpha) CK(d2h(h, out_lalpha, dla, (size_t)B * Lm * K * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  return 0;
}


// ---- decoding all declared sequences in one call (kernels_decode_sequences.h) --------------------
// Everything that can be wrong with the call is found here, before any device work.  Both calls evaluate the lliks
// of all T rows in one emission pass (prepare_ll over the window [0, T) with the boundary check lifted, as
// estep_sequences_core lifts it for its row ranges); host lliks must be the [1][T][K] batch of the concatenated rows.
static int check_decode_sequences(const svihmm_ctx* h, const char* fn, uint32_t flags) {
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (h->seq_off.empty()) return bad("no sequences declared: call svihmm_set_sequences first");
  if (!h->have_globals) return bad("no globals: call svihmm_set_globals first");
  if (flags & SVIHMM_USE_HOST_LLIKS) {
    if (!h->have_host_ll || h->hostB != 1 || h->hostLm != h->T)
      return bad("SVIHMM_USE_HOST_LLIKS without uploaded lliks of shape [1, T, K] (svihmm_set_lliks)");
  } else {
    CK(check_window_model(h, fn));
  }
  if (h->K > 256) return bad("K = " + std::to_string(h->K) + " > 256 not supported");
  if (h->T > 2147483647LL) return bad("T = " + std::to_string(h->T) + " rows are too many (T <= 2^31 - 1)");
  return 0;
}

int svihmm_viterbi_sequences(svihmm_ctx* h, uint32_t flags, int32_t* out_z, double* out_score) {
  const char* fn = "svihmm_viterbi_sequences";
  if (!h) return fail("svihmm_viterbi_sequences: NULL handle");
  if (!out_z && !out_score) return fail("svihmm_viterbi_sequences: neither out_z nor out_score given");
  CK(check_decode_sequences(h, fn, flags));
  if (out_z && viterbi_sequences_chunks(h) * (h->K <= 64 ? 64 : 256) >= ((int64_t)1 << 31))
    return fail("svihmm_viterbi_sequences: too many row chunks for the map composition");
  CK(set_device(h));
  CK(wait_side_streams(h));
  const int N = (int)h->seq_off.size() - 1;
  const int64_t T = h->T, st0 = 0;
  {
    ReportHold hold(h, true, false);
    CK(prepare_ll(h, &st0, 1, (int)T, flags & (SVIHMM_MASK_AS_NAN | SVIHMM_USE_HOST_LLIKS), false));
  }
  h->lastB = 1; h->lastLm = (int)T;
  h->dec_result = 1;
  int32_t* dz = nullptr;
  double* dscore = nullptr;
  CK(launch_viterbi_sequences(h, (const double*)h->ll.p, out_z != nullptr, &dz, &dscore));
  if (out_z) CK(d2h(h, out_z, dz, (size_t)T * sizeof(int32_t)));
  if (out_score) CK(d2h(h, out_score, dscore, (size_t)N * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  return 0;
}

int svihmm_ffbs_sequences(svihmm_ctx* h, uint32_t flags, const double* logA, int32_t S, const double* uniforms,
                          uint64_t seed, int32_t* out_z, double* out_lalpha) {
  const char* fn = "svihmm_ffbs_sequences";
  if (!h) return fail("svihmm_ffbs_sequences: NULL handle");
  if (!logA || !out_z) return fail("svihmm_ffbs_sequences: logA and out_z must be given");
  if (S < 1) return fail("svihmm_ffbs_sequences: S must be positive");
  CK(check_decode_sequences(h, fn, flags));
  const int K = h->K, N = (int)h->seq_off.size() - 1;
  if ((int64_t)S * N >= ((int64_t)1 << 31)) return fail("svihmm_ffbs_sequences: S * N too large");
  CK(check_logA("svihmm_ffbs_sequences", logA, K));
  CK(set_device(h));
  CK(wait_side_streams(h));
  const int64_t T = h->T;
  int32_t* dz = nullptr;
  const double* dla = nullptr;
  {
    ReportHold hold(h, true, false);
    CK(launch_ffbs_sequences(h, flags & (SVIHMM_MASK_AS_NAN | SVIHMM_USE_HOST_LLIKS), logA, S, uniforms, seed,
                             out_lalpha != nullptr, &dz, &dla));
  }
  h->dec_result = 2;
  CK(d2h(h, out_z, dz, (size_t)S * T * sizeof(int32_t)));
  if (out_lalpha) CK(d2h(h, out_lalpha, dla, (size_t)T * K * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  CK(check_emission_status(h));
  return 0;
}


// ---- growing adaptive windows / buffers (kernels_grow.h) ---------------------------------------
// Everything that can be wrong with the call is found here, before any device work.
//   product route: one emission pass over the rows every centre can reach (n windows of one common length W, clamped
//     into [0, T)), then ONE launch of k_grow_products;
//   literal route: per candidate half-width the E-step of svihmm_forward_backward (same dispatch, no outputs) on the
//     windows of the centres still growing + k_grow_probe; only the n "grows again" flags come back per candidate.
static int grow_literal(svihmm_ctx* h, const int64_t* centers, int n, int half0, int m, int inc, int cutoff, double eps,
                        int rule, uint32_t flags, int trace_cap, int32_t* out_half, int32_t* out_steps, double* out_trace) {
  std::vector<double> init((size_t)n * 6, 0.0);
  for (int i = 0; i < n; ++i) init[(size_t)i * 6] = init[(size_t)i * 6 + 1] = 1.7976931348623157e308;
  CK(launch_grow_state(h, n, trace_cap, centers, init.data()));
  std::vector<int32_t> act(n), flag(n);
  std::vector<int64_t> starts(n);
  for (int i = 0; i < n; ++i) act[i] = i;
  int b = half0;
  bool first = true;
  while (!act.empty()) {
    const int nact = (int)act.size(), Lm = 2 * b + 1;
    for (int j = 0; j < nact; ++j) starts[j] = centers[act[j]] - b;
    const int var = pick_fb(h, nact, Lm, false);
    CK(prepare_ll(h, starts.data(), nact, Lm, flags, false, var == SVIHMM_FB_SCALED));
    CK(run_fb(h, nact, Lm, var, false, false));
    h->lastB = nact; h->lastLm = Lm;
    if (var == SVIHMM_FB_SCALED) CK(ensure_q(h, nact, Lm, h->stream));
    CK(launch_grow_probe(h, n, nact, act.data(), b, m, first, inc, cutoff, eps, rule, trace_cap, flag.data()));
    size_t keep = 0;
    for (int j = 0; j < nact; ++j)
      if (flag[act[j]]) act[keep++] = act[j];
    act.resize(keep);
    first = false;
    if (keep && b > INT32_MAX / 2 - inc) return fail("svihmm_grow_windows: half-width overflow");
    b += inc;
  }
  const int32_t* dist = nullptr;
  const double* dtrace = nullptr;
  CK(grow_state_results(h, n, trace_cap, &dist, &dtrace));
  std::vector<int32_t> ist((size_t)n * 3);
  CK(d2h(h, ist.data(), dist, ist.size() * sizeof(int32_t)));
  if (out_trace && trace_cap > 0) CK(d2h(h, out_trace, dtrace, (size_t)n * trace_cap * 2 * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  for (int i = 0; i < n; ++i) {
    out_half[i] = ist[(size_t)i * 3];
    if (out_steps) out_steps[i] = ist[(size_t)i * 3 + 1];
  }
  return 0;
}

static int grow_products(svihmm_ctx* h, const int64_t* centers, int n, int half0, int m, int inc, int cutoff, double eps,
                         int rule, uint32_t flags, int trace_cap, int32_t* out_half, int32_t* out_steps, double* out_trace) {
  const int64_t T = h->T;
  // steps the rule's first condition allows: it goes on from b while b <= min(c - 1 - inc, T - c - inc - 1, cutoff)
  std::vector<int32_t> smax(n), off(n);
  std::vector<int64_t> starts(n);
  int64_t reach = half0;
  for (int i = 0; i < n; ++i) {
    const int64_t c = centers[i];
    int64_t lim = c - 1 - inc;
    if (T - c - inc - 1 < lim) lim = T - c - inc - 1;
    if (cutoff < lim) lim = cutoff;
    const int64_t s = lim >= half0 ? (lim - half0) / inc + 1 : 0;
    smax[i] = (int32_t)s;
    if (half0 + s * inc > reach) reach = half0 + s * inc;
  }
  const int64_t W64 = 2 * reach + 1 < T ? 2 * reach + 1 : T;
  if (W64 * h->K >= ((int64_t)1 << 31)) return fail("svihmm_grow_windows: reach window too long for the product kernel");
  const int W = (int)W64;
  for (int i = 0; i < n; ++i) {
    int64_t s0 = centers[i] - reach;
    if (s0 > T - W) s0 = T - W;
    if (s0 < 0) s0 = 0;
    starts[i] = s0;
    off[i] = (int32_t)(centers[i] - s0);
  }
  CK(prepare_ll(h, starts.data(), n, W, flags, false));
  h->lastB = n; h->lastLm = W;
  int32_t *dhalf = nullptr, *dsteps = nullptr;
  double* dtrace = nullptr;
  CK(launch_grow_products(h, n, W, (const double*)h->ll.p, off.data(), smax.data(), half0, m, inc, eps, rule,
                          out_trace ? trace_cap : 0, &dhalf, &dsteps, &dtrace));
  CK(d2h(h, out_half, dhalf, (size_t)n * sizeof(int32_t)));
  if (out_steps) CK(d2h(h, out_steps, dsteps, (size_t)n * sizeof(int32_t)));
  if (out_trace && trace_cap > 0) CK(d2h(h, out_trace, dtrace, (size_t)n * trace_cap * 2 * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

int svihmm_grow_windows(svihmm_ctx* h, const int64_t* centers, int32_t n, int32_t half0, int32_t probe_off,
                        int32_t increment, int32_t cutoff, double epsilon, int32_t rule, uint32_t flags, int32_t method,
                        int32_t* out_half, int32_t* out_steps, double* out_trace, int32_t trace_cap) {
  const char* fn = "svihmm_grow_windows";
  const auto bad = [fn](const std::string& what) { return fail(std::string(fn) + ": " + what); };
  if (!h) return bad("NULL handle");
  if (h->have_labels)
    return bad("labels are in force (svihmm_set_labels) and the growth rules do not take them; remove them with "
               "svihmm_set_labels(h, NULL)");
  if (h->have_sets)
    return bad("allowed-state sets are in force (svihmm_set_state_sets) and the growth rules do not take them; remove "
               "them with svihmm_set_state_sets(h, NULL, 0)");
  if (!centers || !out_half) return bad("centers and out_half must be given");
  if (n < 1) return bad("n must be positive");
  if (increment < 1) return bad("increment must be positive");
  if (half0 < 0 || probe_off < 0 || probe_off > half0) return bad("need 0 <= probe_off <= half0");
  if (rule != 0 && rule != 1) return bad("rule must be 0 (last residual) or 1 (running average)");
  if (!(epsilon > -1.7976931348623157e308 && epsilon < 1.7976931348623157e308)) return bad("epsilon must be finite");
  if (trace_cap < 0) return bad("trace_cap must not be negative");
  if (method != SVIHMM_GROW_AUTO && method != SVIHMM_GROW_LITERAL && method != SVIHMM_GROW_PRODUCTS)
    return bad("unknown method");
  if (flags & SVIHMM_USE_HOST_LLIKS) return bad("SVIHMM_USE_HOST_LLIKS is not supported (host lliks have no row axis to grow along)");
  if (!h->have_globals) return bad("no globals: call svihmm_set_globals first");
  CK(check_window_model(h, fn));
  for (int i = 0; i < n; ++i)
    if (centers[i] - half0 < 0 || centers[i] + half0 >= h->T)
      return bad("start window of centre " + std::to_string(i) + " reaches outside [0, T)");
  for (int i = 0; i < n; ++i) {
    const int64_t st = centers[i] - half0;
    CK(check_window_sequences(h, std::string(fn) + ": start ", &st, 1, 2 * half0 + 1));
  }
  const bool products_ok = h->K <= 64 && !h->exact_log;
  if (method == SVIHMM_GROW_PRODUCTS && !products_ok)
    return bad("method PRODUCTS needs K <= 64 and every ltran entry >= SVIHMM_LTRAN_LINEAR_MIN (K = " +
               std::to_string(h->K) + (h->exact_log ? ", ltran below the linear range)" : ")"));
  const bool products = method == SVIHMM_GROW_PRODUCTS || (method == SVIHMM_GROW_AUTO && products_ok);
  CK(set_device(h));
  CK(wait_side_streams(h));
  const uint32_t fl = flags & SVIHMM_MASK_AS_NAN;
  const int cap = out_trace ? trace_cap : 0;
  {
    ReportHold hold(h, false, true);   // always fp64
    CK(products ? grow_products(h, centers, n, half0, probe_off, increment, cutoff, epsilon, rule, fl, cap, out_half,
                                out_steps, out_trace)
                : grow_literal(h, centers, n, half0, probe_off, increment, cutoff, epsilon, rule, fl, cap, out_half,
                               out_steps, out_trace));
  }
  CK(check_emission_status(h));
  return 0;
}

// ---- synthetic sequences generated in HBM (gen_synthetic.py:27-44) --------------------------
int svihmm_generate(svihmm_ctx* h, int64_t T, int32_t K, int32_t D, const double* cdf,
                    const double* means, const double* chols, uint64_t seed) {
  if (!h || T <= 0 || K <= 0 || D <= 0 || !cdf || !means || !chols) return fail("svihmm_generate: bad arguments");
  if (K > 64) return fail("svihmm_generate: K > 64 not supported");
  if (D > 4095) return fail("svihmm_generate: D too large");
  CK(set_device(h));
  h->lin_stale = true;
  CK(ensure(h->obs, (size_t)T * D * sizeof(double)));
  CK(ensure(h->gen_z, (size_t)T * sizeof(int32_t)));
  h->have_mask = false;
  const int KS = K <= 16 ? 16 : K <= 32 ? 32 : 64;
  const int Ls = T >= 65536 ? 512 : 256;
  const int Cs = (int)((T + Ls - 1) / Ls);
  const size_t npar = (size_t)K * K + (size_t)K * D + (size_t)K * D * D;
  const size_t bytes = npar * sizeof(double) + (size_t)T * KS + 2 * (size_t)Cs * KS + (size_t)Cs + 64;
  CK(ensure(h->scratch, bytes));
  double* dcdf = (double*)h->scratch.p;
  double* dmean = dcdf + (size_t)K * K;
  double* dchol = dmean + (size_t)K * D;
  unsigned char* path = (unsigned char*)(dchol + (size_t)K * D * D);
  unsigned char* mA = path + (size_t)T * KS;
  unsigned char* mB = mA + (size_t)Cs * KS;
  unsigned char* entry = mB + (size_t)Cs * KS;
  HIPCK(hipMemcpyAsync(dcdf, cdf, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(dmean, means, (size_t)K * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(dchol, chols, (size_t)K * D * D * sizeof(double), hipMemcpyHostToDevice, h->stream));
  {
    ProfScope ps(h, KS_MISC);
#define GPATH(KM)                                                                                        \
  hipLaunchKernelGGL(k_gen_paths<KM>, dim3(Cs), dim3(64), (size_t)K * (KM + 1) * sizeof(double), h->stream, \
                     (const double*)dcdf, (unsigned long long)seed, T, K, Ls, path)
    if (KS == 16) GPATH(16); else if (KS == 32) GPATH(32); else GPATH(64);
#undef GPATH
    hipLaunchKernelGGL(k_gen_compose, dim3(1), dim3(1024), 0, h->stream, (const unsigned char*)path, T, KS, Ls,
                       Cs, mA, mB, entry);
    hipLaunchKernelGGL(k_gen_gather, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, h->stream,
                       (const unsigned char*)path, (const unsigned char*)entry, T, KS, Ls, (int32_t*)h->gen_z.p);
    hipLaunchKernelGGL(k_gen_obs, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, h->stream,
                       (const int32_t*)h->gen_z.p, (const double*)dmean, (const double*)dchol,
                       (unsigned long long)seed, T, D, (double*)h->obs.p);
    HIPCK(hipGetLastError());
  }
  h->T = T; h->D = D; h->gen_T = T;
  drop_clamp(h);
  h->seq_off.clear();
  h->svi_active = false;
  h->center_pending = false;
  {   // centre: the plain average of the state means (a point inside the data)
    std::vector<double> c((size_t)D, 0.0);
    h->center_deferred = h->have_emission && fam_table(h->fam);
    if (h->variant[SVIHMM_VAR_CENTRING] != SVIHMM_CENTRING_OFF && !(h->have_emission && fam_table(h->fam))) {
      for (int k = 0; k < K; ++k)
        for (int d = 0; d < D; ++d) c[d] += means[(size_t)k * D + d] / K;
      for (int d = 0; d < D; ++d) if (!finite_val(c[d])) c[d] = 0.0;
    }
    CK(reset_shift(h, c, 0, T));
  }
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}
int svihmm_read_generated(svihmm_ctx* h, int32_t* sts_out, double* obs_out) {
  if (!h || (!sts_out && !obs_out)) return fail("svihmm_read_generated: bad arguments");
  if (h->gen_T <= 0 || h->gen_T != h->T) return fail("svihmm_read_generated: no generated sequence is resident");
  CK(set_device(h));
  if (sts_out) CK(d2h(h, sts_out, h->gen_z.p, (size_t)h->T * sizeof(int32_t)));
  if (obs_out) CK(d2h(h, obs_out, h->obs.p, (size_t)h->T * h->D * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  if (obs_out && h->shifted) {          // the resident copy is centred: hand out caller coordinates
    const size_t D = (size_t)h->D;
    for (int64_t t = 0; t < h->T; ++t)
      for (size_t d = 0; d < D; ++d) obs_out[(size_t)t * D + d] += h->shift[d];
  }
  return 0;
}

// ---- multi-GPU -------------------------------------------------------------------------
int svihmm_comm_unique_id(char uid_out[128]) {
  static_assert(sizeof(ncclUniqueId) == 128, "ncclUniqueId size");
  ncclUniqueId id;
  NCCLCK(ncclGetUniqueId(&id));
  std::memcpy(uid_out, &id, 128);
  return 0;
}

int svihmm_comm_init(svihmm_ctx* h, const char uid[128], int32_t rank, int32_t nranks) {
  if (!h || !uid || nranks <= 0 || rank < 0 || rank >= nranks)
    return fail("svihmm_comm_init: bad arguments");
  CK(set_device(h));
  if (h->comm) { ncclCommDestroy(h->comm); h->comm = nullptr; }
  ncclUniqueId id;
  std::memcpy(&id, uid, 128);
  NCCLCK(ncclCommInitRank(&h->comm, nranks, id, rank));
  h->rank = rank; h->nranks = nranks;
  return 0;
}

int svihmm_comm_count(svihmm_ctx* h, int32_t* nranks_out) {
  if (!h || !nranks_out) return fail("svihmm_comm_count: bad arguments");
  if (!h->comm) { *nranks_out = 0; return 0; }
  int n = 0;
  NCCLCK(ncclCommCount(h->comm, &n));
  *nranks_out = n;
  return 0;
}

int svihmm_comm_destroy(svihmm_ctx* h) {
  if (!h) return 0;
  if (h->comm) { ncclCommDestroy(h->comm); h->comm = nullptr; }
  h->nranks = 1; h->rank = 0;
  return 0;
}

int svihmm_allreduce_packed(svihmm_ctx* h) {
  if (!h) return fail("svihmm_allreduce_packed: NULL handle");
  if (!h->have_packed) return fail("svihmm_allreduce_packed: no statistics computed yet");
  if (!h->comm) return fail("svihmm_allreduce_packed: communicator not initialised");
  CK(set_device(h));
  ProfScope ps(h, KS_ALLREDUCE);
  CK(allreduce_packed_dev(h));
  h->mirror_valid = false;
  return launch_mirror(h);   // the host-visible copy follows the reduced statistics
}

// Host-mediated exchange of the same statistics (a communicator other than RCCL -- MPI, gloo -- or
// two handles on one device): export hands out what the all-reduce would put on the wire (caller
// coordinates), import takes the reduced vector back into the handle's centred `packed`, from where
// svihmm_read_packed / the device-side global step continue as after svihmm_allreduce_packed.
int svihmm_export_packed(svihmm_ctx* h, double* out_packed) {
  if (!h || !out_packed) return fail("svihmm_export_packed: bad arguments");
  if (!h->have_packed) return fail("svihmm_export_packed: no statistics computed yet");
  CK(set_device(h));
  double* buf = nullptr;
  CK(packed_to_common(h, true, &buf));
  return d2h_sync_small(h, out_packed, buf, (size_t)packed_len(h) * sizeof(double));
}
int svihmm_import_packed(svihmm_ctx* h, const double* packed_in) {
  if (!h || !packed_in) return fail("svihmm_import_packed: bad arguments");
  if (!h->have_globals || h->D <= 0) return fail("svihmm_import_packed: set obs / globals / emission first");
  CK(set_device(h));
  const size_t nb = (size_t)packed_len(h) * sizeof(double);
  CK(ensure(h->packed, nb));
  const bool sh = common_needs_shift(h, true);
  if (sh) CK(ensure(h->commtmp, nb));
  double* dst = sh ? (double*)h->commtmp.p : (double*)h->packed.p;
  CK(upload_blocks(h, dst, {{packed_in, packed_len(h)}}));
  CK(packed_from_common(h, dst));
  h->have_packed = true;
  h->mirror_valid = false;
  return 0;
}

int svihmm_allreduce_host(svihmm_ctx* h, double* buf, int64_t n, int32_t op) {
  if (!h || !buf || n <= 0) return fail("svihmm_allreduce_host: bad arguments");
  if (!h->comm) return fail("svihmm_allreduce_host: communicator not initialised");
  CK(set_device(h));
  // a persistent staging buffer: the barriers of a timed region must not pay hipMalloc / hipFree
  CK(ensure(h->commtmp, (size_t)n * sizeof(double)));
  void* tp = h->commtmp.p;
  HIPCK(hipMemcpyAsync(tp, buf, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  NCCLCK(ncclAllReduce(tp, tp, (size_t)n, ncclDouble, op == 1 ? ncclMax : ncclSum, h->comm, h->stream));
  HIPCK(hipMemcpyAsync(buf, tp, n * sizeof(double), hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

// ---- measurement --------------------------------------------------------------------------
static void drain(svihmm_ctx* h) {
  for (auto& p : h->pending) {
    hipEventSynchronize(p.e1);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, p.e0, p.e1) == hipSuccess) {
      h->ms[p.slot] += ms;
      h->cnt[p.slot] += 1;
    }
    h->pool.push_back(p.e0);
    h->pool.push_back(p.e1);
  }
  h->pending.clear();
}

int svihmm_profile_enable(svihmm_ctx* h, int32_t on) {
  if (!h) return fail("NULL handle");
  CK(set_device(h));
  if (!on) drain(h);
  h->prof = on != 0;
  // on = 1: every slot; on = SVIHMM_PROF_SLOTS | (1 << slot) | ...: only those slots (an event pair
  // between two dependent kernels costs a few microseconds of dispatch: a timed region that wants
  // one kernel's duration should not pay for eleven)
  h->prof_mask = (on & SVIHMM_PROF_SLOTS) ? ((uint32_t)on & 0xfffu) : 0xffffffffu;
  return 0;
}
int svihmm_profile_reset(svihmm_ctx* h) {
  if (!h) return fail("NULL handle");
  CK(set_device(h));
  drain(h);
  for (int i = 0; i < SVIHMM_NKERN; ++i) { h->ms[i] = 0; h->cnt[i] = 0; }
  return 0;
}
int svihmm_profile_read(svihmm_ctx* h, double ms_out[SVIHMM_NKERN], int64_t count_out[SVIHMM_NKERN]) {
  if (!h) return fail("NULL handle");
  CK(set_device(h));
  HIPCK(hipStreamSynchronize(h->stream));
  drain(h);
  for (int i = 0; i < SVIHMM_NKERN; ++i) { ms_out[i] = h->ms[i]; count_out[i] = h->cnt[i]; }
  return 0;
}
const char* svihmm_last_kernel_name(svihmm_ctx* h, int32_t slot) {
  if (!h || slot < 0 || slot >= SVIHMM_NKERN || !h->last_kernel[slot]) return "";
  return h->last_kernel[slot];
}
int svihmm_set_variant(svihmm_ctx* h, int32_t which, int32_t value) {
  if (!h || which < 0 || which >= SVIHMM_NVARIANT) return fail("svihmm_set_variant: bad arguments");
#ifndef SVIHMM_MEASURE
  // codes under which a call's results are invalid exist in the measurement build only
  if (which == SVIHMM_VAR_SWEEP_FAMILY && value == SVIHMM_SWEEP_FAMILY_SKIP)
    return fail("svihmm_set_variant: measurement-only code (build with -DSVIHMM_MEASURE: make measure)");
#endif
  h->variant[which] = value;
  return 0;
}

// ---- diagnostics ---------------------------------------------------------------------------
int svihmm_selftest_mfma(svihmm_ctx* h, const double* A16x4, const double* B4x16, double* C16x16) {
  if (!h) return fail("NULL handle");
  CK(set_device(h));
  CK(ensure(h->scratch, (64 + 64 + 256) * sizeof(double)));
  double* dA = (double*)h->scratch.p; double* dB = dA + 64; double* dC = dB + 64;
  HIPCK(hipMemcpyAsync(dA, A16x4, 64 * 8, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(dB, B4x16, 64 * 8, hipMemcpyHostToDevice, h->stream));
  hipLaunchKernelGGL(k_selftest_mfma, dim3(1), dim3(64), 0, h->stream, dA, dB, dC);
  HIPCK(hipGetLastError());
  HIPCK(hipMemcpyAsync(C16x16, dC, 256 * 8, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

}  // extern "C"

