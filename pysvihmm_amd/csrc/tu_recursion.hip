// tu_recursion.hip -- forward / backward recursions, blocked scan, FFBS: kernels and launchers
// One of the translation units of libsvihmm_hip.so (see host.h).
#include <algorithm>
#include "host.h"
#include "device_helpers.h"
#include "kernels_ffbs_draw.h"
#include "kernels_recursion.h"
#include "kernels_viterbi.h"
#include "kernels_ffbs_windows.h"
#include "kernels_grow.h"
#include "kernels_sequences.h"
#include "kernels_decode_sequences.h"
#define SVIHMM_LABELS_GATHER
#include "kernels_labels.h"

// The Viterbi forward sweep of n units addressed by `units` (kernels_viterbi.h: VitWindows / VitSequences): the one
// dispatch on the model's width.  LDSBT: psi in LDS, the launch writes z itself (z null: score only); otherwise psi
// goes to HBM and unit u's final argmax to zlast[u].  lds: the launch's dynamic LDS, sized by its longest unit.
template <bool LDSBT, class Units>
static void vit_sweep(svihmm_ctx* h, unsigned n, size_t lds, const double* ll, const Units& units, unsigned char* psi,
                      int32_t* z, int32_t* zlast, double* score) {
  const int K = h->K;
  const double* lt = (const double*)h->ltran.p;
  const double* mi = (const double*)h->mod_init.p;
#define VITW(KM)                                                                                                   \
  hipLaunchKernelGGL((k_vit_wave<KM, LDSBT, Units>), dim3(n), dim3(64), lds, h->stream, ll, lt, mi, units, K, psi, \
                     z, zlast, score)
  if (K <= 16) VITW(16); else if (K <= 32) VITW(32); else if (K <= 64) VITW(64);
  else
    hipLaunchKernelGGL((k_vit_wide<LDSBT, Units>), dim3(n), dim3(256), lds, h->stream, ll, lt, mi, units, K, psi, z,
                       zlast, score);
#undef VITW
}

extern "C" {

int launch_fb(svihmm_ctx* h, int B, int Lm, int dir0, int ndir,
                     const double* ll, double* la, double* lb) {
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  const int K = h->K;
  const size_t n = (size_t)B * Lm * K * sizeof(double);
  if (!ll) {
    if (dir0 == 0) CK(ensure(h->la, n));
    if (dir0 + ndir > 1) CK(ensure(h->lb, n));
    ll = (const double*)h->ll.p;
    la = (double*)h->la.p;
    lb = (double*)h->lb.p;
  }
  ProfScope ps(h, KS_FB);
  dim3 grid(B, ndir);
  const double* A = (const double*)h->Aexp.p;
  const double* mi = (const double*)h->mod_init.p;
  if (h->exact_log) {   // transition expectations outside exp()'s range: the literal recursion
    const int threads = (K + 63) / 64 * 64;
    const int in_lds = ((size_t)K * (K + 1) + 2 * K) * 8 <= 150 * 1024;
    const size_t lds = (2 * (size_t)K + (in_lds ? (size_t)K * (K + 1) : 0)) * 8;
    if (lds > 64 * 1024)
      hipFuncSetAttribute((const void*)k_fb_exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_fb_exact, grid, dim3(threads), lds, h->stream, ll, (const double*)h->ltran.p, mi,
                       Lm, K, dir0, in_lds, la, lb);
    HIPCK(hipGetLastError());
    return 0;
  }
  if (K <= 16)
    hipLaunchKernelGGL(k_fb_wave<16>, grid, dim3(64), 0, h->stream, ll, A, mi, Lm, K, dir0, la, lb);
  else if (K <= 32)
    hipLaunchKernelGGL(k_fb_wave<32>, grid, dim3(64), 0, h->stream, ll, A, mi, Lm, K, dir0, la, lb);
  else if (K <= 64)
    hipLaunchKernelGGL(k_fb_wave<64>, grid, dim3(64), 0, h->stream, ll, A, mi, Lm, K, dir0, la, lb);
  else {
    const int threads = (K + 63) / 64 * 64;
    const int in_lds = ((size_t)K * K * 8 + 2 * K * 8 + 128) <= 150 * 1024;
    const size_t lds = (2 * (size_t)K + 16) * 8 + (in_lds ? (size_t)K * K * 8 : 0);
    if (lds > 64 * 1024)
      hipFuncSetAttribute((const void*)k_fb_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_fb_generic, grid, dim3(threads), lds, h->stream, ll, A,
                       (const double*)h->AexpT.p, mi, Lm, K, dir0, in_lds, la, lb);
  }
  HIPCK(hipGetLastError());
  return 0;
}

int launch_posterior(svihmm_ctx* h, int B, int Lm, bool total) {
  const int K = h->K;
  // rows per workgroup: 256 for big batches, down to 16 so that small ones give >= ~2048 workgroups
  int rps = 256;
  while (rps > 16 && (int64_t)B * ((Lm + rps - 1) / rps) < 2048) rps >>= 1;
  const int nseg = (Lm + rps - 1) / rps;
  CK(ensure(h->q, (size_t)B * Lm * K * sizeof(double)));
  CK(ensure(h->lse_part, (size_t)B * nseg * sizeof(double)));
  CK(ensure(h->local_lb, (size_t)B * sizeof(double)));
  CK(ensure(h->packed, (size_t)packed_len(h) * sizeof(double)));
  ProfScope ps(h, KS_POSTERIOR);
  dim3 grid((unsigned)((size_t)B * nseg));
#define POST_LAUNCH(KPL)                                                                  \
  hipLaunchKernelGGL(k_posterior<KPL>, grid, dim3(256), 0, h->stream, (const double*)h->la.p, \
                     (const double*)h->lb.p, Lm, K, nseg, rps, (double*)h->q.p, (double*)h->lse_part.p)
  if (K <= 64) POST_LAUNCH(1);
  else if (K <= 256) POST_LAUNCH(4);
  else POST_LAUNCH(16);
#undef POST_LAUNCH
  double* lbtot = nullptr;
  if (total) lbtot = (double*)h->packed.p + (packed_len(h) - 1);
  hipLaunchKernelGGL(k_reduce_lb, dim3(1), dim3(256), 0, h->stream, (const double*)h->lse_part.p,
                     B, nseg, (double*)h->local_lb.p, lbtot);
  HIPCK(hipGetLastError());
  return 0;
}

// forward sweep, then backward sweep with the posterior fused (K <= 64).  want_lb: also
// materialise lbeta (API readback); total: write sum_b local_lb into packed[last].
int launch_fb_fused(svihmm_ctx* h, int B, int Lm, bool want_lb, bool total) {
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  const int K = h->K;
  const size_t n = (size_t)B * Lm * K * sizeof(double);
  CK(ensure(h->la, n));
  CK(ensure(h->q, n));
  if (want_lb) CK(ensure(h->lb, n));
  CK(ensure(h->local_lb, (size_t)B * sizeof(double)));
  CK(ensure(h->logz, (size_t)B * sizeof(double)));
  CK(ensure(h->packed, (size_t)packed_len(h) * sizeof(double)));
  const int NW = (K + 15) / 16;
  dim3 grid((B + 15) / 16);
  const double* ll = (const double*)h->ll.p;
  double* la = (double*)h->la.p;
  double* lb = want_lb ? (double*)h->lb.p : nullptr;
  double* q = (double*)h->q.p;
  double* llb = (double*)h->local_lb.p;
  double* lz = (double*)h->logz.p;
  {
    ProfScope ps(h, KS_FB);
#define FWD(NWV, F) hipLaunchKernelGGL((k_fwd_mfma<NWV, F>), grid, dim3(64 * NWV), 0, h->stream, ll, \
                                       (const double*)h->Aexp.p, (const double*)h->mod_init.p, B, Lm, K, la, llb, lz)
    const bool full = (K == 16 * NW);
    if (NW == 1) { if (full) FWD(1, true); else FWD(1, false); }
    else if (NW == 2) { if (full) FWD(2, true); else FWD(2, false); }
    else if (NW == 3) { if (full) FWD(3, true); else FWD(3, false); }
    else { if (full) FWD(4, true); else FWD(4, false); }
#undef FWD
    HIPCK(hipGetLastError());
  }
  {
    ProfScope ps(h, KS_POSTERIOR);
    const bool full = (K == 16 * NW);
#define BWD(NWV, F, W) hipLaunchKernelGGL((k_bwd_mfma<NWV, F, W>), grid, dim3(64 * NWV), 0, h->stream, ll, \
                                          (const double*)h->AexpT.p, (const double*)la, (const double*)lz, B, Lm, K, lb, q)
#define BWD2(NWV) do { if (full) { if (want_lb) BWD(NWV, true, true); else BWD(NWV, true, false); } \
                       else { if (want_lb) BWD(NWV, false, true); else BWD(NWV, false, false); } } while (0)
    if (NW == 1) BWD2(1); else if (NW == 2) BWD2(2); else if (NW == 3) BWD2(3); else BWD2(4);
#undef BWD2
#undef BWD
    if (total) {
      double* lbtot = (double*)h->packed.p + (packed_len(h) - 1);
      hipLaunchKernelGGL(k_sum_lb, dim3(1), dim3(256), 0, h->stream, (const double*)llb, B, lbtot);
    }
    HIPCK(hipGetLastError());
  }
  return 0;
}

// scaled linear-domain sweeps (K <= 64): Eh / kexp -> ah, (na, k), Z -> var_x
int ensure_fb_lin(svihmm_ctx* h, int B, int Lm) {
  const int K = h->K;
  const size_t n = (size_t)B * Lm * K * sizeof(double);
  CK(ensure(h->la, n));
  CK(ensure(h->lb, n));
  CK(ensure(h->hx, (size_t)B * Lm * sizeof(double)));
  CK(ensure(h->gx, (size_t)B * Lm * sizeof(double)));
  CK(ensure(h->zfac, (size_t)B * sizeof(double2)));
  CK(ensure(h->local_lb, (size_t)B * sizeof(double)));
  CK(ensure(h->logz, (size_t)B * sizeof(double)));
  CK(ensure(h->packed, (size_t)packed_len(h) * sizeof(double)));
  CK(ensure(h->a0v, (size_t)B * K * sizeof(double)));
  CK(ensure(h->a0e, (size_t)B * sizeof(double)));
  return 0;
}
// initial messages of windows [b0, b0+nb): mod_init + ll_0 in the log domain (k_lin_init); the
// first rows' log-likelihoods come from the scaled emission's side output (ll0) or, where the
// plain lliks are kept (host lliks, wide models, Categorical), straight from those
static int launch_lin_init(svihmm_ctx* h, int b0, int nb, int Lm, hipStream_t stream) {
  const int K = h->K;
  const double* src = h->eh_in_llE ? (const double*)h->ll.p + (size_t)b0 * Lm * K
                                   : (const double*)h->ll0.p + (size_t)b0 * K;
  const size_t stride = h->eh_in_llE ? (size_t)Lm * K : (size_t)K;
  hipLaunchKernelGGL(k_lin_init, dim3((unsigned)((nb + 3) / 4)), dim3(256), 0, stream,
                     (const double*)h->mod_init.p, src, stride, (const double*)h->kexp.p + (size_t)b0 * Lm,
                     nb, Lm, K, (double*)h->a0v.p + (size_t)b0 * K, (double*)h->a0e.p + b0);
  HIPCK(hipGetLastError());
  return 0;
}
// minibatch-sized batches, 16 < K <= 64: the kernels that split one window over one wave's registers (fp64,
// k_wave_linr) or four waves (fp32 storage, k_wave_lin4)
static bool minibatch_wave_kernel(const svihmm_ctx* h, int K, int nb, int Lm) {
  if (K <= 16 || K > 64 || nb >= lin_wave_max(h) || h->variant[SVIHMM_VAR_SWEEP_FAMILY] == SVIHMM_SWEEP_FAMILY_TILES ||
      h->variant[SVIHMM_VAR_SWEEP_FAMILY] == SVIHMM_SWEEP_FAMILY_WAVE_LIN)
    return false;
  return h->cur_f32 ? nb <= lin_wave4_max(h) : (nb <= lin_waver_max(h) && Lm <= (1 << 20));
}
// SVI loop on counters (svihmm_hip.hip, svi_globals): those two kernels wait for the side stream's globals
// kernel themselves -- no stream-order event in front of them
SviSync sweep_gate(svihmm_ctx* h, hipStream_t stream) {
  SviSync sy = {};
  if (h->svi_flags && h->in_svi_estep && h->globals_ev && stream == h->stream && h->svi_sync.p) {
    sy.gate = (const unsigned*)h->svi_sync.p + 16;
    sy.gate_tgt = (unsigned)h->tgt_glob;
    sy.status = h->svi_status_dev;
    // (sweeps that cannot get their globals poison their iteration: the global step behind them does not run)
    sy.dead = (unsigned*)h->svi_sync.p + 16 * 7;
    sy.ticks = h->svi_ticks;
    sy.poison = (unsigned*)h->svi_sync.p + 16 * 5;
    sy.poison_val = SVI_POISON_BASE - (unsigned)(h->svi_cur_it < 0 ? 0 : h->svi_cur_it);
    // (debug: a count that never comes, 2 ms bound -- svi_recover's test)
    if (h->variant[SVIHMM_VAR_SVI_LOOP] == SVIHMM_SVI_LOOP_STUCK_GATE && h->svi_cur_it == 3) {
      sy.gate_tgt += 1000u;
      sy.ticks = (unsigned long long)(2.0 * (h->wall_clock_khz > 0.0 ? h->wall_clock_khz : 100000.0));
    }
    h->globals_ev = nullptr;
  }
  if (h->svi_flags && h->in_svi_estep && stream == h->stream && h->svi_sync.p && h->elbo_pending) {
    // the deferred ELBO kernels of the previous iteration start with these sweeps (svihmm_svi_iteration)
    sy.early = (unsigned*)h->svi_sync.p + 16 * 4;
    ++h->tgt_early;
    h->sweep_signalled = true;
  }
  return sy;
}
// both sweeps over windows [b0, b0+nb) of the current batch on `stream` (buffers ensured):
// one launch, blockIdx.y = direction
int launch_fb_lin_range(svihmm_ctx* h, int b0, int nb, int Lm, hipStream_t stream) {
  const int K = h->K;
  const bool wave_kernel = minibatch_wave_kernel(h, K, nb, Lm);
  if (h->svi_flags && h->in_svi_estep && stream == h->stream && !wave_kernel) CK(wait_globals(h));
  // measurement only (tools/r4_overlap_probe.py): SVIHMM_SWEEP_FAMILY_SKIP skips the sweep launch -- the
  // statistics then read the previous step's messages; bounds what hiding the sweeps could give
#ifdef SVIHMM_MEASURE
  if (h->variant[SVIHMM_VAR_SWEEP_FAMILY] == SVIHMM_SWEEP_FAMILY_SKIP) return 0;
#endif
  const int NW = (K + 15) / 16;
  const bool full = (K == 16 * NW);
  dim3 grid((nb + 15) / 16, 2);
  const size_t ro = (size_t)b0 * Lm;
  const double* Eh = (const double*)(h->eh_in_llE ? h->llE.p : h->ll.p) + ro * K;
  const double* kx = (const double*)h->kexp.p + ro;
  double* ah = (double*)h->la.p + ro * K;
  double* bh = (double*)h->lb.p + ro * K;
  double* hx = (double*)h->hx.p + ro;
  double* gx = (double*)h->gx.p + ro;
  double2* zf = (double2*)h->zfac.p + b0;
  double* llb = (double*)h->local_lb.p + b0;
  double* lz = (double*)h->logz.p + b0;
  const double* a0v = (const double*)h->a0v.p + (size_t)b0 * K;
  const double* a0e = (const double*)h->a0e.p + b0;
  // first-row log-likelihoods of the windows (see launch_lin_init): the wave-per-window kernels
  // form the initial message themselves, the tile kernels take it from k_lin_init
  const double* mi = (const double*)h->mod_init.p;
  const double* l0 = h->eh_in_llE ? (const double*)h->ll.p + ro * K : (const double*)h->ll0.p + (size_t)b0 * K;
  const size_t l0s = h->eh_in_llE ? (size_t)Lm * K : (size_t)K;
  ProfScope ps(h, KS_FB, stream);
  if (h->cur_f32) {
    // fp32 mode (K <= 64, b0 == 0): the same kernels instantiated for float storage
    const float* Ef = (const float*)h->ll.p;
    float* af = (float*)h->la.p;
    float* bf = (float*)h->lb.p;
    if (K > 64) {
      // wide models (round 5): k_sweeps_lin2 on v_mfma_f32_16x16x4_f32, the transition matrix streamed from
      // its float copy (rows up to 256 + slack zeroed once per buffer, K rows converted per launch)
      CK(launch_lin_init(h, b0, nb, Lm, stream));
      const size_t nrow_t = 256 + 16, kk = (size_t)K * K;
      CK(ensure(h->AexpF, nrow_t * K * sizeof(float)));
      CK(ensure(h->AexpTF, nrow_t * K * sizeof(float)));
      HIPCK(hipMemsetAsync((char*)h->AexpF.p + kk * 4, 0, (nrow_t * K - kk) * 4, stream));
      HIPCK(hipMemsetAsync((char*)h->AexpTF.p + kk * 4, 0, (nrow_t * K - kk) * 4, stream));
      hipLaunchKernelGGL(k_f64_to_f32, dim3(64), dim3(256), 0, stream, (const double*)h->Aexp.p, (float*)h->AexpF.p, kk);
      hipLaunchKernelGGL(k_f64_to_f32, dim3(64), dim3(256), 0, stream, (const double*)h->AexpT.p, (float*)h->AexpTF.p, kk);
      // 16 windows per workgroup: with two window tiles per wave the 128 resident transition values + the
      // second tile's accumulators spill (4.0 ms on configs[4]; one tile: 3.17; the streamed kernel 3.70)
      const bool w32 = false;
#define SWP2F(F, WT)                                                                                          \
  do {                                                                                                        \
    const size_t lds = (size_t)(WT) * sizeof(LinShared<16>);                                                  \
    dim3 g2((unsigned)((nb + 16 * (WT) - 1) / (16 * (WT))), 2);                                               \
    hipFuncSetAttribute((const void*)k_sweeps_lin2<8, F, WT, float, true>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds); \
    hipLaunchKernelGGL((k_sweeps_lin2<8, F, WT, float, true>), g2, dim3(512), lds, stream, Ef, kx,            \
                       (const float*)h->AexpF.p, (const float*)h->AexpTF.p, a0v, a0e, nb, Lm, K, af, bf, hx, gx, llb, lz, zf); \
  } while (0)
      if (w32) { if (K == 256) SWP2F(true, 2); else SWP2F(false, 2); }
      else if (K == 256) SWP2F(true, 1); else SWP2F(false, 1);
#undef SWP2F
      HIPCK(hipGetLastError());
      return 0;
    }
    if (nb < lin_wave_max(h) && h->variant[SVIHMM_VAR_SWEEP_FAMILY] != SVIHMM_SWEEP_FAMILY_TILES) {
      dim3 gw((unsigned)nb, 2);
#define WLF(KM, FK) hipLaunchKernelGGL((k_wave_lin<KM, FK, float>), gw, dim3(64), 0, stream, Ef, kx, (const double*)h->Aexp.p, \
                                       (const double*)h->AexpT.p, mi, l0, l0s, Lm, K, af, bf, hx,   \
                                       gx, llb, lz, zf)
#define WL4F(KM) hipLaunchKernelGGL((k_wave_lin4<KM, float>), gw, dim3(256), 0, stream, Ef, kx, (const double*)h->Aexp.p, \
                                    (const double*)h->AexpT.p, mi, l0, l0s, Lm, K, af, bf, hx, gx, \
                                    llb, lz, zf, gsy)
      // (round 5: the register-resident one-wave kernel k_wave_linr of the fp64 path was also built with fp32
      //  arithmetic: 278 against 303 ns per step, but over 257 steps the statistics drift to 1.2e-4 of the fp64
      //  oracle -- inside the mode's 1e-3, above this suite's 1e-4 canary; the fp32 mode keeps the four-wave
      //  kernel, which computes in fp64 on float storage)
      if (wave_kernel && nb <= lin_waver_max(h) && Lm <= (1 << 20) &&
          h->variant[SVIHMM_VAR_SWEEP_FAMILY] != SVIHMM_SWEEP_FAMILY_WAVE_LIN4) {
        // (round 5, second half: the one-wave register-resident kernel with fp64 arithmetic on the float storage)
        const SviSync gsy = sweep_gate(h, stream);
        hipLaunchKernelGGL((k_wave_linr<float, double>), gw, dim3(64), 0, stream, Ef, kx, (const double*)h->Aexp.p,
                           (const double*)h->AexpT.p, mi, l0, l0s, Lm, K, af, bf, hx, gx, llb, lz, zf, gsy);
      }
      else if (wave_kernel) { const SviSync gsy = sweep_gate(h, stream); WL4F(64); }
      else if (K <= 16) WLF(16, false); else if (K <= 32) WLF(32, false);
      else if (K == 64) WLF(64, true); else WLF(64, false);
#undef WLF
#undef WL4F
    } else {
      CK(launch_lin_init(h, b0, nb, Lm, stream));
      const LinChain none = {};
#define SWF(NWV, F) hipLaunchKernelGGL((k_sweeps_lin<NWV, F, 0, false, float>), grid, dim3(64 * NWV),              \
                                       sizeof(LinShared<NWV>), stream, Ef, kx, (const double*)h->Aexp.p,         \
                                       (const double*)h->AexpT.p, a0v, a0e, nb, Lm, Lm, K,   \
                                       af, bf, hx, gx, llb, lz, zf, none)
      if (NW == 1) { if (full) SWF(1, true); else SWF(1, false); }
      else if (NW == 2) { if (full) SWF(2, true); else SWF(2, false); }
      else if (NW == 3) { if (full) SWF(3, true); else SWF(3, false); }
      else { if (full) SWF(4, true); else SWF(4, false); }
#undef SWF
    }
    HIPCK(hipGetLastError());
    return 0;
  }
  if (K <= 64 && nb < lin_wave_max(h) && h->variant[SVIHMM_VAR_SWEEP_FAMILY] != SVIHMM_SWEEP_FAMILY_TILES) {
    // small batches: one wavefront per (window, direction)
    dim3 gw((unsigned)nb, 2);
#define WL(KM, FK) hipLaunchKernelGGL((k_wave_lin<KM, FK>), gw, dim3(64), 0, stream, Eh, kx, (const double*)h->Aexp.p, \
                                      (const double*)h->AexpT.p, mi, l0, l0s, Lm, K, ah, bh, hx,  \
                                      gx, llb, lz, zf)
    // up to a few hundred windows the chip is far from full with one wave per (window,
    // direction): split each window's source states over four waves (SVIHMM_SWEEP_FAMILY_WAVE_LIN: off)
    // minibatch-sized batches, K > 16 (round 5): one wave per (window, direction) with the mat-vec in registers
    // (k_wave_linr; it replaces round 3's four-wave k_wave_lin4<64, double>: 316 against 319 ns per step with a
    // quarter of the waves and no LDS exchange; SVIHMM_SWEEP_FAMILY_WAVE_LIN: the LDS-broadcast one-wave kernel below)
    if (wave_kernel) {
      const SviSync gsy = sweep_gate(h, stream);
      // (transition expectations inside a float's range: re-normalised every fourth step -- kernels_wave_linr.h, RN;
      //  SVIHMM_RENORM4_OFF: every step)
      if (h->f32_ok && h->variant[SVIHMM_VAR_RENORM4] != SVIHMM_RENORM4_OFF)
        hipLaunchKernelGGL((k_wave_linr<double, double, 4>), gw, dim3(64), 0, stream, Eh, kx, (const double*)h->Aexp.p,
                           (const double*)h->AexpT.p, mi, l0, l0s, Lm, K, ah, bh, hx, gx, llb, lz, zf, gsy);
      else
        hipLaunchKernelGGL((k_wave_linr<double>), gw, dim3(64), 0, stream, Eh, kx, (const double*)h->Aexp.p,
                           (const double*)h->AexpT.p, mi, l0, l0s, Lm, K, ah, bh, hx, gx, llb, lz, zf, gsy);
    }
    else if (K <= 16) WL(16, false); else if (K <= 32) WL(32, false);
    else if (K == 64) WL(64, true); else WL(64, false);
#undef WL
    HIPCK(hipGetLastError());
    return 0;
  }
  CK(launch_lin_init(h, b0, nb, Lm, stream));
  LinChain none = {};
  if (h->step_major) {      // (prepare_ll chose it for exactly the launch below: step_major_ok)
    if (!(NW == 4 && full && b0 == 0 && nb == h->curB)) return fail("internal: step-major messages without their sweep kernel");
    none.smaj = 1;
  }
#define SWPX(NWV, F, BSV)                                                                                  \
  do {                                                                                                     \
    const size_t lds = sizeof(LinShared<NWV>);                                                             \
    if (lds > 64 * 1024)                                                                                   \
      hipFuncSetAttribute((const void*)k_sweeps_lin<NWV, F, 0, BSV>,                                       \
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);                           \
    hipLaunchKernelGGL((k_sweeps_lin<NWV, F, 0, BSV>), grid, dim3(64 * NWV), lds, stream, Eh, kx,          \
                       (const double*)h->Aexp.p, (const double*)h->AexpT.p,                                \
                       a0v, a0e, nb, Lm, Lm, K, ah, bh, hx, gx, llb, lz, zf, none);    \
  } while (0)
#define SWP(NWV, F) SWPX(NWV, F, false)
  if (NW == 1) { if (full) SWP(1, true); else SWP(1, false); }
  else if (NW == 2) { if (full) SWP(2, true); else SWP(2, false); }
  else if (NW == 3) { if (full) SWP(3, true); else SWP(3, false); }
  else if (NW == 4) { if (full) SWP(4, true); else SWP(4, false); }
  else if (NW <= 8) { if (K == 128) SWPX(8, true, true); else SWPX(8, false, true); }      // K > 64: B streamed
  else {
    // 128 < K <= 256: eight waves of two state tiles (256 VGPRs each) instead of 16 x 1
#define SWP2(F, WT)                                                                                        \
  do {                                                                                                     \
    const size_t lds = (size_t)(WT) * sizeof(LinShared<16>);                                               \
    dim3 g2((unsigned)((nb + 16 * (WT) - 1) / (16 * (WT))), 2);                                            \
    hipFuncSetAttribute((const void*)k_sweeps_lin2<8, F, WT>, hipFuncAttributeMaxDynamicSharedMemorySize,  \
                        (int)lds);                                                                         \
    hipLaunchKernelGGL((k_sweeps_lin2<8, F, WT>), g2, dim3(512), lds, stream, Eh, kx,                      \
                       (const double*)h->Aexp.p, (const double*)h->AexpT.p, a0v, a0e,  \
                       nb, Lm, K, ah, bh, hx, gx, llb, lz, zf);                                            \
  } while (0)
    // more 16-window workgroups than CUs: 32 windows per workgroup share the streamed transition
    // tile (SVIHMM_WIDE_SWEEPS_16: off)
    // (more workgroups than CUs)
    const bool w32 = 2 * ((nb + 15) / 16) > h->ncu && h->variant[SVIHMM_VAR_WIDE_SWEEPS] != SVIHMM_WIDE_SWEEPS_16;
    // 128 < K <= 192: twelve waves of one state tile (three per SIMD; the eight two-tile waves would
    // run four empty tiles: 4.85 against 6.1 ms at K = 192, D = 32, T = 1e6).  SVIHMM_SWEEP_FAMILY_ONE_TILE:
    // one tile per wave for every K, _TILES: two tiles per wave for every K
    if (NW <= 12 && h->variant[SVIHMM_VAR_SWEEP_FAMILY] != SVIHMM_SWEEP_FAMILY_TILES) {
      if (K == 192) SWPX(12, true, true); else SWPX(12, false, true);
    }
    else if (h->variant[SVIHMM_VAR_SWEEP_FAMILY] == SVIHMM_SWEEP_FAMILY_ONE_TILE) {
      if (K == 256) SWPX(16, true, true); else SWPX(16, false, true);
    }
    else if (w32) { if (K == 256) SWP2(true, 2); else SWP2(false, 2); }
    else if (K == 256) SWP2(true, 1); else SWP2(false, 1);
#undef SWP2
  }
#undef SWP
#undef SWPX
  HIPCK(hipGetLastError());
  return 0;
}
// var_x of the last scaled sweep (B windows of length Lm), formed on first use
int ensure_q(svihmm_ctx* h, int B, int Lm, hipStream_t stream) {
  if (!h->lin_mode || h->q_valid) return 0;
  const int K = h->K;
  const int64_t n = (int64_t)B * Lm;
  CK(ensure(h->q, (size_t)n * K * sizeof(double)));
  ProfScope ps(h, KS_POSTERIOR, stream);
  dim3 grid((unsigned)((n + 15) / 16));
#define PQ(KT) hipLaunchKernelGGL(k_lin_posterior<KT>, grid, dim3(256), 0, stream, (const double*)h->la.p, \
                                  (const double*)h->lb.p, (const double*)h->hx.p, (const double*)h->gx.p,   \
                                  (const double2*)h->zfac.p, n, Lm, K, (double*)h->q.p, h->step_major ? B : 0)
#define PQF(KT) hipLaunchKernelGGL((k_lin_posterior<KT, float>), grid, dim3(256), 0, stream, (const float*)h->la.p, \
                                   (const float*)h->lb.p, (const double*)h->hx.p, (const double*)h->gx.p,          \
                                   (const double2*)h->zfac.p, n, Lm, K, (double*)h->q.p)
  if (h->cur_f32) { if (K <= 16) PQF(1); else if (K <= 32) PQF(2); else if (K <= 48) PQF(3); else if (K <= 64) PQF(4);
                    else if (K <= 128) PQF(8); else if (K <= 192) PQF(12); else PQF(16); }
  else if (K <= 16) PQ(1); else if (K <= 32) PQ(2); else if (K <= 48) PQ(3); else if (K <= 64) PQ(4);
  else if (K <= 128) PQ(8); else if (K <= 192) PQ(12); else PQ(16);
#undef PQ
#undef PQF
  HIPCK(hipGetLastError());
  h->q_valid = true;
  return 0;
}
// ELBO total still owed to packed[last] (set by the scaled sweeps, paid by k_finalize or here)
int launch_sum_lb(svihmm_ctx* h, int B, hipStream_t stream) {
  double* lbtot = (double*)h->packed.p + (packed_len(h) - 1);
  hipLaunchKernelGGL(k_sum_lb, dim3(1), dim3(256), 0, stream, (const double*)h->local_lb.p, B, lbtot);
  HIPCK(hipGetLastError());
  return 0;
}
// One long window (B = 1, the full-chain E-step) as an exact blocked scan over chunks of
// CHAIN_L steps: chunk matrices (S1), boundary vectors (S2), all chunks as concurrent windows
// with boundary conditions (S3).  See the comment above LinChain in kernels_recursion.h.
// chunk length: 256 steps give the most concurrent windows in S3; very long chains use 1024 so
// that the sequential boundary scan (S2) stays short (S1's work does not depend on it)
static int chain_len(int Lm) { return Lm >= 512 * 1024 ? 1024 : 256; }
bool use_chain(const svihmm_ctx* h, int B, int Lm) {
  return B == 1 && h->K <= 256 && Lm >= 2048 && h->variant[SVIHMM_VAR_CHAIN] != SVIHMM_CHAIN_OFF && !h->exact_log;
}
int launch_fb_chain(svihmm_ctx* h, int Lm, bool total) {
  const int K = h->K, T = Lm, L = chain_len(Lm);
  // state tiles the sweep kernels are instantiated for: exact up to 64 states, 8 / 16 tiles with
  // the transition tile streamed beyond (the chunk matrices are laid out for that width)
  const int NWt = (K + 15) / 16;
  const int NW = NWt <= 4 ? NWt : NWt <= 8 ? 8 : 16, Kp = 16 * NW;
  const bool full = (K == Kp);
  const int Cfull = (T - 2) / L;            // interior chunks; the tail chunk has 1..L steps
  const int C = Cfull + 1;
  const int ltail = T - 1 - Cfull * L;      // steps of the tail chunk (rows Cfull*L .. T-1)
  CK(ensure_fb_lin(h, 1, Lm));
  // chunk matrices + transposes + row exponents | boundary vectors and exponents | per-chunk scalars
  const size_t nM = (size_t)C * Kp * K;
  CK(ensure(h->chain, (2 * nM + (size_t)C * Kp + 2 * (size_t)(C + 1) * K + 7 * (size_t)(C + 1) + 8) * sizeof(double)));
  double* Mm = (double*)h->chain.p;
  double* MmT = Mm + nM;
  double* Mh = MmT + nM;
  double* abnd = Mh + (size_t)C * Kp;
  double* bbnd = abnd + (size_t)(C + 1) * K;
  double* aexp = bbnd + (size_t)(C + 1) * K;
  double* bexp = aexp + (C + 1);
  double* kbef = bexp + (C + 1);
  double* lbw = kbef + (C + 1);             // per-chunk local_lb
  double* lzw = lbw + (C + 1);              // scratch logz of the S3 windows
  double* ksum = lzw + (C + 1);             // per-chunk sums of the emission row exponents
  h->chain_kbef = kbef; h->chain_C = C; h->chain_L = L; h->chain_T = T;
  CK(ensure(h->chain2, (size_t)(C + 1) * sizeof(double2)));
  double2* zfw = (double2*)h->chain2.p;     // scratch zfac of the S3 windows (the global one comes from S2)
  const double* Eh = (const double*)(h->eh_in_llE ? h->llE.p : h->ll.p);
  const double* kx = (const double*)h->kexp.p;
  double* ah = (double*)h->la.p; double* bh = (double*)h->lb.p;
  double* hx = (double*)h->hx.p; double* gx = (double*)h->gx.p;
  const double* A = (const double*)h->Aexp.p; const double* At = (const double*)h->AexpT.p;
  const double* a0v = (const double*)h->a0v.p;
  const double* a0e = (const double*)h->a0e.p;
  hipStream_t st = h->stream;
  ProfScope ps(h, KS_FB, st);
  CK(launch_lin_init(h, 0, 1, Lm, st));
#define SWPM(NWV, F, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH)                       \
  hipLaunchKernelGGL((k_sweeps_lin<NWV, F, MD>), GRID, dim3(64 * NWV), sizeof(LinShared<NWV>), st, EHP, KXP, A, At, \
                     a0v, a0e, BB, LL, WS, K, AH, BH, HX, GX, LB, LZ, ZF, CH)
#define SWPB(NWV, F, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH)                       \
  do {                                                                                                      \
    hipFuncSetAttribute((const void*)k_sweeps_lin<NWV, F, MD, true>,                                        \
                        hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(LinShared<NWV>));           \
    hipLaunchKernelGGL((k_sweeps_lin<NWV, F, MD, true>), GRID, dim3(64 * NWV), sizeof(LinShared<NWV>), st,  \
                       EHP, KXP, A, At, a0v, a0e, BB, LL, WS, K, AH, BH, HX, GX, LB, LZ, ZF, CH);                 \
  } while (0)
#define SWPD(MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH)                                \
  do {                                                                                                      \
    if (NW == 8) { if (full) SWPB(8, true, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); \
                   else SWPB(8, false, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); }   \
    else if (NW == 16) { if (full) SWPB(16, true, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); \
                         else SWPB(16, false, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); } \
    else if (NW == 1) { if (full) SWPM(1, true, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); \
                   else SWPM(1, false, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); }   \
    else if (NW == 2) { if (full) SWPM(2, true, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); \
                        else SWPM(2, false, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); } \
    else if (NW == 3) { if (full) SWPM(3, true, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); \
                        else SWPM(3, false, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); } \
    else { if (full) SWPM(4, true, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH);         \
           else SWPM(4, false, MD, GRID, BB, LL, WS, EHP, KXP, AH, BH, HX, GX, LB, LZ, ZF, CH); }           \
  } while (0)
  LinChain ch = {};
  ch.Mout = Mm; ch.MoutT = MmT; ch.Mh = Mh;
  // S1: chunk matrices.  Interior chunks: L steps (rows c*L .. c*L+L); tail: ltail steps.
  if (Cfull > 0)
    SWPD(2, dim3((unsigned)(Cfull * NW), 1), Cfull, L + 1, L, Eh, kx, ah, bh, hx, gx, lbw, lzw, zfw, ch);
  {
    LinChain ct = ch;
    ct.Mout = Mm + (size_t)Cfull * Kp * K; ct.MoutT = MmT + (size_t)Cfull * Kp * K; ct.Mh = Mh + (size_t)Cfull * Kp;
    const size_t ro = (size_t)Cfull * L;
    SWPD(2, dim3((unsigned)NW, 1), 1, ltail + 1, L, Eh + ro * K, kx + ro, ah, bh, hx, gx, lbw, lzw, zfw, ct);
  }
  // S2: boundary vectors, Z
  hipLaunchKernelGGL(k_chunk_ksum, dim3(C), dim3(64), 0, st, kx, C, L, (int64_t)T, ksum);
#define SCAN(KM)                                                                                                   \
  do {                                                                                                             \
    const size_t lds = (size_t)4 * KM * 64 * sizeof(double);                                                       \
    if (lds > 64 * 1024)                                                                                           \
      hipFuncSetAttribute((const void*)k_chunk_scan<KM>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);    \
    hipLaunchKernelGGL(k_chunk_scan<KM>, dim3(2), dim3(256), lds, st, (const double*)Mm, (const double*)MmT,       \
                       (const double*)Mh, C, Kp, K, Eh, (const double*)ksum, a0v, a0e, abnd, aexp, bbnd, bexp, kbef,     \
                       (double2*)h->zfac.p, (double*)h->logz.p);                                                   \
  } while (0)
  if (K <= 16) SCAN(16); else if (K <= 32) SCAN(32); else if (K <= 64) SCAN(64);
  else
    hipLaunchKernelGGL(k_chunk_scan_wide, dim3(2), dim3(256), 0, st, (const double*)Mm, (const double*)MmT,
                       (const double*)Mh, C, Kp, K, Eh, (const double*)ksum, a0v, a0e, abnd, aexp, bbnd, bexp, kbef,
                       (double2*)h->zfac.p, (double*)h->logz.p);
#undef SCAN
  // S3: every chunk as a window with boundary conditions
  ch.init_vec = abnd; ch.init_exp = aexp; ch.kbefore = kbef;
  ch.term_vec = bbnd + K; ch.term_exp = bexp + 1;       // window c ends at boundary c + 1
  if (Cfull > 0)
    SWPD(1, dim3((unsigned)((Cfull + 15) / 16), 2), Cfull, L + 1, L, Eh, kx, ah, bh, hx, gx, lbw, lzw, zfw, ch);
  {
    LinChain ct = ch;
    ct.init_vec = abnd + (size_t)Cfull * K; ct.init_exp = aexp + Cfull; ct.kbefore = kbef + Cfull;
    const size_t ro = (size_t)Cfull * L;
    SWPD(3, dim3(1, 2), 1, ltail + 1, L, Eh + ro * K, kx + ro, ah + ro * K, bh + ro * K, hx + ro, gx + ro,
         lbw + Cfull, lzw + Cfull, zfw + Cfull, ct);
  }
#undef SWPD
#undef SWPB
#undef SWPM
  HIPCK(hipGetLastError());
  // local_lb[0] = sum of the chunks' parts (fixed order)
  hipLaunchKernelGGL(k_sum_lb, dim3(1), dim3(256), 0, st, (const double*)lbw, C, (double*)h->local_lb.p);
  if (total) {
    double* lbtot = (double*)h->packed.p + (packed_len(h) - 1);
    hipLaunchKernelGGL(k_sum_lb, dim3(1), dim3(256), 0, st, (const double*)lbw, C, lbtot);
  }
  HIPCK(hipGetLastError());
  return 0;
}

int launch_fb_lin(svihmm_ctx* h, int B, int Lm, bool total) {
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  if (use_chain(h, B, Lm)) {
    if (h->svi_flags && h->in_svi_estep) CK(wait_globals(h));    // (the chain kernels take no gate)
    return launch_fb_chain(h, Lm, total);
  }
  CK(ensure_fb_lin(h, B, Lm));
  CK(launch_fb_lin_range(h, 0, B, Lm, h->stream));
  if (total) h->lb_pending = B;   // summed by k_finalize's extra workgroup (or flush_lb)
  return 0;
}
int flush_lb(svihmm_ctx* h, hipStream_t stream) {
  if (!h->lb_pending) return 0;
  const int B = h->lb_pending;
  h->lb_pending = 0;
  return launch_sum_lb(h, B, stream);
}

int launch_scale_ll(svihmm_ctx* h, int B, int Lm) {
  const int64_t n = (int64_t)B * Lm;
  const int K = h->K;
  CK(ensure(h->llE, (size_t)n * K * sizeof(double)));
  CK(ensure(h->kexp, (size_t)n * sizeof(double)));
  ProfScope ps(h, KS_EMISSION);
  dim3 grid((unsigned)((n + 15) / 16));
#define SC(KT) hipLaunchKernelGGL(k_scale_ll<KT>, grid, dim3(256), 0, h->stream, (const double*)h->ll.p, \
                                  n, K, (double*)h->llE.p, (double*)h->kexp.p)
  if (K <= 16) SC(1); else if (K <= 32) SC(2); else if (K <= 48) SC(3); else if (K <= 64) SC(4);
  else if (K <= 128) SC(8); else if (K <= 192) SC(12); else SC(16);
#undef SC
  HIPCK(hipGetLastError());
  return 0;
}

int launch_scale_ll_f32(svihmm_ctx* h, int B, int Lm) {
  const int64_t n = (int64_t)B * Lm;
  const int K = h->K;
  CK(ensure(h->kexp, (size_t)n * sizeof(double)));
  ProfScope ps(h, KS_EMISSION);
  dim3 grid((unsigned)((n + 15) / 16));
#define SCF(KT) hipLaunchKernelGGL(k_scale_ll_f32<KT>, grid, dim3(256), 0, h->stream, (float*)h->ll.p, n, K, (double*)h->kexp.p)
  if (K <= 128) SCF(8); else if (K <= 192) SCF(12); else SCF(16);
#undef SCF
  HIPCK(hipGetLastError());
  return 0;
}

// Log-domain lliks / lalpha / lbeta of windows [b0, b0+nb) of the last (scaled) sweep,
// recomputed by the log-domain kernels into the m_* side buffers.
int materialise(svihmm_ctx* h, int b0, int nb) {
  if (h->m_nb > 0 && b0 >= h->m_b0 && b0 + nb <= h->m_b0 + h->m_nb) return 0;
  CK(wait_globals(h));
  if (h->lin_stale)
    return fail("log-domain intermediates of the last E-step are rebuilt on demand and the "
                "observations / globals / emission parameters have changed since: read them "
                "before the next parameter upload");
  const int Lm = h->lastLm, K = h->K;
  const size_t n = (size_t)nb * Lm * K * sizeof(double);
  CK(ensure(h->m_la, n));
  CK(ensure(h->m_lb, n));
  const double* ll;
  if (h->eh_in_llE) {   // the plain lliks are still in h->ll
    ll = (const double*)h->ll.p + (size_t)b0 * Lm * K;
  } else {
    CK(ensure(h->m_ll, n));
    CK(launch_emission(h, nb, Lm, h->last_flags, false, (const int64_t*)h->starts.p + b0,
                       (double*)h->m_ll.p));
    ll = (const double*)h->m_ll.p;
  }
  if (h->lastB == 1 && K <= 256 && h->chain_T == Lm && h->chain_kbef && use_chain(h, 1, Lm)) {
    // the blocked scan's messages -> logs (k_chain_lalpha both ways), entries lost to underflow
    // recomputed in the log domain row by row (k_lalpha_fix / k_lbeta_fix): no sequential pass
    const size_t ne = (size_t)Lm * K;
    CK(ensure(h->scratch, (2 * ne + 8) * sizeof(double)));
    double* ta = (double*)h->scratch.p;
    double* tb = ta + ne;
    double* ktop = tb + ne;
    const int64_t T = Lm;
    ProfScope ps(h, KS_FB);
    hipLaunchKernelGGL(k_ksum_all, dim3(1), dim3(256), 0, h->stream, (const double*)h->kexp.p, T, ktop);
    hipLaunchKernelGGL(k_chain_lalpha, dim3(h->chain_C), dim3(256), 0, h->stream, (const double*)h->la.p,
                       (const double*)h->hx.p, (const double*)h->kexp.p, h->chain_kbef, h->chain_L,
                       h->chain_C, T, K, ta, (const double*)nullptr);
    hipLaunchKernelGGL(k_chain_lalpha, dim3(h->chain_C), dim3(256), 0, h->stream, (const double*)h->lb.p,
                       (const double*)h->gx.p, (const double*)h->kexp.p, h->chain_kbef, h->chain_L,
                       h->chain_C, T, K, tb, (const double*)ktop);
    const unsigned nblk = (unsigned)((T + 63) / 64);
#define LFIX(KM)                                                                                                  \
  do {                                                                                                            \
    hipLaunchKernelGGL(k_lalpha_fix<KM>, dim3(nblk), dim3(256), 0, h->stream, (const double*)ta,                  \
                       (const double*)h->la.p, ll, (const double*)h->ltran.p, (const double*)h->mod_init.p, T, K, \
                       (double*)h->m_la.p);                                                                       \
    hipLaunchKernelGGL(k_lbeta_fix<KM>, dim3(nblk), dim3(256), 0, h->stream, (const double*)tb,                   \
                       (const double*)h->lb.p, ll, (const double*)h->ltran.p, T, K, (double*)h->m_lb.p);          \
  } while (0)
    if (K <= 16) LFIX(16); else if (K <= 32) LFIX(32); else if (K <= 64) LFIX(64);
    else {
      hipLaunchKernelGGL(k_lalpha_fix_wide, dim3(nblk), dim3(256), 0, h->stream, (const double*)ta,
                         (const double*)h->la.p, ll, (const double*)h->ltran.p, (const double*)h->mod_init.p, T, K,
                         (double*)h->m_la.p);
      hipLaunchKernelGGL(k_lbeta_fix_wide, dim3(nblk), dim3(256), (size_t)4 * K * sizeof(double), h->stream,
                         (const double*)tb, (const double*)h->lb.p, ll, (const double*)h->ltran.p, T, K,
                         (double*)h->m_lb.p);
    }
#undef LFIX
    HIPCK(hipGetLastError());
  } else {
    CK(launch_fb(h, nb, Lm, 0, 2, ll, (double*)h->m_la.p, (double*)h->m_lb.p));
  }
  h->m_b0 = b0; h->m_nb = nb;
  return 0;
}

// backward sampling from the device-resident lalpha[T,K] (hmm_fast.pyx:97-122): blocked
// composition of the per-row draw maps (K <= 256, T >= 1024), else the sequential single-wave
// sampler.  ffbs_plan: which of the two and the bytes of path / chunk-map scratch it needs;
// ffbs_launch: the launches alone, on device operands (lalpha rows, logA, one uniform per row) ->
// dz (device int64[T]); ffbs_draw: upload of logA and the uniforms + the launches, *dz_out in
// h->scratch, valid until the next call.
struct FfbsPlan { bool blocked; int KS, Ls, Cs; size_t extra; };
static FfbsPlan ffbs_plan(const svihmm_ctx* h, int64_t T, int K) {
  FfbsPlan pl;
  pl.blocked = K <= 256 && T >= 1024 && h->variant[SVIHMM_VAR_CHAIN] != SVIHMM_CHAIN_OFF;
  pl.KS = K <= 16 ? 16 : K <= 32 ? 32 : K <= 64 ? 64 : 256;      // path entries per row
  pl.Ls = T >= 65536 ? 512 : 256;
  pl.Cs = (int)((T + pl.Ls - 1) / pl.Ls);
  pl.extra = pl.blocked ? (size_t)T * pl.KS + 2 * (size_t)pl.Cs * pl.KS + (size_t)pl.Cs + 64 : 0;
  return pl;
}
static int ffbs_launch(svihmm_ctx* h, const FfbsPlan& pl, const double* la, int64_t T, int K, const double* dlogA,
                       const double* dun, int64_t* dz, unsigned char* path) {
  const int KS = pl.KS, Ls = pl.Ls, Cs = pl.Cs;
  unsigned char* mA = path + (size_t)T * KS;
  unsigned char* mB = mA + (size_t)Cs * KS;
  unsigned char* entry = mB + (size_t)Cs * KS;
  ProfScope ps(h, KS_FFBS);
  if (pl.blocked) {
#define FPATH(KM)                                                                                          \
  hipLaunchKernelGGL(k_ffbs_paths<KM>, dim3(Cs), dim3(64), ((size_t)K * (KM + 1) + 2 * KM) * sizeof(double), \
                     h->stream, la, dlogA, dun, T, K, Ls, path)
    if (KS == 16) FPATH(16); else if (KS == 32) FPATH(32); else if (KS == 64) FPATH(64);
    else
      hipLaunchKernelGGL(k_ffbs_paths_wide, dim3(Cs), dim3(256), 0, h->stream, la, dlogA, dun, T, K, Ls, path);
#undef FPATH
    hipLaunchKernelGGL(k_ffbs_compose, dim3(1), dim3(1024), 0, h->stream, (const unsigned char*)path, T, KS,
                       Ls, Cs, mA, mB, entry);
    hipLaunchKernelGGL(k_ffbs_gather, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, h->stream,
                       (const unsigned char*)path, (const unsigned char*)entry, T, KS, Ls, dz);
  } else {
    hipLaunchKernelGGL(k_ffbs_sample, dim3(1), dim3(64), K > 64 ? (size_t)K * 8 : 0, h->stream,
                       la, dlogA, dun, T, K, dz);
  }
  HIPCK(hipGetLastError());
  return 0;
}
static int ffbs_draw(svihmm_ctx* h, const double* la, int64_t T, int K, const double* logA,
                     const double* uniforms, int64_t** dz_out) {
  const FfbsPlan pl = ffbs_plan(h, T, K);
  const size_t base = ((size_t)K * K + (size_t)T) * sizeof(double) + (size_t)T * sizeof(int64_t);
  CK(ensure(h->scratch, base + pl.extra));
  double* dlogA = (double*)h->scratch.p;
  double* dun = dlogA + (size_t)K * K;
  int64_t* dz = (int64_t*)(dun + T);
  *dz_out = dz;
  HIPCK(hipMemcpyAsync(dlogA, logA, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(dun, uniforms, (size_t)T * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return ffbs_launch(h, pl, la, T, K, dlogA, dun, dz, (unsigned char*)(dz + T));
}

// The forward filter of the FFBS entry points: lalpha [B][Lm][K] of the windows, resident until the next
// call (*la_out).  One long chain (use_chain) through the exact blocked scan (scaled sweeps), then lalpha
// from (ah, h, K); everything else with the per-window log-domain kernel.  want_exact: the caller hands
// lalpha itself back, so the entries the scaled messages lost to underflow are repaired too.
static int ffbs_filter(svihmm_ctx* h, const int64_t* starts, int B, int Lm, uint32_t flags, bool want_exact,
                       const double** la_out) {
  const int K = h->K;
  const int64_t T = Lm;
  if (B == 1 && K <= 256 && use_chain(h, 1, Lm)) {
    CK(prepare_ll(h, starts, 1, Lm, flags, false, true));
    CK(launch_fb_chain(h, Lm, false));
    CK(ensure(h->m_la, (size_t)T * K * sizeof(double)));
    h->m_nb = 0;
    ProfScope ps(h, KS_FB);
    hipLaunchKernelGGL(k_chain_lalpha, dim3(h->chain_C), dim3(256), 0, h->stream, (const double*)h->la.p,
                       (const double*)h->hx.p, (const double*)h->kexp.p, h->chain_kbef, h->chain_L,
                       h->chain_C, T, K, (double*)h->m_la.p);
    HIPCK(hipGetLastError());
    const double* la = (const double*)h->m_la.p;
    if (want_exact) {
      // the caller wants lalpha itself: entries the scaled messages lost to underflow are
      // recomputed in the log domain (plain lliks into m_ll, corrected copy into m_lb)
      CK(ensure(h->m_lb, (size_t)T * K * sizeof(double)));
      const double* llp = (const double*)h->ll.p;     // host-supplied / two-pass lliks are still there
      if (!h->eh_in_llE) {
        CK(ensure(h->m_ll, (size_t)T * K * sizeof(double)));
        CK(launch_emission(h, 1, Lm, flags, false, nullptr, (double*)h->m_ll.p));
        llp = (const double*)h->m_ll.p;
      }
      const unsigned nblk = (unsigned)((T + 63) / 64);
#define LFIX(KM) hipLaunchKernelGGL(k_lalpha_fix<KM>, dim3(nblk), dim3(256), 0, h->stream, la, (const double*)h->la.p, \
                                    llp, (const double*)h->ltran.p,                                              \
                                    (const double*)h->mod_init.p, T, K, (double*)h->m_lb.p)
      if (K <= 16) LFIX(16); else if (K <= 32) LFIX(32); else if (K <= 64) LFIX(64);
      else
        hipLaunchKernelGGL(k_lalpha_fix_wide, dim3(nblk), dim3(256), 0, h->stream, la, (const double*)h->la.p, llp,
                           (const double*)h->ltran.p, (const double*)h->mod_init.p, T, K, (double*)h->m_lb.p);
#undef LFIX
      HIPCK(hipGetLastError());
      la = (const double*)h->m_lb.p;
    }
    *la_out = la;
  } else {
    CK(prepare_ll(h, starts, B, Lm, flags, false));
    CK(launch_fb(h, B, Lm, 0, 1));
    *la_out = (const double*)h->la.p;
  }
  return 0;
}

int svihmm_ffbs(svihmm_ctx* h, const double* logA, const double* uniforms, uint32_t flags,
                int64_t* out_z, double* out_lalpha) {
  if (!h || !logA || !uniforms || !out_z) return fail("svihmm_ffbs: bad arguments");
  CK(set_device(h));
  const int64_t T = h->T;
  if (T <= 0) return fail("svihmm_ffbs: no observations");
  if (T > 2147483647LL) return fail("svihmm_ffbs: T too large");
  int64_t st0 = 0;
  const int K = h->K;
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  CK(wait_globals(h));
  const double* la = nullptr;
  CK(ffbs_filter(h, &st0, 1, (int)T, flags, out_lalpha != nullptr, &la));
  int64_t* dz = nullptr;
  CK(ffbs_draw(h, la, T, K, logA, uniforms, &dz));
  CK(d2h(h, out_z, dz, (size_t)T * sizeof(int64_t)));
  if (out_lalpha) CK(d2h(h, out_lalpha, la, (size_t)T * K * sizeof(double)));
  HIPCK(hipStreamSynchronize(h->stream));
  h->lastB = 1; h->lastLm = (int)T;
  return 0;
}

// The device inputs and output of the window / sequence samplers in h->vit: logA | z int32 [n] | the caller's
// uniforms [n] (null: Philox), n = draws x rows; logA and the uniforms are uploaded here.
struct FfbsIo { double* logA; int32_t* z; double* unif; };
static int ffbs_io(svihmm_ctx* h, const double* logA, const double* uniforms, size_t n, FfbsIo* io) {
  const int K = h->K;
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_z = up((size_t)K * K * sizeof(double)), o_u = o_z + up(n * sizeof(int32_t));
  CK(ensure(h->vit, o_u + (uniforms ? n * sizeof(double) : 0) + 256));
  char* base = (char*)h->vit.p;
  io->logA = (double*)base;
  io->z = (int32_t*)(base + o_z);
  io->unif = uniforms ? (double*)(base + o_u) : nullptr;
  HIPCK(hipMemcpyAsync(io->logA, logA, (size_t)K * K * sizeof(double), hipMemcpyHostToDevice, h->stream));
  if (uniforms) HIPCK(hipMemcpyAsync(io->unif, uniforms, n * sizeof(double), hipMemcpyHostToDevice, h->stream));
  return 0;
}
// Long windows / sequences: the blocked composition of ffbs_launch once per (unit, draw).  The per-draw scratch in
// h->scratch = (Philox: uniforms [maxlen]) | z int64 [maxlen] | path, chunk maps is reused by every draw.
// ffbs_blocked_draw: the path of `len` rows from the unit's lalpha rows `la` into io.z[g0 ..]; its uniforms are
// entries g0 .. of the caller's, or of the Philox stream.
struct FfbsBlockedScratch { double* unif; int64_t* z; unsigned char* path; };
static int ffbs_blocked_scratch(svihmm_ctx* h, const FfbsIo& io, int64_t maxlen, size_t extra, FfbsBlockedScratch* sc) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_zl = io.unif ? 0 : up((size_t)maxlen * sizeof(double));
  const size_t o_path = o_zl + up((size_t)maxlen * sizeof(int64_t));
  CK(ensure(h->scratch, o_path + extra));
  char* sb = (char*)h->scratch.p;
  sc->unif = (double*)sb;
  sc->z = (int64_t*)(sb + o_zl);
  sc->path = (unsigned char*)(sb + o_path);
  return 0;
}
static int ffbs_blocked_draw(svihmm_ctx* h, const FfbsIo& io, const FfbsBlockedScratch& sc, uint64_t seed,
                             const double* la, int64_t len, int64_t g0) {
  const unsigned nb256 = (unsigned)((len + 255) / 256);
  if (!io.unif) {
    ProfScope ps(h, KS_FFBS);
    hipLaunchKernelGGL(k_ffw_fill_uniforms, dim3(nb256), dim3(256), 0, h->stream, (unsigned long long)seed, g0, len,
                       sc.unif);
  }
  CK(ffbs_launch(h, ffbs_plan(h, len, h->K), la, len, h->K, io.logA, io.unif ? io.unif + g0 : sc.unif, sc.z, sc.path));
  ProfScope ps(h, KS_FFBS);
  hipLaunchKernelGGL(k_ffw_store_path, dim3(nb256), dim3(256), 0, h->stream, (const int64_t*)sc.z, len, io.z + g0);
  return 0;
}

// svihmm_ffbs_windows: one forward filter over the windows (ffbs_filter), then S backward draws of every window
// from the resident lalpha.  Windows below FFW_SWITCH rows: one launch, a lane per (window, draw) pair
// (kernels_ffbs_windows.h).  Longer ones -- the whole chain included -- run the blocked composition once per
// (window, draw) on la + b Lm K (ffbs_blocked_draw).  Nothing scales with S T K.
// *dz_out (int32 [S][B][Lm]) / *dla_out (lalpha [B][Lm][K]) stay valid until the next call.
int launch_ffbs_windows(svihmm_ctx* h, const int64_t* starts, int B, int Lm, uint32_t flags, const double* logA,
                        int S, const double* uniforms, uint64_t seed, bool want_lalpha, int32_t** dz_out,
                        const double** dla_out) {
  const int K = h->K;
  if (K > 256) return fail("svihmm_ffbs_windows: K > 256 not supported");
  CK(wait_globals(h));
  const double* la = nullptr;
  CK(ffbs_filter(h, starts, B, Lm, flags, want_lalpha, &la));
  h->have_lb = false;
  h->lastB = B; h->lastLm = Lm;
  FfbsIo io;
  CK(ffbs_io(h, logA, uniforms, (size_t)S * B * Lm, &io));
  *dz_out = io.z;
  *dla_out = la;
  if (Lm < FFW_SWITCH) {
    const unsigned nblk = (unsigned)(((int64_t)B * S + 63) / 64);
    ProfScope ps(h, KS_FFBS);
    if (K <= 64) {
      const int KM = K <= 16 ? 16 : K <= 32 ? 32 : 64;
      const int nwmax = ffw_windows_per_wave(B, S), RT = ffw_row_tile(nwmax, KM, Lm);
      const size_t lds = ffw_lds_bytes(K, KM, nwmax, RT);
#define FWIN(KMAX)                                                                                                  \
  do {                                                                                                              \
    if (lds > 64 * 1024)                                                                                            \
      hipFuncSetAttribute((const void*)k_ffbs_win<KMAX>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);     \
    hipLaunchKernelGGL(k_ffbs_win<KMAX>, dim3(nblk), dim3(64), lds, h->stream, la, (const double*)io.logA,          \
                       (const double*)io.unif, (unsigned long long)seed, B, S, Lm, K, nwmax, RT, io.z);             \
  } while (0)
      if (KM == 16) FWIN(16); else if (KM == 32) FWIN(32); else FWIN(64);
#undef FWIN
    } else {
      hipLaunchKernelGGL(k_ffbs_win_wide, dim3(nblk), dim3(64), 0, h->stream, la, (const double*)io.logA,
                         (const double*)io.unif, (unsigned long long)seed, B, S, Lm, K, io.z);
    }
    HIPCK(hipGetLastError());
    return 0;
  }
  FfbsBlockedScratch sc;
  CK(ffbs_blocked_scratch(h, io, Lm, ffbs_plan(h, Lm, K).extra, &sc));
  for (int s = 0; s < S; ++s)
    for (int b = 0; b < B; ++b)
      CK(ffbs_blocked_draw(h, io, sc, seed, la + (size_t)b * Lm * K, Lm, ((int64_t)s * B + b) * Lm));
  HIPCK(hipGetLastError());
  return 0;
}

// hmm_fast.pyx:80-95: with lalpha_init supplied the reference skips the filter and only samples
int svihmm_ffbs_sample(svihmm_ctx* h, int64_t T, int32_t K, const double* lalpha, const double* logA,
                       const double* uniforms, int64_t* out_z) {
  if (!h || !lalpha || !logA || !uniforms || !out_z || T <= 0 || K <= 0)
    return fail("svihmm_ffbs_sample: bad arguments");
  if (T > 2147483647LL) return fail("svihmm_ffbs_sample: T too large");
  CK(set_device(h));
  const size_t n = (size_t)T * K * sizeof(double);
  CK(ensure(h->m_la, n));
  h->m_nb = 0;
  HIPCK(hipMemcpyAsync(h->m_la.p, lalpha, n, hipMemcpyHostToDevice, h->stream));
  int64_t* dz = nullptr;
  CK(ffbs_draw(h, (const double*)h->m_la.p, T, K, logA, uniforms, &dz));
  CK(d2h(h, out_z, dz, (size_t)T * sizeof(int64_t)));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}

// h->vit of the Viterbi launchers: score [nscore] | z int32 [nz] | final argmax [nlast] | psi | path (P padded rows of
// KS bytes each) | chunk maps mA, mB [C][KS] | entry [C].  P = C = 0 when every unit backtracks inside its launch.
struct VitScratch { double* score; int32_t *z, *zlast; unsigned char *psi, *path, *mA, *mB, *entry; };
static int vit_scratch(svihmm_ctx* h, size_t nscore, size_t nz, size_t nlast, int64_t P, int64_t C, int KS,
                       VitScratch* v) {
  size_t o = 0;
  auto take = [&o](size_t bytes) { const size_t at = o; o += (bytes + 255) & ~(size_t)255; return at; };
  const size_t o_score = take(nscore * sizeof(double)), o_z = take(nz * sizeof(int32_t));
  const size_t o_zlast = take(nlast * sizeof(int32_t));
  const size_t o_psi = take((size_t)P * KS), o_path = take((size_t)P * KS);
  const size_t o_mA = take((size_t)C * KS), o_mB = take((size_t)C * KS), o_entry = take((size_t)C);
  CK(ensure(h->vit, o + 256));
  char* base = (char*)h->vit.p;
  v->score = (double*)(base + o_score);
  v->z = (int32_t*)(base + o_z);
  v->zlast = (int32_t*)(base + o_zlast);
  v->psi = (unsigned char*)(base + o_psi);
  v->path = (unsigned char*)(base + o_path);
  v->mA = (unsigned char*)(base + o_mA);
  v->mB = (unsigned char*)(base + o_mB);
  v->entry = (unsigned char*)(base + o_entry);
  return 0;
}

// svihmm_viterbi: max-plus forward sweep + backtrack over the lliks ll [B*Lm, K] with the globals currently set.
// Windows whose psi fits the LDS budget (kernels_viterbi.h: Lm <= vit_lds_rows(KS)) are decoded in one launch;
// longer ones write psi to HBM and backtrack by composing chunk maps (k_vit_paths, k_ffbs_compose, k_vit_gather).
// *dz_out (int32 [B*Lm], only when want_z) and *dscore_out (double [B]) live in h->vit until the next call.
int launch_viterbi(svihmm_ctx* h, int B, int Lm, const double* ll, bool want_z, int32_t** dz_out,
                   double** dscore_out) {
  const int K = h->K;
  if (K > 256) return fail("svihmm_viterbi: K > 256 not supported (one-byte back-pointers)");
  const int KS = K <= 64 ? 64 : 256;
  const int Ls = vit_lds_rows(KS);
  const bool in_lds = Lm <= Ls;
  const int Cw = (Lm + Ls - 1) / Ls;
  const int64_t Lpad = (int64_t)Cw * Ls;
  const int64_t C = (int64_t)B * Cw;
  if (!in_lds && C * KS >= ((int64_t)1 << 31)) return fail("svihmm_viterbi: too many row chunks for the map composition");
  const size_t n = (size_t)B * Lm;
  VitScratch v;
  CK(vit_scratch(h, B, n, B, in_lds ? 0 : B * Lpad, in_lds ? 0 : C, KS, &v));
  *dz_out = want_z ? v.z : nullptr;
  *dscore_out = v.score;
  const VitWindows units{Lm, Lpad};
  ProfScope ps(h, KS_MISC);
  const size_t lds = (size_t)2 * KS * 8 + (in_lds && want_z ? (size_t)Lm * KS : 0);
  if (in_lds) vit_sweep<true>(h, B, lds, ll, units, nullptr, want_z ? v.z : nullptr, nullptr, v.score);
  else vit_sweep<false>(h, B, lds, ll, units, v.psi, nullptr, v.zlast, v.score);
  HIPCK(hipGetLastError());
  if (!in_lds && want_z) {
    hipLaunchKernelGGL(k_vit_paths<VitWindows>, dim3((unsigned)C), dim3(KS), (size_t)Ls * KS, h->stream,
                       (const unsigned char*)v.psi, (const int32_t*)v.zlast, units, Ls, KS, K, v.path);
    hipLaunchKernelGGL(k_ffbs_compose, dim3(1), dim3(1024), 0, h->stream, (const unsigned char*)v.path, (int64_t)B * Lpad,
                       KS, Ls, (int)C, v.mA, v.mB, v.entry);
    hipLaunchKernelGGL(k_vit_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, h->stream,
                       (const unsigned char*)v.path, (const unsigned char*)v.entry, Lm, Ls, Cw, Lpad, KS, (int64_t)n, v.z);
    HIPCK(hipGetLastError());
  }
  return 0;
}

// svihmm_grow_windows, product route (kernels_grow.h): one workgroup per centre over the lliks ll [n][W][K] of the
// centres' reach windows; off[i] = the centre's row inside its window, smax[i] = the growth steps the sequence ends
// and the cutoff allow (host arrays, checked against the window here: the kernel reads rows off - bmax .. off + bmax).
// Results live in h->vit until the next call: *half_out / *steps_out int32 [n], *trace_out double [n][trace_cap][2].
int launch_grow_products(svihmm_ctx* h, int n, int W, const double* ll, const int32_t* off, const int32_t* smax,
                         int half0, int m, int inc, double eps, int rule, int trace_cap, int32_t** half_out,
                         int32_t** steps_out, double** trace_out) {
  const int K = h->K;
  if (K > 64 || h->exact_log) return fail("svihmm_grow_windows: the product kernel needs K <= 64 and linear-range globals");
  for (int i = 0; i < n; ++i) {
    const int64_t reach = (int64_t)half0 + (int64_t)inc * smax[i];
    if (smax[i] < 0 || off[i] - reach < 0 || off[i] + reach >= W)
      return fail("svihmm_grow_windows: internal error: centre " + std::to_string(i) + " reaches outside its lliks window");
  }
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t o_trace = 0, o_off = up((size_t)n * trace_cap * 2 * sizeof(double));
  const size_t o_smax = o_off + up((size_t)n * 4), o_half = o_smax + up((size_t)n * 4), o_steps = o_half + up((size_t)n * 4);
  CK(ensure(h->vit, o_steps + up((size_t)n * 4)));
  char* base = (char*)h->vit.p;
  double* dtrace = trace_cap > 0 ? (double*)(base + o_trace) : nullptr;
  int32_t* doff = (int32_t*)(base + o_off);
  int32_t* dsmax = (int32_t*)(base + o_smax);
  int32_t* dhalf = (int32_t*)(base + o_half);
  int32_t* dsteps = (int32_t*)(base + o_steps);
  HIPCK(hipMemcpyAsync(doff, off, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(dsmax, smax, (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
  // (pageable sources: the two host arrays must not change before the copies have left them)
  HIPCK(hipStreamSynchronize(h->stream));
  const double* A = (const double*)h->Aexp.p;
  const double* mi = (const double*)h->mod_init.p;
  ProfScope ps(h, KS_FB);
#define GROWP(NT)                                                                                                  \
  do {                                                                                                             \
    const size_t lds = grow_lds_bytes(NT);                                                                         \
    if (lds > 64 * 1024)                                                                                           \
      HIPCK(hipFuncSetAttribute((const void*)k_grow_products<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds)); \
    hipLaunchKernelGGL(k_grow_products<NT>, dim3(n), dim3(GROW_THREADS), lds, h->stream, ll, A, mi,                \
                       (const int32_t*)doff, (const int32_t*)dsmax, W, K, half0, m, inc, eps, rule, dhalf, dsteps, \
                       dtrace, trace_cap);                                                                         \
  } while (0)
  if (K <= 16) GROWP(1); else if (K <= 32) GROWP(2); else if (K <= 48) GROWP(3); else GROWP(4);
#undef GROWP
  HIPCK(hipGetLastError());
  *half_out = dhalf; *steps_out = dsteps; *trace_out = dtrace;
  return 0;
}

// svihmm_grow_windows, literal route: the rule's state on the device.  launch_grow_state lays it out in h->vit and
// uploads its initial value (init: [n][6] doubles, centers: [n]); launch_grow_probe folds one candidate's posteriors
// q [nact][2 b + 1][K] (window j = centre idx[j]) into it and leaves the centres' "grows again" flags in *active_out.
struct GrowState { double *qold, *st, *trace; int64_t* centers; int32_t *ist, *active, *idx; };
static GrowState grow_state(svihmm_ctx* h, int n, int trace_cap) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const int K = h->K;
  char* base = (char*)h->vit.p;
  GrowState g;
  size_t o = 0;
  g.trace = (double*)(base + o); o += up((size_t)n * trace_cap * 2 * sizeof(double));
  g.qold = (double*)(base + o); o += up((size_t)n * 2 * K * sizeof(double));
  g.st = (double*)(base + o); o += up((size_t)n * 6 * sizeof(double));
  g.centers = (int64_t*)(base + o); o += up((size_t)n * sizeof(int64_t));
  g.ist = (int32_t*)(base + o); o += up((size_t)n * 3 * 4);
  g.active = (int32_t*)(base + o); o += up((size_t)n * 4);
  g.idx = (int32_t*)(base + o);
  return g;
}
int launch_grow_state(svihmm_ctx* h, int n, int trace_cap, const int64_t* centers, const double* init) {
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t bytes = up((size_t)n * trace_cap * 2 * 8) + up((size_t)n * 2 * h->K * 8) + up((size_t)n * 48) +
                       up((size_t)n * 8) + up((size_t)n * 12) + 2 * up((size_t)n * 4);
  CK(ensure(h->vit, bytes));
  const GrowState g = grow_state(h, n, trace_cap);
  // trace: NaN beyond a centre's steps (all bits set is a quiet NaN); everything else zero
  if (trace_cap > 0) HIPCK(hipMemsetAsync(g.trace, 0xff, (size_t)n * trace_cap * 2 * 8, h->stream));
  HIPCK(hipMemsetAsync(g.qold, 0, (size_t)n * 2 * h->K * 8, h->stream));
  HIPCK(hipMemsetAsync(g.ist, 0, (size_t)n * 12, h->stream));
  HIPCK(hipMemcpyAsync(g.st, init, (size_t)n * 48, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipMemcpyAsync(g.centers, centers, (size_t)n * 8, hipMemcpyHostToDevice, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}
int launch_grow_probe(svihmm_ctx* h, int n, int nact, const int32_t* idx, int b, int m, bool first, int inc, int cutoff,
                      double eps, int rule, int trace_cap, int32_t* active_host) {
  const GrowState g = grow_state(h, n, trace_cap);
  HIPCK(hipMemcpyAsync(g.idx, idx, (size_t)nact * 4, hipMemcpyHostToDevice, h->stream));
  {
    ProfScope ps(h, KS_MISC);
    hipLaunchKernelGGL(k_grow_probe, dim3(nact), dim3(64), 0, h->stream, (const double*)h->q.p, 2 * b + 1, h->K, b, m,
                       (const int32_t*)g.idx, first ? 1 : 0, (const int64_t*)g.centers, (int64_t)h->T, inc, cutoff, eps,
                       rule, g.qold, g.st, g.ist, g.active, trace_cap > 0 ? g.trace : (double*)nullptr, trace_cap);
    HIPCK(hipGetLastError());
  }
  HIPCK(hipMemcpyAsync(active_host, g.active, (size_t)n * 4, hipMemcpyDeviceToHost, h->stream));
  HIPCK(hipStreamSynchronize(h->stream));
  return 0;
}
// the literal route's results (device pointers into h->vit): ist [n][3] = half-width, steps, count; trace
int grow_state_results(svihmm_ctx* h, int n, int trace_cap, const int32_t** ist_out, const double** trace_out) {
  const GrowState g = grow_state(h, n, trace_cap);
  *ist_out = g.ist; *trace_out = g.trace;
  return 0;
}

// ---- svihmm_estep_sequences (kernels_sequences.h) ----------------------------------------------
// The ragged sweeps over the nseq sequences listed in `order` (device, longest first), ndir directions of them: 2 =
// forward and backward (la, lb), 1 = the forward filter alone (lb null; the kernels take the direction from
// blockIdx.y).  ll's row 0 is global row row_base.
static int launch_seq_sweeps(svihmm_ctx* h, int nseq, int ndir, const int32_t* order, const int64_t* seq_off,
                             int64_t row_base, const double* ll, double* la, double* lb) {
  const int K = h->K;
  const double* A = (const double*)h->Aexp.p;
  const double* mi = (const double*)h->mod_init.p;
  dim3 grid((unsigned)nseq, (unsigned)ndir);
  ProfScope ps(h, KS_FB);
  if (h->exact_log) {
    const int threads = (K + 63) / 64 * 64;
    const int in_lds = ((size_t)K * (K + 1) + 2 * K) * 8 <= 150 * 1024;
    const size_t lds = (2 * (size_t)K + (in_lds ? (size_t)K * (K + 1) : 0)) * 8;
    if (lds > 64 * 1024)
      hipFuncSetAttribute((const void*)k_seq_exact, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_seq_exact, grid, dim3(threads), lds, h->stream, ll, row_base, seq_off, order,
                       (const double*)h->ltran.p, mi, K, in_lds, la, lb);
  } else if (K <= 16)
    hipLaunchKernelGGL(k_seq_wave<16>, grid, dim3(64), 0, h->stream, ll, row_base, seq_off, order, A, mi, K, la, lb);
  else if (K <= 32)
    hipLaunchKernelGGL(k_seq_wave<32>, grid, dim3(64), 0, h->stream, ll, row_base, seq_off, order, A, mi, K, la, lb);
  else if (K <= 64)
    hipLaunchKernelGGL(k_seq_wave<64>, grid, dim3(64), 0, h->stream, ll, row_base, seq_off, order, A, mi, K, la, lb);
  else {
    const int threads = (K + 63) / 64 * 64;
    const int in_lds = ((size_t)K * K * 8 + 2 * K * 8 + 128) <= 150 * 1024;
    const size_t lds = (2 * (size_t)K + 16) * 8 + (in_lds ? (size_t)K * K * 8 : 0);
    if (lds > 64 * 1024)
      hipFuncSetAttribute((const void*)k_seq_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_seq_block, grid, dim3(threads), lds, h->stream, ll, row_base, seq_off, order, A,
                       (const double*)h->AexpT.p, mi, K, in_lds, la, lb);
  }
  HIPCK(hipGetLastError());
  return 0;
}
// Sweeps + posterior over the span rows of those sequences -> posterior rows at their global index in q [T][K] and
// seq_lb[s].  lalpha / lbeta / the per-row LSE live in h->seq_work, which no other route touches.  maxlen: the longest
// of the sequences.
int launch_fb_sequences(svihmm_ctx* h, int nseq, const int32_t* order, const int64_t* seq_off, int64_t row_base,
                        int64_t span, int maxlen, const double* ll, double* q, double* seq_lb) {
  if (!h->have_globals) return fail("no globals: call svihmm_set_globals");
  const int K = h->K;
  if (K > 256) return fail("svihmm_estep_sequences: K > 256 not supported");
  const size_t ne = (size_t)span * K;
  CK(ensure(h->seq_work, (2 * ne + (size_t)span) * sizeof(double)));
  double* la = (double*)h->seq_work.p;
  double* lb = la + ne;
  double* row_lse = lb + ne;
  CK(launch_seq_sweeps(h, nseq, 2, order, seq_off, row_base, ll, la, lb));
  {
    ProfScope ps(h, KS_POSTERIOR);
    // 64 rows per posterior workgroup of the longest sequence, at most 1024 workgroups per sequence
    int nseg = (maxlen + 63) / 64;
    if (nseg > 1024) nseg = 1024;
    if (nseg < 1) nseg = 1;
    dim3 gp((unsigned)nseq, (unsigned)nseg);
#define SEQ_POST(KPL)                                                                                        \
  hipLaunchKernelGGL(k_seq_posterior<KPL>, gp, dim3(256), 0, h->stream, (const double*)la, (const double*)lb, \
                     row_base, seq_off, order, K, q, row_lse)
    if (K <= 64) SEQ_POST(1); else SEQ_POST(4);
#undef SEQ_POST
    hipLaunchKernelGGL(k_seq_lb, dim3((unsigned)nseq), dim3(64), 0, h->stream, (const double*)row_lse, row_base,
                       seq_off, order, seq_lb);
    HIPCK(hipGetLastError());
  }
  return 0;
}
// behind launch_stats_posteriors over the concatenated posteriors as ONE window: the boundary correction of A_raw
// (join pairs out, with `wrap` each sequence's own wrap pair in), q0, and the ELBO total into the packed lb slot
int launch_seq_finish(svihmm_ctx* h, int N, const int64_t* seq_off, bool wrap, const double* q, const double* seq_lb,
                      double* q0) {
  const int K = h->K;
  ProfScope ps(h, KS_STATS);
  hipLaunchKernelGGL(k_seq_fix, dim3((unsigned)((K * K + 255) / 256 + 1)), dim3(256), 0, h->stream, q, seq_off, N, K,
                     wrap ? 1 : 0, (double*)h->packed.p, q0);
  hipLaunchKernelGGL(k_sum_lb, dim3(1), dim3(256), 0, h->stream, seq_lb, N,
                     (double*)h->packed.p + (packed_len(h) - 1));
  HIPCK(hipGetLastError());
  return 0;
}
// svihmm_estep_sequence_subset: the M listed sequences of the resident rows (and mask bytes) into the compact copy
// obs_out [R][D] / mask_out [R].  tab (device): dst_off [M + 1] | src_off [M], in rows.  maxlen: the longest of them.
int launch_seq_gather(svihmm_ctx* h, int M, const int64_t* tab, int maxlen, double* obs_out, uint8_t* mask_out,
                      int32_t* labels_out, uint64_t* sets_out) {
  // 8 KiB of rows per workgroup and pass, at most 1024 workgroups per occurrence
  int64_t nseg = ((int64_t)maxlen * h->D * 8 + 8191) / 8192;
  if (nseg > 1024) nseg = 1024;
  if (nseg < 1) nseg = 1;
  ProfScope ps(h, KS_MISC);
  hipLaunchKernelGGL(k_seq_gather, dim3((unsigned)M, (unsigned)nseg), dim3(256), 0, h->stream,
                     (const unsigned long long*)h->obs.p, h->have_mask ? (const uint8_t*)h->mask.p : nullptr, tab,
                     tab + M + 1, h->D, (unsigned long long*)obs_out, h->have_mask ? mask_out : nullptr);
  // labels in force: the listed sequences' labels travel the same way (k_label_gather, the same grid)
  if (h->have_labels)
    hipLaunchKernelGGL(k_label_gather, dim3((unsigned)M, (unsigned)nseg), dim3(256), 0, h->stream,
                       (const int32_t*)h->labels.p, tab, tab + M + 1, labels_out);
  if (h->have_sets)
    hipLaunchKernelGGL(k_set_gather, dim3((unsigned)M, (unsigned)nseg), dim3(256), 0, h->stream,
                       (const unsigned long long*)h->sets.p, tab, tab + M + 1, h->sets_W,
                       (unsigned long long*)sets_out);
  HIPCK(hipGetLastError());
  return 0;
}

// ---- decoding all declared sequences in one call (kernels_decode_sequences.h) -------------------
// svihmm_viterbi_sequences.  Sequences whose psi fits the LDS budget (len <= vit_lds_rows(KS); all of them when no
// path is wanted) are decoded inside the forward launch; all longer ones go in ONE forward launch that writes psi
// to a common run of padded chunks, backtracked by k_vit_paths / k_ffbs_compose / k_vitseq_gather.
// A launch's dynamic LDS is one number: the short sequences go in ONE launch sized by the longest of them (cutting
// them into several launches by LDS request measured slower: DESIGN.md section 4, "Decoding several sequences").
// h->vit: vit_scratch.  h->dec_tab: pad_off int64 [long] | order (short) | order (long) | chunk table.
int64_t viterbi_sequences_chunks(const svihmm_ctx* h) {
  const int Ls = vit_lds_rows(h->K <= 64 ? 64 : 256);
  int64_t C = 0;
  for (size_t s = 0; s + 1 < h->seq_off.size(); ++s) {
    const int64_t len = h->seq_off[s + 1] - h->seq_off[s];
    if (len > Ls) C += (len + Ls - 1) / Ls;
  }
  return C;
}
int launch_viterbi_sequences(svihmm_ctx* h, const double* ll, bool want_z, int32_t** dz_out, double** dscore_out) {
  const int K = h->K, N = (int)h->seq_off.size() - 1;
  const int64_t T = h->T;
  const std::vector<int64_t>& so = h->seq_off;
  const int KS = K <= 64 ? 64 : 256, Ls = vit_lds_rows(KS);
  std::vector<int32_t> shorts, longs;
  for (int s = 0; s < N; ++s) ((!want_z || so[s + 1] - so[s] <= Ls) ? shorts : longs).push_back(s);
  const auto longer = [&so](int32_t a, int32_t b) { return so[a + 1] - so[a] > so[b + 1] - so[b]; };
  std::stable_sort(shorts.begin(), shorts.end(), longer);     // longest first (ties in ascending s)
  std::stable_sort(longs.begin(), longs.end(), longer);
  const size_t ns = shorts.size(), nl = longs.size();
  std::vector<int64_t> pad(nl);
  std::vector<int32_t> ctab;
  int64_t P = 0;
  for (size_t u = 0; u < nl; ++u) {
    const int Cw = (int)((so[longs[u] + 1] - so[longs[u]] + Ls - 1) / Ls);
    pad[u] = P;
    for (int cw = 0; cw < Cw; ++cw) { ctab.push_back((int32_t)u); ctab.push_back(cw); }
    P += (int64_t)Cw * Ls;
  }
  const int64_t C = (int64_t)ctab.size() / 2;
  const size_t t_os = nl * sizeof(int64_t), t_ol = t_os + ns * sizeof(int32_t), t_ct = t_ol + nl * sizeof(int32_t);
  const size_t t_end = t_ct + ctab.size() * sizeof(int32_t);
  h->dec_host.resize(t_end);
  if (nl) {
    std::memcpy(h->dec_host.data(), pad.data(), nl * sizeof(int64_t));
    std::memcpy(h->dec_host.data() + t_ol, longs.data(), nl * sizeof(int32_t));
    std::memcpy(h->dec_host.data() + t_ct, ctab.data(), ctab.size() * sizeof(int32_t));
  }
  if (ns) std::memcpy(h->dec_host.data() + t_os, shorts.data(), ns * sizeof(int32_t));
  CK(ensure(h->dec_tab, t_end + 256));
  HIPCK(hipMemcpyAsync(h->dec_tab.p, h->dec_host.data(), t_end, hipMemcpyHostToDevice, h->stream));
  const char* tb = (const char*)h->dec_tab.p;
  const int64_t* dpad = (const int64_t*)tb;
  const int32_t* dos = (const int32_t*)(tb + t_os);
  const int32_t* dol = (const int32_t*)(tb + t_ol);
  const int32_t* dct = (const int32_t*)(tb + t_ct);
  VitScratch v;
  CK(vit_scratch(h, N, (size_t)T, nl, P, C, KS, &v));
  *dz_out = want_z ? v.z : nullptr;
  *dscore_out = v.score;
  const int64_t* sod = (const int64_t*)h->seq_off_d.p;
  ProfScope ps(h, KS_MISC);
  if (ns) {
    const int64_t la = so[shorts[0] + 1] - so[shorts[0]];
    const size_t lds = (size_t)2 * KS * 8 + (want_z ? (size_t)la * KS : 0);
    vit_sweep<true>(h, (unsigned)ns, lds, ll, VitSequences{sod, dos, nullptr, nullptr}, nullptr,
                    want_z ? v.z : nullptr, nullptr, v.score);
  }
  HIPCK(hipGetLastError());
  if (nl) {
    const VitSequences units{sod, dol, dpad, dct};
    vit_sweep<false>(h, (unsigned)nl, (size_t)2 * KS * 8, ll, units, v.psi, nullptr, v.zlast, v.score);
    hipLaunchKernelGGL(k_vit_paths<VitSequences>, dim3((unsigned)C), dim3(KS), (size_t)Ls * KS, h->stream,
                       (const unsigned char*)v.psi, (const int32_t*)v.zlast, units, Ls, KS, K, v.path);
    hipLaunchKernelGGL(k_ffbs_compose, dim3(1), dim3(1024), 0, h->stream, (const unsigned char*)v.path, P, KS, Ls,
                       (int)C, v.mA, v.mB, v.entry);
    hipLaunchKernelGGL(k_vitseq_gather, dim3((unsigned)C), dim3(256), 0, h->stream, (const unsigned char*)v.path,
                       (const unsigned char*)v.entry, units, Ls, KS, v.z);
    HIPCK(hipGetLastError());
  }
  return 0;
}

// svihmm_ffbs_sequences: ONE forward filter over all sequences into lalpha [T][K] (h->seq_work), then S backward
// draws of every sequence.  Filter routing as estep_sequences_core: whole-chain sequences (use_chain) one after the
// other through ffbs_filter's chain route, copied to their rows; all others -- every sequence under sparse globals or
// host lliks -- in one launch of the ragged sweeps' forward direction (grid (n, 1): the kernels take the direction
// from blockIdx.y).  The emission pass over all T rows comes last, so the lliks of all rows stay readable.
// Draws: sequences below FFW_SWITCH rows in one launch, a lane per (sequence, draw) pair; longer ones through the
// blocked composition once per (sequence, draw), as launch_ffbs_windows does (ffbs_blocked_draw).
// *dz_out: int32 [S][T]; h->dec_tab: order (filter) | order (sampler).
int launch_ffbs_sequences(svihmm_ctx* h, uint32_t flags, const double* logA, int S, const double* uniforms, uint64_t seed,
                          bool want_lalpha, int32_t** dz_out, const double** dla_out) {
  const int K = h->K, N = (int)h->seq_off.size() - 1;
  const int64_t T = h->T;
  const std::vector<int64_t>& so = h->seq_off;
  const bool host_ll = flags & SVIHMM_USE_HOST_LLIKS;
  CK(wait_globals(h));
  std::vector<int32_t> ragged, chains, lanes, blocked;
  for (int s = 0; s < N; ++s) {
    const int len = (int)(so[s + 1] - so[s]);
    (!host_ll && use_chain(h, 1, len) ? chains : ragged).push_back(s);
    (len < FFW_SWITCH ? lanes : blocked).push_back(s);
  }
  const auto longer = [&so](int32_t a, int32_t b) { return so[a + 1] - so[a] > so[b + 1] - so[b]; };
  std::stable_sort(ragged.begin(), ragged.end(), longer);
  std::stable_sort(lanes.begin(), lanes.end(), longer);
  CK(ensure(h->seq_work, (size_t)T * K * sizeof(double)));
  double* la_all = (double*)h->seq_work.p;
  for (int32_t s : chains) {
    const int len = (int)(so[s + 1] - so[s]);
    const double* la = nullptr;
    CK(ffbs_filter(h, &so[s], 1, len, flags, want_lalpha, &la));
    HIPCK(hipMemcpyAsync(la_all + (size_t)so[s] * K, la, (size_t)len * K * sizeof(double), hipMemcpyDeviceToDevice,
                         h->stream));
  }
  const int64_t st0 = 0;
  CK(prepare_ll(h, &st0, 1, (int)T, flags, false, false));
  h->have_lb = false;
  h->lastB = 1; h->lastLm = (int)T;
  const size_t nr = ragged.size(), nlane = lanes.size();
  h->dec_host.resize((nr + nlane) * sizeof(int32_t));
  if (nr) std::memcpy(h->dec_host.data(), ragged.data(), nr * sizeof(int32_t));
  if (nlane) std::memcpy(h->dec_host.data() + nr * sizeof(int32_t), lanes.data(), nlane * sizeof(int32_t));
  CK(ensure(h->dec_tab, (nr + nlane) * sizeof(int32_t) + 256));
  HIPCK(hipMemcpyAsync(h->dec_tab.p, h->dec_host.data(), (nr + nlane) * sizeof(int32_t), hipMemcpyHostToDevice, h->stream));
  const int32_t* dor = (const int32_t*)h->dec_tab.p;
  const int32_t* dlanes = dor + nr;
  const int64_t* sod = (const int64_t*)h->seq_off_d.p;
  const double* ll = (const double*)h->ll.p;
  if (nr) CK(launch_seq_sweeps(h, (int)nr, 1, dor, sod, 0, ll, la_all, nullptr));
  FfbsIo io;
  CK(ffbs_io(h, logA, uniforms, (size_t)S * T, &io));
  *dz_out = io.z;
  *dla_out = la_all;
  if (nlane) {
    const unsigned nblk = (unsigned)(((int64_t)nlane * S + 63) / 64);
    ProfScope ps(h, KS_FFBS);
    if (K <= 64) {
      const int KM = K <= 16 ? 16 : K <= 32 ? 32 : 64;
      const size_t lds = ffs_lds_bytes(K, KM);
#define FSEQ(KMAX)                                                                                                 \
  hipLaunchKernelGGL(k_ffbs_seq<KMAX>, dim3(nblk), dim3(64), lds, h->stream, (const double*)la_all,                \
                     (const double*)io.logA, (const double*)io.unif, (unsigned long long)seed, sod, dlanes,     \
                     (int)nlane, S, T, K, io.z)
      if (KM == 16) FSEQ(16); else if (KM == 32) FSEQ(32); else FSEQ(64);
#undef FSEQ
    } else {
      hipLaunchKernelGGL(k_ffbs_seq_wide, dim3(nblk), dim3(64), 0, h->stream, (const double*)la_all,
                         (const double*)io.logA, (const double*)io.unif, (unsigned long long)seed, sod, dlanes,
                         (int)nlane, S, T, K, io.z);
    }
    HIPCK(hipGetLastError());
  }
  if (blocked.empty()) return 0;
  int64_t maxlen = 0;
  size_t extra = 0;
  for (int32_t s : blocked) {
    maxlen = std::max(maxlen, so[s + 1] - so[s]);
    extra = std::max(extra, ffbs_plan(h, so[s + 1] - so[s], K).extra);
  }
  FfbsBlockedScratch sc;
  CK(ffbs_blocked_scratch(h, io, maxlen, extra, &sc));
  for (int d = 0; d < S; ++d)
    for (int32_t s : blocked)
      CK(ffbs_blocked_draw(h, io, sc, seed, la_all + (size_t)so[s] * K, so[s + 1] - so[s], (int64_t)d * T + so[s]));
  HIPCK(hipGetLastError());
  return 0;
}

}  // extern "C"
