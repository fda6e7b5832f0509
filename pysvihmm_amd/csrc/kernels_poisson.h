// kernels_poisson.h -- Poisson count emissions (svihmm_set_emission_poisson)
//
//   p(x_t | z_t = k) = prod_d Poisson(x_t[d] | lambda_{k,d}),   q(lambda_{k,d}) = Gamma(a_{k,d}, b_{k,d}),
//   obs [T][D] counts stored as doubles; the host supplies elog = psi(a) - log b, erate = a / b and
//   logfact[c] = lgamma(c + 1) for c = 0..C.
//
// Entry (t, d) is PRESENT when x >= 0.0 && x < (double)(C + 1), compared as doubles (a NaN fails both); its count is
// c = (int)x.  An absent entry adds nothing to the row's llik and nothing to the statistics, the row's other columns
// are not affected.
//
//   k_emission_poisson   ll[row][k] = s - g, with s = g = +0.0 and, for the present d in ascending order,
//                          p = (double)c_d * elog[k][d] (one rounded multiply), s = s + p, s = s - erate[k][d],
//                          g = g + logfact[c_d]:
//                        contraction is off in the kernel, so the result is bit-identical to that loop on the host.
//                        g is formed once per row.  A row masked under SVIHMM_MASK_AS_NAN, or without a present
//                        entry, is all +0.0.  Output in the layout / scaling convention of k_emission_cat.
//   PoissonStats         the family's policy of k_stats_columns (kernels_columns.h): [sx | n] as a GEMM with F = 2 D
//                        feature rows,
//                          out[f][k]     = sum_t c_tf q[t][k]                     (f < D)
//                          out[D + d][k] = sum_t 1[entry (t, d) present] q[t][k]
//                        over the unmasked rows.  A operand formed on the fly from 32-bit staged counts (-1: absent or
//                        masked row); k_finalize_cat reduces the partials with V = 2 D.
//
// Shapes: every D <= SVIHMM_POISSON_MAX_D, C <= SVIHMM_POISSON_MAX_COUNT, K <= 256 runs on these two kernels.
//
// The resident SVI loop takes the family as its family 4 (svihmm_svi_begin_poisson; kernels_svi.h: k_pois_table
// rebuilds the pairs these kernels read, svi_pois_step blends the Gamma factors), and hmmsgd_metaobs.VBHMM runs on it.
// Out of scope for this family, as for the multi-column Categorical one: svihmm_pred_logprob and the fp32 mode.
#pragma once

#define PO_EM_ROWS 32          // rows whose counts k_emission_poisson stages at a time

#ifdef SVIHMM_POISSON_EMISSION
// lane = state (strided for K > 64); a wave owns every fourth row of the staged block.
// tab: [D + 1][K] pairs (elog, erate), so one 16-byte read serves a column's multiply-add-subtract; row D is all +0.0.
// An absent column is walked as count 0 against row D: p = 0.0 * 0.0 = +0.0 and the subtrahend is +0.0, which leave
// every value s can hold unchanged (see the note at the g pass) -- the bits of the loop that skips, without a select
// on the vector side (the count is one value for the wave, so the row and the count are chosen on the scalar side).
// TLDS: the pairs sit in LDS (the host picks it when 2 D K doubles fit 64 KB), otherwise they are read through L2.
// LDS: [ pairs (D+1)*K double2 (TLDS) | g PO_EM_ROWS doubles | counts PO_EM_ROWS * CS ints ],  CS = ((D + 3) & ~3) + 4
template <bool TLDS>
__global__ __launch_bounds__(256) void k_emission_poisson(
    const double* __restrict__ obs, const uint8_t* __restrict__ mask, const int64_t* __restrict__ starts,
    int64_t nrows, int Lm, int K, int D, int C, const double2* __restrict__ table,
    const double* __restrict__ logfact, uint32_t flags, double* __restrict__ ll, int rows_per_wg) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char po_smem[];
  double2* tab = (double2*)po_smem;
  double* gs = (double*)(po_smem + (TLDS ? (size_t)(D + 1) * K * sizeof(double2) : 0));
  int* cnt = (int*)(gs + PO_EM_ROWS);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (TLDS)
    for (int e = tid; e < (D + 1) * K; e += 256) tab[e] = table[e];
  const double2* __restrict__ T = TLDS ? (const double2*)tab : table;
  const bool use_mask = (flags & SVIHMM_MASK_AS_NAN) && mask;
  const int DP = (D + 3) & ~3;       // a row's counts padded with "absent" to whole groups of four
  const int CS = DP + 4;             // (rows stay 16-byte aligned: four counts come in one read)
  const double lim = (double)(C + 1);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = imin64(nrows, r0 + rows_per_wg);
  for (int64_t base = r0; base < r1; base += PO_EM_ROWS) {
    __syncthreads();       // (the previous block's counts are consumed; first trip: the table is staged)
    const int nr = (int)imin64(PO_EM_ROWS, r1 - base);
    for (int e = tid; e < nr * DP; e += 256) {
      const int r = e / DP, d = e - r * DP;
      int c = -1;
      if (d < D) {
        const int64_t orow = obs_row(starts, Lm, base + r);
        const double x = obs[orow * D + d];
        if (x >= 0.0 && x < lim && !(use_mask && mask[orow])) c = (int)x;
      }
      cnt[r * CS + d] = c;
    }
    __syncthreads();
    // g of each row, once: the logfact reads of four columns overlap, the adds stay in ascending d.  An absent column
    // adds +0.0, which leaves every value g (and s below) can hold unchanged: both start at +0.0, and in
    // round-to-nearest a sum or difference is -0.0 only when the running value already is.
    if (tid < nr) {
      const int* __restrict__ cr = cnt + tid * CS;
      double g = 0.0;
      for (int d0 = 0; d0 < DP; d0 += 4) {
        double t[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int c = cr[d0 + j];
          const double v = logfact[c < 0 ? 0 : c];
          t[j] = c < 0 ? 0.0 : v;
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) g = g + t[j];
      }
      gs[tid] = g;
    }
    __syncthreads();
    for (int r = w; r < nr; r += 4) {
      const int* __restrict__ cr = cnt + r * CS;
      const double g = gs[r];
      for (int k = lane; k < K; k += 64) {
        double s = 0.0;
        for (int d0 = 0; d0 < DP; d0 += 4) {
          double p[4], e[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int c = __builtin_amdgcn_readfirstlane(cr[d0 + j]);     // the row's entry: one value for the wave
            const double2 v = T[(size_t)(c < 0 ? D : d0 + j) * K + k];
            p[j] = (double)(c < 0 ? 0 : c) * v.x;
            e[j] = v.y;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s = s + p[j];
            s = s - e[j];
          }
        }
        ll[(base + r) * K + k] = s - g;
      }
    }
  }
}
#endif  // SVIHMM_POISSON_EMISSION

#ifdef SVIHMM_POISSON_STATS
// The policy of k_stats_columns (kernels_columns.h, included before this file): 32-bit staged counts, -1 for absent.
// A operand of feature f for a staged count c: (double)c for f < D, 1.0 for D <= f < 2 D, either 0.0 when c is absent.
struct PoissonStats {
  double lim;                      // (double)(C + 1)
  typedef int Staged;
  typedef void Aux;
  struct Feat { int d; bool issx; double one; };      // column, and what a present entry contributes (the count, or one)
  static __device__ Staged absent() { return -1; }
  __device__ int features(int D) const { return 2 * D; }
  __device__ Feat feature(int f, int D, const void*) const {
    return Feat{f < D ? f : f < 2 * D ? f - D : 0, f < D, (f >= D && f < 2 * D) ? 1.0 : 0.0};
  }
  __device__ Staged stage(double x, int, int, const void*, int* row_present) const {
    const int c = (x >= 0.0 && x < lim) ? (int)x : -1;
    if (c >= 0) *row_present = 1;        // (every writer stores the same value)
    return c;
  }
  static __device__ double operand(Staged c, const Feat& ft) { return c < 0 ? 0.0 : ft.issx ? (double)c : ft.one; }
};
#endif  // SVIHMM_POISSON_STATS
