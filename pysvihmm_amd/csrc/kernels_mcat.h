// kernels_mcat.h -- multi-column Categorical emissions (svihmm_set_emission_mcat)
//
//   p(x_t | z_t = k) = prod_d Cat(x_t[d] | theta_{k,d}),   obs [T][D] symbol indices stored as doubles,
//   V[d] symbols in column d, F = sum_d V[d] features, feature f = off_d + v  <->  (d(f), v(f)).
//
// Entry (t, d) is PRESENT when it is not NaN and 0 <= (int)x < V[d]; an absent entry adds nothing to the row's
// llik and nothing to the counts, the row's other columns are not affected.
//
//   k_emission_mcat   ll[row][k] = sum over present d, ascending, of table[off_d + x_d][k]   (table [F][K],
//                     transposed as k_emission_cat keeps it): s starts at +0.0 and takes one plain add per present
//                     column, so the result is bit-identical to the same loop on the host.  A row masked under
//                     SVIHMM_MASK_AS_NAN is all zeros.  Output in the layout / scaling convention of k_emission_cat
//                     (unscaled lliks: the k_scale_ll pass and the sweeps follow unchanged).
//   k_stats_onehot    the counts as a GEMM, the scheme of k_stats_columns (kernels_columns.h) in a kernel of its own:
//                       out[f][k] = sum_t 1[x_t,d(f) = v(f) and row t unmasked] q[t][k]
//                     A operand formed on the fly from 16-bit staged symbols (-1: absent or masked row): every
//                     product is 1.0 q or 0.0 q, exact, so the only rounding is the fp64 accumulation.
//
// Shapes: every F <= SVIHMM_MCAT_MAX_F, D <= SVIHMM_MCAT_MAX_D, K <= 256 runs on these two kernels (no fallback
// kernel).
//
// The resident SVI loop takes the family as its family 3 (svihmm_svi_begin_mcat; kernels_svi.h: k_mcat_table rebuilds
// the table these kernels read, the step and the ELBO term are the Categorical family's, column by column), and
// hmmsgd_metaobs.VBHMM runs on it.
// Out of scope for this family: svihmm_pred_logprob (NIW only: refuses with a message) and the fp32 mode (the family
// rides the Categorical branches, which never enter it: last_batch_f32 stays 0).
#pragma once

// meta (int32, device): [ off_d  D | V_d  D | d(f)  F | v(f)  F ]
#define MC_EM_ROWS 32          // rows whose symbols k_emission_mcat stages at a time

// (tu_emission.hip takes the lookup, tu_stats.hip -- after kernels_stats.h and kernels_columns.h -- the GEMM)
#ifdef SVIHMM_MCAT_EMISSION
// lane = state (strided for K > 64); a wave owns every fourth row of the staged block.
// TLDS: the table sits in LDS (the host picks it when F K doubles fit 64 KB), otherwise it is read through L2.
// LDS: [ table F*K doubles (TLDS) | feature index MC_EM_ROWS * ((D + 7) & ~7) ints ]
template <bool TLDS>
__global__ __launch_bounds__(256) void k_emission_mcat(
    const double* __restrict__ obs, const uint8_t* __restrict__ mask, const int64_t* __restrict__ starts,
    int64_t nrows, int Lm, int K, int D, int F, const int* __restrict__ meta, const double* __restrict__ table,
    uint32_t flags, double* __restrict__ ll, int rows_per_wg) {
  extern __shared__ __attribute__((aligned(16))) char mc_smem[];
  double* tab = (double*)mc_smem;
  int* sidx = (int*)(mc_smem + (TLDS ? (size_t)F * K * sizeof(double) : 0));
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (TLDS)
    for (int e = tid; e < F * K; e += 256) tab[e] = table[e];
  const double* __restrict__ T = TLDS ? (const double*)tab : table;
  const int* __restrict__ voff = meta;
  const int* __restrict__ vnum = meta + D;
  const bool use_mask = (flags & SVIHMM_MASK_AS_NAN) && mask;
  const int DP = (D + 7) & ~7;       // a row's indices padded with "absent" to whole groups of eight
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = imin64(nrows, r0 + rows_per_wg);
  for (int64_t base = r0; base < r1; base += MC_EM_ROWS) {
    __syncthreads();       // (the previous block's indices are consumed; first trip: the table is staged)
    const int nr = (int)imin64(MC_EM_ROWS, r1 - base);
    for (int e = tid; e < nr * DP; e += 256) {
      const int r = e / DP, d = e - r * DP;
      int f = -1;
      if (d < D) {
        const int64_t orow = obs_row(starts, Lm, base + r);
        const double x = obs[orow * D + d];
        const bool bad = (x != x) || (use_mask && mask[orow]);
        const int v = bad ? -1 : (int)x;
        if (v >= 0 && v < vnum[d]) f = voff[d] + v;
      }
      sidx[e] = f;
    }
    __syncthreads();
    for (int r = w; r < nr; r += 4) {
      const int* __restrict__ sr = sidx + r * DP;
      for (int k = lane; k < K; k += 64) {
        // eight columns at a time: their index and table reads are independent and overlap, the adds stay in
        // ascending d.  An absent column adds +0.0, which leaves every s this loop can hold unchanged (s starts
        // at +0.0 and a sum of finite terms in round-to-nearest is never -0.0): the bits of the skipping loop.
        double s = 0.0;
        for (int d0 = 0; d0 < DP; d0 += 8) {
          double t[8];
#pragma unroll
          for (int j = 0; j < 8; ++j) {
            const int f = __builtin_amdgcn_readfirstlane(sr[d0 + j]);     // the row's entry: one value for the wave
            const double v = T[(size_t)(f < 0 ? 0 : f) * K + k];
            t[j] = f < 0 ? 0.0 : v;
          }
#pragma unroll
          for (int j = 0; j < 8; ++j) s += t[j];
        }
        ll[(base + r) * K + k] = s;
      }
    }
  }
}
#endif  // SVIHMM_MCAT_EMISSION

#ifdef SVIHMM_MCAT_STATS
// k_stats_columns's scheme, operand layout, row records and posterior staging (kernels_columns.h, included before this
// file: COL_RB, COL_QS, ColRow) in a kernel of its own: as a policy of the frame this family's statistics slot measured
// about 1 % above this kernel's, more than the run-to-run spread, in three samples, so it stays on the code it had.
// A masked row, or one without a present entry, is staged with zero posteriors (the frame's rule).
// LDS: [ q COL_RB * COL_QS doubles | row records COL_RB ColRow | row-has-a-present-entry COL_RB ints | symbols COL_RB * DS int16 ]
template <int MT>
__global__ __launch_bounds__(256) void k_stats_onehot(
    const double* __restrict__ obs, const uint8_t* __restrict__ mask, const int64_t* __restrict__ starts,
    int64_t nrows, int Lm, int K, int Kp, int D, int F, const int* __restrict__ meta,
    const double* __restrict__ q, int64_t rows_per_chunk, int Lq, int off, double* __restrict__ partc) {
  extern __shared__ __attribute__((aligned(16))) char mc_smem[];
  double* qs = (double*)mc_smem;
  ColRow* rows = (ColRow*)(mc_smem + (size_t)COL_RB * COL_QS * sizeof(double));
  int* present = (int*)(mc_smem + (size_t)COL_RB * COL_QS * sizeof(double) + COL_RB * sizeof(ColRow));
  short* sym = (short*)(mc_smem + (size_t)COL_RB * COL_QS * sizeof(double) + COL_RB * sizeof(ColRow) + COL_RB * sizeof(int));
  const int DS = D | 1;            // (odd row stride of the 16-bit symbols)
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int* __restrict__ vnum = meta + D;
  const int* __restrict__ fd = meta + 2 * D;
  const int* __restrict__ fv = fd + F;
  const int kbase = 64 * blockIdx.z;
  const int fbase = 64 * MT * blockIdx.y;
  // this lane's feature of each tile: column and symbol (no such feature: a symbol no staged value equals)
  int myd[MT], myv[MT];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    const int f = fbase + 16 * (4 * m + w) + li;
    myd[m] = f < F ? fd[f] : 0;
    myv[m] = f < F ? fv[f] : -2;
  }
  typedef MF<double>::v4 v4;
  v4 acc[MT][4];
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n) acc[m][n] = v4{0.0, 0.0, 0.0, 0.0};
  const int64_t c0 = (int64_t)blockIdx.x * rows_per_chunk;
  const int64_t c1 = imin64(nrows, c0 + rows_per_chunk);
  for (int64_t s0 = c0; s0 < c1; s0 += COL_RB) {
    __syncthreads();                 // (the previous stage is consumed)
    if (tid < COL_RB) {
      const int64_t g = s0 + tid;
      ColRow rr = {-1, -1};
      if (g < c1) {
        const int64_t bw = g / Lm;
        const int64_t t = g - bw * Lm;
        const int64_t orow = starts[bw] + off + t;
        rr.qrow = bw * Lq + off + t;
        rr.orow = (mask && mask[orow]) ? -1 : orow;
      }
      rows[tid] = rr;
      present[tid] = 0;
    }
    __syncthreads();
    // posteriors: COL_RB rows x the group's 64 states, loaded now and committed once the symbols have said which
    // rows count (zeros beyond K, beyond the chunk, for masked rows and for rows without a present entry)
    const int qc = tid & 63;
    double qreg[COL_RB / 4];
#pragma unroll
    for (int i = 0; i < COL_RB / 4; ++i) {
      const ColRow rr = rows[(tid >> 6) + 4 * i];
      qreg[i] = (rr.orow >= 0 && kbase + qc < K) ? q[rr.qrow * K + kbase + qc] : 0.0;
    }
    // symbols: 16-bit, -1 for an absent entry and for every entry of a masked / missing row
    for (int e = tid; e < COL_RB * D; e += 256) {
      const int r = e / D, d = e - r * D;
      const int64_t orow = rows[r].orow;
      int v = -1;
      if (orow >= 0) {
        const double x = obs[orow * D + d];
        const int xi = (x != x) ? -1 : (int)x;
        if (xi >= 0 && xi < vnum[d]) v = xi;
      }
      sym[r * DS + d] = (short)v;
      if (v >= 0) present[r] = 1;        // (every writer stores the same value)
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < COL_RB / 4; ++i) {
      const int r = (tid >> 6) + 4 * i;
      qs[r * COL_QS + qc] = present[r] ? qreg[i] : 0.0;
    }
    __syncthreads();
#pragma unroll 2
    for (int ks = 0; ks < COL_RB / 4; ++ks) {
      const int r = 4 * ks + lg;
      double Bv[4];
#pragma unroll
      for (int n = 0; n < 4; ++n) Bv[n] = qs[r * COL_QS + 16 * n + li];
#pragma unroll
      for (int m = 0; m < MT; ++m) {
        const double A = ((int)sym[r * DS + myd[m]] == myv[m]) ? 1.0 : 0.0;
#pragma unroll
        for (int n = 0; n < 4; ++n) acc[m][n] = MF<double>::mma(A, Bv[n], acc[m][n]);
      }
    }
  }
  double* __restrict__ out = partc + (size_t)blockIdx.x * F * Kp;
#pragma unroll
  for (int m = 0; m < MT; ++m)
#pragma unroll
    for (int n = 0; n < 4; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int f = fbase + 16 * (4 * m + w) + MF<double>::crow(lg, r);
        const int k = kbase + 16 * n + li;
        if (f < F && k < Kp) out[(size_t)f * Kp + k] = acc[m][n][r];
      }
}
#endif  // SVIHMM_MCAT_STATS
