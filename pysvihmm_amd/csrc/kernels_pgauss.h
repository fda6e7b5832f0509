// kernels_pgauss.h -- Gaussian tracks with missing entries (svihmm_set_emission_pgauss)
//
//   p(x_t | z_t = k) = prod_{d present} N(x_t[d] | mu_{k,d}, sigma^2_{k,d}),  a normal-inverse-gamma mean-field factor
//   (mu, nus, alphas, betas) per (k, d); obs [T][D] doubles.  The host supplies, each [K][D],
//     mu,   hprec = -0.5 alphas / betas,   cst = -0.5 / nus - 0.5 (log betas - psi(alphas)) - 0.5 log 2 pi:
//   no digamma and no log of a parameter runs on the device.
//
// Entry (t, d) is PRESENT when x > -SVIHMM_PGAUSS_ABSENT && x < SVIHMM_PGAUSS_ABSENT (1e150, compared as doubles: a
// NaN fails both, +-Inf and 1e308-style sentinels are absent).  An absent entry adds nothing to the row's llik and
// nothing to the statistics, the row's other columns are not affected.  |mu| and |origin| are below the bound (the
// host's check), so |x - mu| < 2e150 and its square is finite.
//
//   k_emission_pgauss    ll[row][k] = s, with s = +0.0 and, for the present d in ascending order,
//                          r = x - mu[k][d], p = r * r, p = p * hprec[k][d], s = s + p, s = s + cst[k][d],
//                        every operation rounded on its own (contraction is off in the kernel): bit-identical to that
//                        loop on the host.  The centred form evaluated directly: no centred resident copy is needed.
//                        A row masked under SVIHMM_MASK_AS_NAN, or without a present entry, is all +0.0.  Output in the
//                        layout / scaling convention of k_emission_cat.
//   PgaussStats          the family's policy of k_stats_columns (kernels_columns.h): [sxx | sx | n] about origin[D]
//                        as a GEMM with F = 3 D feature rows, r = x - origin[d]:
//                          out[d][k]       = sum_t (r * r) q[t][k]      (the square a rounded product of its own)
//                          out[D + d][k]   = sum_t r q[t][k]
//                          out[2 D + d][k] = sum_t 1[entry (t, d) present] q[t][k]
//                        over the unmasked rows; k_finalize_cat reduces the partials with V = 3 D.
//
// Shapes: every D <= SVIHMM_PGAUSS_MAX_D, K <= 256 runs on these two kernels.
//
// Out of scope for this family, each refused by the host: the resident SVI loop, svihmm_pred_logprob, the fp32 mode.
#pragma once

#define PG_EM_ROWS 32          // rows whose entries k_emission_pgauss stages at a time
#define PG_ABSENT 1e150        // SVIHMM_PGAUSS_ABSENT

__device__ __forceinline__ bool pg_present(double x) { return x > -PG_ABSENT && x < PG_ABSENT; }

#ifdef SVIHMM_PGAUSS_EMISSION
// lane = state (strided for K > 64); a wave owns every fourth row of the staged block.
// Tables: mh [D + 1][K] pairs (mu, hprec), one aligned 16-byte read, followed by cst [D + 1][K]; row D of both is all
// +0.0.  (Three doubles per (column, state): K = 64, D = 32 is 50 KB and stays in LDS, which a padded 32-byte record
// would not.)
// An absent column (staged as NaN: absent, or the row is masked) is walked as x = +0.0 against row D:
//   r = 0.0 - 0.0 = +0.0, p = r * r = +0.0, p = p * (+0.0) = +0.0, s = s + (+0.0), s = s + (+0.0),
// and x + (+0.0) == x, to the bit, for every x but -0.0.  s is never -0.0: it starts at +0.0; a present column's p is
// (r * r >= +0.0) times (hprec <= 0, the host's check), so -0.0, negative or (hprec = +0.0) +0.0; a round-to-nearest
// sum is -0.0 only if both operands are, so s + p is not -0.0 as long as s is not, and then neither is (s + p) + cst.
// So walking the zero row gives the bits of the loop that skips, without a select on the vector side: the row's value
// is one for the wave, so the table row and the value are chosen on the scalar side.
// TLDS: the tables sit in LDS (the host picks it when 3 (D + 1) K doubles fit 64 KB), otherwise they are read through L2.
// LDS: [ mh (D+1)*K double2 | cst (D+1)*K doubles (both TLDS) | x PG_EM_ROWS * DP doubles ],  DP = (D + 3) & ~3
template <bool TLDS>
__global__ __launch_bounds__(256) void k_emission_pgauss(
    const double* __restrict__ obs, const uint8_t* __restrict__ mask, const int64_t* __restrict__ starts,
    int64_t nrows, int Lm, int K, int D, const double2* __restrict__ table, uint32_t flags,
    double* __restrict__ ll, int rows_per_wg) {
#pragma clang fp contract(off)
  extern __shared__ __attribute__((aligned(16))) char pg_smem[];
  const int NT = (D + 1) * K;
  double2* tab = (double2*)pg_smem;
  double* tabc = (double*)(tab + NT);
  double* xs = (double*)(pg_smem + (TLDS ? (size_t)NT * 3 * sizeof(double) : 0));
  const double* __restrict__ gcst = (const double*)(table + NT);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (TLDS)
    for (int e = tid; e < NT; e += 256) { tab[e] = table[e]; tabc[e] = gcst[e]; }
  const double2* __restrict__ MH = TLDS ? (const double2*)tab : table;
  const double* __restrict__ CS = TLDS ? (const double*)tabc : gcst;
  const bool use_mask = (flags & SVIHMM_MASK_AS_NAN) && mask;
  const int DP = (D + 3) & ~3;       // a row's entries padded with "absent" to whole groups of four
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_wg;
  const int64_t r1 = imin64(nrows, r0 + rows_per_wg);
  for (int64_t base = r0; base < r1; base += PG_EM_ROWS) {
    __syncthreads();       // (the previous block's entries are consumed; first trip: the tables are staged)
    const int nr = (int)imin64(PG_EM_ROWS, r1 - base);
    for (int e = tid; e < nr * DP; e += 256) {
      const int r = e / DP, d = e - r * DP;
      double v = NAN;
      if (d < D) {
        const int64_t orow = obs_row(starts, Lm, base + r);
        const double x = obs[orow * D + d];
        if (pg_present(x) && !(use_mask && mask[orow])) v = x;
      }
      xs[r * DP + d] = v;
    }
    __syncthreads();
    for (int r = w; r < nr; r += 4) {
      const double* __restrict__ xr = xs + r * DP;
      for (int k = lane; k < K; k += 64) {
        double s = 0.0;
        for (int d0 = 0; d0 < DP; d0 += 4) {
          double p[4], c[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const double xv = wave_uniform(xr[d0 + j]);     // the row's entry: one value for the wave
            const bool absent = xv != xv;
            const size_t ti = (size_t)(absent ? D : d0 + j) * K + k;
            const double2 v = MH[ti];
            const double rr = (absent ? 0.0 : xv) - v.x;
            double t = rr * rr;
            t = t * v.y;
            p[j] = t;
            c[j] = CS[ti];
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            s = s + p[j];
            s = s + c[j];
          }
        }
        ll[(base + r) * K + k] = s;
      }
    }
  }
}
#endif  // SVIHMM_PGAUSS_EMISSION

#ifdef SVIHMM_PGAUSS_STATS
// The policy of k_stats_columns (kernels_columns.h, included before this file).  Staged per row and column:
// r = x - origin[d] as fp64, NaN for absent.  A operand of feature f for a staged r: r * r (f < D), r (D <= f < 2 D),
// 1.0 (2 D <= f < 3 D), each 0.0 where r is NaN.  Contraction is off where the policy computes: the difference and the
// square are rounded operations of their own.
struct PgaussStats {
  typedef double Staged;
  typedef double Aux;              // origin
  struct Feat { int d, third; };   // column and third (0 r * r, 1 r, 2 one, 3 none)
  static __device__ Staged absent() { return NAN; }
  __device__ int features(int D) const { return 3 * D; }
  __device__ Feat feature(int f, int D, const double*) const {
    const int third = f < D ? 0 : f < 2 * D ? 1 : f < 3 * D ? 2 : 3;
    return Feat{third < 3 ? f - third * D : 0, third};
  }
  __device__ Staged stage(double x, int d, int, const double* __restrict__ origin, int* row_present) const {
#pragma clang fp contract(off)
    if (!pg_present(x)) return NAN;
    *row_present = 1;                    // (every writer stores the same value)
    return x - origin[d];
  }
  static __device__ double operand(Staged v, const Feat& ft) {
#pragma clang fp contract(off)
    const double sq = v * v;
    const double a = ft.third == 0 ? sq : ft.third == 1 ? v : 1.0;
    return (v != v || ft.third == 3) ? 0.0 : a;
  }
};
#endif  // SVIHMM_PGAUSS_STATS
