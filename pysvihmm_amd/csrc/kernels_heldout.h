// kernels_heldout.h -- held-out log-probability against the posterior rows an E-step left in HBM
// (svihmm_heldout_rows / svihmm_heldout_entries).  Part of libsvihmm_hip.so; compiled in svihmm_hip.hip after
// kernels_misc.h (k_pred_final adds the workgroups' partials in workgroup order for both kernels here).
//
//   lp = LSE_k( log(q[g][k] + 1e-9) + term_k )            (hmmbase.py:322-340)
//
//   k_heldout_rows      term_k = ll[g][k], the family's llik of batch row g on its TRUE values (launch_emission with the
//                       masking flag off, into the side buffer), for the batch rows whose resident row is masked.
//                       k_pred_logprob's row kernel with the row map made general: starts != nullptr: batch row g is
//                       resident row starts[g / Lm] + g % Lm (a window batch); starts == nullptr: the identity
//                       (svihmm_estep_sequences, and the gathered copy of svihmm_estep_sequence_subset, whose own mask
//                       bytes come in as `mask`).
//   k_heldout_entries   one entry (g, d, x) of a product family per 16-lane row:
//                         multi-column Categorical  term_k = table[off_d + (int)x][k]                 (table [F][K])
//                         Poisson                   t = (double)c * elog[k][d]  (one rounded multiply: contraction is off),
//                                                   t = t - erate[k][d],  t = t - logfact[c],  c = (int)x
//                                                   (table [D + 1][K] pairs (elog, erate))
//                         Gaussian tracks           t = x - mu[k][d], t = t * t, t = t * hprec[k][d], t = t + cst[k][d],
//                                                   each rounded on its own (table [D + 1][K] pairs (mu, hprec), then
//                                                   [D + 1][K] cst: kernels_pgauss.h)
//                       Both tables are the transposed copies the emission kernels read (a feature's / a column's states
//                       are contiguous; k_mcat_table / k_pois_table rebuild exactly these in the SVI loop), so the
//                       table read of the 16 lanes is as coalesced as the q row read: 128 contiguous bytes of q and 128
//                       (mcat) or 256 (Poisson) of the table per 16 states.  row / col / val / logfact[c] are one
//                       address for the 16 lanes (a broadcast load), the PRESENT test is uniform within them.
//                       PRESENT is the families' own rule (kernels_mcat.h, kernels_poisson.h); for the symbol columns it
//                       is written as x == x && x > -1.0 && x < V[d], which is 0 <= (int)x < V[d] for every double whose
//                       conversion is defined and false for the others.
//
// Reduction as in k_pred_logprob: entry / row e belongs to workgroup e / HELDOUT_PER_BLOCK and inside it to 16-lane row
// (e % HELDOUT_PER_BLOCK) % 16 (fixed), LSE over the states with row16_max / row16_sum (DPP, no LDS), {sum, count}
// of the 16 rows through 2 x 16 doubles of LDS in row order, one partial pair per workgroup, k_pred_final over the
// pairs in workgroup order.  No atomics: a run is bit-reproducible.  out_lp takes plain vector stores from lane 0.
#pragma once

#define HELDOUT_PER_BLOCK 2048

// {sum, count} of the workgroup's 16 rows -> part[2 b], part[2 b + 1]
__device__ __forceinline__ void heldout_block_partial(double acc, double cnt, double (*red)[16], double* __restrict__ part) {
  const int li = threadIdx.x & 15, rg = threadIdx.x >> 4;
  if (li == 0) { red[0][rg] = acc; red[1][rg] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    double a = 0.0, c = 0.0;
    for (int i = 0; i < 16; ++i) { a += red[0][i]; c += red[1][i]; }
    part[2 * blockIdx.x] = a;
    part[2 * blockIdx.x + 1] = c;
  }
}

template <int KT>
__global__ __launch_bounds__(256) void k_heldout_rows(
    const double* __restrict__ q, const double* __restrict__ ll, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ starts, int64_t nrows, int Lm, int K, double* __restrict__ out_lp,
    double* __restrict__ part) {
  __shared__ double red[2][16];
  const int li = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int64_t r0 = (int64_t)blockIdx.x * HELDOUT_PER_BLOCK;
  const int64_t r1 = imin64(nrows, r0 + HELDOUT_PER_BLOCK);
  double acc = 0.0, cnt = 0.0;
  for (int64_t g = r0 + rg; g < r1; g += 16) {
    int64_t orow = g;
    if (starts) {
      const int64_t b = g / Lm;
      orow = starts[b] + (g - b * Lm);
    }
    if (!mask[orow]) {                     // uniform within the 16-lane row
      if (out_lp && li == 0) out_lp[g] = NAN;
      continue;
    }
    double v[KT], mx = -INFINITY;
#pragma unroll
    for (int c = 0; c < KT; ++c) {
      const int k = li + 16 * c;
      v[c] = k < K ? log(q[g * K + k] + 1e-9) + ll[g * K + k] : -INFINITY;
      mx = fmax(mx, v[c]);
    }
    mx = row16_max(mx);
    double sm = 0.0;
#pragma unroll
    for (int c = 0; c < KT; ++c) sm += (li + 16 * c < K) ? exp(v[c] - mx) : 0.0;
    sm = row16_sum(sm);
    const double lp = mx + log(sm);
    if (out_lp && li == 0) out_lp[g] = lp;
    acc += lp;
    cnt += 1.0;
  }
  heldout_block_partial(acc, cnt, red, part);
}

// FAM 1 (Poisson): table = [D + 1][K] pairs (elog, erate) read as double2, logfact [C + 1]; FAM 2 (Gaussian tracks):
// table = [D + 1][K] pairs (mu, hprec) read as double2, then [D + 1][K] cst; FAM 0: table = [F][K] doubles and
// meta = [off_d D | V_d D | ...] (svihmm_ctx::mcat_meta).  row[e] in [0, nrows) and col[e] in [0, D) are the host's check.
template <int KT, int FAM>
__global__ __launch_bounds__(256) void k_heldout_entries(
    const double* __restrict__ q, const int64_t* __restrict__ row, const int32_t* __restrict__ col,
    const double* __restrict__ val, int64_t n, int K, int D, const double* __restrict__ table,
    const int* __restrict__ meta, const double* __restrict__ logfact, int C, double* __restrict__ out_lp,
    double* __restrict__ part) {
#pragma clang fp contract(off)
  __shared__ double red[2][16];
  const int li = threadIdx.x & 15, rg = threadIdx.x >> 4;
  const int64_t e0 = (int64_t)blockIdx.x * HELDOUT_PER_BLOCK;
  const int64_t e1 = imin64(n, e0 + HELDOUT_PER_BLOCK);
  double acc = 0.0, cnt = 0.0;
  for (int64_t e = e0 + rg; e < e1; e += 16) {
    const double x = val[e];
    const int d = col[e];
    const int64_t g = row[e];
    constexpr bool POIS = FAM == 1, PG = FAM == 2;
    const double lim = PG ? 1e150 : POIS ? (double)(C + 1) : (double)meta[D + d];
    const bool present = PG ? (x > -lim && x < lim) : POIS ? (x >= 0.0 && x < lim) : (x == x && x > -1.0 && x < lim);
    if (!present) {                        // uniform within the 16-lane row
      if (out_lp && li == 0) out_lp[e] = NAN;
      continue;
    }
    const int c = PG ? 0 : (int)x;
    const double cd = (double)c;
    const double lf = POIS ? logfact[c] : 0.0;
    const size_t trow = (POIS || PG) ? (size_t)d * K : (size_t)(meta[d] + c) * K;
    double v[KT], mx = -INFINITY;
#pragma unroll
    for (int j = 0; j < KT; ++j) {
      const int k = li + 16 * j;
      double vv = -INFINITY;
      if (k < K) {
        double t;
        if (PG) {
          const double2 mh = ((const double2*)table)[trow + k];
          t = x - mh.x;
          t = t * t;
          t = t * mh.y;
          t = t + (table + 2 * (size_t)(D + 1) * K)[trow + k];
        } else if (POIS) {
          const double2 er = ((const double2*)table)[trow + k];
          t = cd * er.x;
          t = t - er.y;
          t = t - lf;
        } else {
          t = table[trow + k];
        }
        vv = log(q[g * K + k] + 1e-9) + t;
      }
      v[j] = vv;
      mx = fmax(mx, vv);
    }
    mx = row16_max(mx);
    double sm = 0.0;
#pragma unroll
    for (int j = 0; j < KT; ++j) sm += (li + 16 * j < K) ? exp(v[j] - mx) : 0.0;
    sm = row16_sum(sm);
    const double lp = mx + log(sm);
    if (out_lp && li == 0) out_lp[e] = lp;
    acc += lp;
    cnt += 1.0;
  }
  heldout_block_partial(acc, cnt, red, part);
}
