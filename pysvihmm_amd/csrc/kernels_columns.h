// kernels_columns.h -- the statistics GEMM of the column-wise families: one frame, k_stats_columns<P, MT>, with a
// policy P per family (Poisson, Gaussian tracks with missing entries; the multi-column Categorical family keeps the
// same scheme in a kernel of its own, k_stats_onehot in kernels_mcat.h, and shares COL_RB, COL_QS and ColRow).
//
//   out[f][k] = sum over the unmasked rows t of  a_f(x_t) q[t][k]     on v_mfma_f64_16x16x4_f64,
//
// obs [T][D] doubles, F = P::features(D) feature rows, each a function of ONE column's entry: the frame stages every
// entry once per row (P::Staged, P::absent() for an entry that is not present and for every entry of a masked or
// missing row) and forms the A operand on the fly from the staged value and the lane's feature descriptor.  Per-chunk
// partials [chunk][F][Kp] (the layout k_stats_cat writes), reduced in chunk order by k_finalize_cat: no atomics, a run
// is bit-reproducible.
//
// The policy, a POD passed by value as a kernel argument and defined next to its family's lookup kernel
// (PoissonStats kernels_poisson.h, PgaussStats kernels_pgauss.h), supplies what differs:
//   typedef .. Staged;  static Staged absent();           the staged entry and the value that means absent
//   typedef .. Aux;                                       element type of the family's device table (origin;
//                                                         void: none), a __restrict__ kernel argument of its own
//   int features(int D) const;                            F
//   struct Feat;  Feat feature(f, D, aux) const;          what a lane keeps of feature f: its column Feat::d and what
//                                                         operand() needs (f >= F: column 0, a feature that is 0.0)
//   Staged stage(x, d, D, aux, int* row_present) const;   entry x of column d staged; where it is present the policy
//                                                         stores 1 to *row_present, otherwise it returns absent()
//   static double operand(Staged s, const Feat& ft);      a_f of a staged entry, 0.0 for an absent one
// A workgroup always carries four state tiles (64 states): models with K < 64 run the remaining tiles on zero columns.
#pragma once

#define COL_RB 64              // rows per stage
#define COL_QS 80              // doubles per staged q row: 64 states + 16, so that rows r and r + 1 of a 32-lane
                               // group sit on the two halves of the LDS banks (stride = 32 dwords mod 64)
struct ColRow { int64_t orow, qrow; };       // orow < 0: no such row / masked

// LDS: [ q COL_RB * COL_QS doubles | row records COL_RB ColRow | row-has-a-present-entry COL_RB ints |
//        staged entries COL_RB * (D | 1) P::Staged ]   (42240 bytes + the entries: 106 KB for doubles at D = 128;
//        tu_stats.hip, launch_stats_columns, sizes it and raises the dynamic limit)
// Workgroup (blockIdx.x = row chunk, .y = group of 64 MT features, .z = group of 64 states), 4 waves; wave w owns
// the feature tiles 4 m + w (m < MT) of its group against the four state tiles.
// Operand layout of v_mfma_f64_16x16x4_f64 (MF<double> / k_stats_mfma4, svihmm_selftest_mfma): A lane l ->
// [feature l & 15][row l >> 4], B lane l -> [row l >> 4][state l & 15], C lane l register r -> [feature (l >> 4) + 4 r]
// [state l & 15].
// A row that is masked, or whose every entry is absent, contributes nothing whatever its posterior holds (the rule of
// k_stats_cat, which skips such rows): its posterior is staged as zeros, so a NaN or Inf a svihmm_suffstats caller left
// there stays out of the statistics.  A row with some entries present is a GEMM row: a non-finite posterior of such a
// row reaches, through 0.0 x NaN, every feature of its state's column in the tiles that stage it, not only the present
// ones (k_stats_cat has one column, so the case does not arise there).
template <class P, int MT>
__global__ __launch_bounds__(256) void k_stats_columns(
    const double* __restrict__ obs, const uint8_t* __restrict__ mask, const int64_t* __restrict__ starts,
    int64_t nrows, int Lm, int K, int Kp, int D, const P p, const typename P::Aux* __restrict__ aux,
    const double* __restrict__ q, int64_t rows_per_chunk, int Lq, int off, double* __restrict__ partc) {
  typedef typename P::Staged Staged;
  extern __shared__ __attribute__((aligned(16))) char col_smem[];
  double* qs = (double*)col_smem;
  ColRow* rows = (ColRow*)(qs + COL_RB * COL_QS);
  int* present = (int*)(rows + COL_RB);
  Staged* st = (Staged*)(present + COL_RB);
  const int DS = D | 1;            // (odd row stride of the staged entries)
  const int F = p.features(D);
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int kbase = 64 * blockIdx.z;
  const int fbase = 64 * MT * blockIdx.y;
  typename P::Feat ft[MT];         // this lane's feature of each tile
#pragma unroll
  for (int m = 0; m < MT; ++m) ft[m] = p.feature(fbase + 16 * (4 * m + w) + li, D, aux);
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
    // posteriors: COL_RB rows x the group's 64 states, loaded now and committed once the entries have said which
    // rows count (zeros beyond K, beyond the chunk, for masked rows and for rows without a present entry)
    const int qc = tid & 63;
    double qreg[COL_RB / 4];
#pragma unroll
    for (int i = 0; i < COL_RB / 4; ++i) {
      const ColRow rr = rows[(tid >> 6) + 4 * i];
      qreg[i] = (rr.orow >= 0 && kbase + qc < K) ? q[rr.qrow * K + kbase + qc] : 0.0;
    }
    for (int e = tid; e < COL_RB * D; e += 256) {
      const int r = e / D, d = e - r * D;
      const int64_t orow = rows[r].orow;
      Staged s = P::absent();
      if (orow >= 0) s = p.stage(obs[orow * D + d], d, D, aux, present + r);
      st[r * DS + d] = s;
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
        const double A = P::operand(st[r * DS + ft[m].d], ft[m]);
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
