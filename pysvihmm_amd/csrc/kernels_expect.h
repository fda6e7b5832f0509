// kernels_expect.h -- posterior expectations of per-state tables against the posterior rows an E-step left in HBM
// (svihmm_posterior_expect / svihmm_posterior_expect_entries).  Part of libsvihmm_hip.so; compiled in svihmm_hip.hip.
//
//   k_posterior_expect          out[g][f] = sum_k q[g][k] table[k][f]  for every batch row g: a [rows x K] . [K x F]
//                               fp64 GEMM on v_mfma_f64_16x16x4_f64, the posterior rows the A operand, the table the
//                               B operand.
//   k_posterior_expect_entries  out[e] = sum_k q[row[e]][k] table[k][col[e]], one entry per thread, k ascending, each
//                               product and each sum rounded on its own (contraction off): a NumPy loop restates it
//                               bit for bit.
//
// The dense kernel is a stream: it reads rows * K * 8 bytes once per feature group and writes rows * F * 8 bytes; at
// 2 K F flops per row the matrix pipe idles (DESIGN.md has the arithmetic).  What it is built around:
//
//   * Workgroup (blockIdx.x, blockIdx.y), 4 waves.  blockIdx.y owns the feature group [16 NT y, 16 NT (y + 1)); its
//     slice of the table is staged ONCE, whole, [Kpad][16 NT + 2] doubles of LDS (Kpad = K rounded up to EXPECT_KC;
//     states >= K and features >= F are zeros written by the staging loop, no global load stands behind them).  The
//     row stride 16 NT + 2 puts the 16-lane groups lg and lg + 1 of a B read, which are 8 table rows apart, on the two
//     halves of the banks.  Then no barrier: wave w of workgroup x walks the 32-row tiles 4 x + w, + 4 gridDim.x, ...
//     so the grid is sized to the device (a few workgroups per CU), not to the rows, and the staging is paid once per
//     workgroup, not once per tile.
//   * A operand: in a k-chunk of EXPECT_KC = 32 states lane (i = l & 15, lg = l >> 4) loads the 8 CONSECUTIVE doubles
//     q[row i][32 c + 8 lg .. + 7] -- 64 bytes per lane, 256 contiguous bytes per row from its four lanes -- and MFMA
//     step s of the chunk takes element s of every lane: it contracts the states 32 c + 8 lg + s, lg = 0 .. 3.  The B
//     read of step s follows that map.  So the order in which an output's K products are added is a property of the
//     kernel (chunk c ascending, step s ascending, the MFMA's four states), the same for every row, tile and grid:
//     two runs, and the same row met in two batches, give the same bits.  No atomics.
//     VEC doubles per load instruction: 4 where K % 4 == 0 (the lane's span is 32-byte aligned), 2 where K is even,
//     else 1; a span that starts at or past K, and every span of a row >= nrows, is zeros without a load.
//   * Two 16-row MFMA tiles per wave against one B read (32 rows per wave tile): half the LDS traffic per byte of q.
//   * The next chunk's loads (of the same tile, or chunk 0 of the wave's next tile) are issued before the current
//     chunk's MFMAs: 2 x 64 bytes per lane in flight per wave across the whole walk, tile boundaries included.
//   * C lane l register r is out[row (l >> 4) + 4 r][feature l & 15]: a store instruction writes, per register, 16
//     consecutive doubles of four rows -- full 128-byte row segments straight from the accumulators, no LDS round
//     trip.  Rows >= nrows and features >= F are masked at the store.
#pragma once

#define EXPECT_KC 32           // states per k-chunk: 8 consecutive doubles per lane, 8 MFMA steps
#define EXPECT_ROWS 32         // rows per wave tile: two MFMA row tiles
#define EXPECT_LD_PAD 2        // doubles added to the staged table's row stride

typedef double ex_v4 __attribute__((ext_vector_type(4)));

// the lane's 8 doubles of chunk c of both row tiles of wave tile `tile` (zeros outside the rows and the states)
template <int VEC>
__device__ __forceinline__ void expect_load_chunk(double (&a)[2][8], const double* __restrict__ q, int64_t nrows, int K,
                                                  int64_t tile, int c, int li, int lg) {
  typedef double vec_t __attribute__((ext_vector_type(VEC)));
  const int kb = EXPECT_KC * c + 8 * lg;
#pragma unroll
  for (int m = 0; m < 2; ++m) {
    const int64_t row = tile * EXPECT_ROWS + 16 * m + li;
    const double* __restrict__ src = q + row * K + kb;
    const bool valid = row < nrows;
#pragma unroll
    for (int p = 0; p < 8; p += VEC) {
      if constexpr (VEC == 1) {
        a[m][p] = (valid && kb + p < K) ? src[p] : 0.0;
      } else {
        vec_t v;
#pragma unroll
        for (int j = 0; j < VEC; ++j) v[j] = 0.0;
        if (valid && kb + p < K) v = *(const vec_t*)(src + p);       // K % VEC == 0: the span ends at or before K
#pragma unroll
        for (int j = 0; j < VEC; ++j) a[m][p + j] = v[j];
      }
    }
  }
}

template <int NT, int VEC>
__global__ __launch_bounds__(256) void k_posterior_expect(
    const double* __restrict__ q, const double* __restrict__ table, int64_t nrows, int K, int F,
    double* __restrict__ out) {
  extern __shared__ __attribute__((aligned(16))) char expect_smem[];
  double* Bs = (double*)expect_smem;
  constexpr int FG = 16 * NT, LD = FG + EXPECT_LD_PAD;
  const int Kpad = (K + EXPECT_KC - 1) / EXPECT_KC * EXPECT_KC;
  const int f0 = FG * blockIdx.y;
  for (int i = threadIdx.x; i < Kpad * FG; i += 256) {
    const int k = i / FG, j = i - k * FG;
    Bs[k * LD + j] = (k < K && f0 + j < F) ? table[(size_t)k * F + f0 + j] : 0.0;
  }
  __syncthreads();                                   // the only barrier: the waves part ways here

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int li = lane & 15, lg = lane >> 4;
  const int64_t ntile = (nrows + EXPECT_ROWS - 1) / EXPECT_ROWS;
  const int64_t stride = (int64_t)gridDim.x * 4;
  const int nchunk = Kpad / EXPECT_KC;
  int64_t tile = (int64_t)blockIdx.x * 4 + w;
  if (tile >= ntile) return;
  int c = 0;
  ex_v4 acc[2][NT];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[m][n] = ex_v4{0.0, 0.0, 0.0, 0.0};

  // one chunk: issue the loads of what follows into `nxt`, run the chunk held in `cur`, store after a tile's last
  // chunk.  Returns false after the wave's last chunk.  (tile, c) are wave-uniform: every MFMA runs with all lanes on.
  auto step = [&](double (&cur)[2][8], double (&nxt)[2][8]) -> bool {
    int cn = c + 1;
    int64_t tn = tile;
    if (cn == nchunk) { cn = 0; tn = tile + stride; }
    const bool more = tn < ntile;
    if (more) expect_load_chunk<VEC>(nxt, q, nrows, K, tn, cn, li, lg);
    const double* bp = Bs + (EXPECT_KC * c + 8 * lg) * LD + li;
#pragma unroll
    for (int s = 0; s < 8; ++s) {
#pragma unroll
      for (int n = 0; n < NT; ++n) {
        const double b = bp[s * LD + 16 * n];
        acc[0][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[0][s], b, acc[0][n], 0, 0, 0);
        acc[1][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(cur[1][s], b, acc[1][n], 0, 0, 0);
      }
    }
    if (cn == 0) {
#pragma unroll
      for (int m = 0; m < 2; ++m)
#pragma unroll
        for (int n = 0; n < NT; ++n) {
          const int f = f0 + 16 * n + li;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int64_t row = tile * EXPECT_ROWS + 16 * m + lg + 4 * r;
            if (row < nrows && f < F) out[row * F + f] = acc[m][n][r];
          }
          acc[m][n] = ex_v4{0.0, 0.0, 0.0, 0.0};
        }
    }
    c = cn;
    tile = tn;
    return more;
  };
  double a0[2][8], a1[2][8];
  expect_load_chunk<VEC>(a0, q, nrows, K, tile, 0, li, lg);
  while (true) {
    if (!step(a0, a1)) break;
    if (!step(a1, a0)) break;
  }
}

// row[e] in [0, nrows) and col[e] in [0, F) are the host's check
__global__ __launch_bounds__(256) void k_posterior_expect_entries(
    const double* __restrict__ q, const int64_t* __restrict__ row, const int32_t* __restrict__ col,
    const double* __restrict__ table, int64_t n, int K, int F, double* __restrict__ out) {
#pragma clang fp contract(off)
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n) return;
  const double* __restrict__ qr = q + row[e] * K;
  const double* __restrict__ tc = table + col[e];
  double s = 0.0;
  for (int k = 0; k < K; ++k) {
    const double p = qr[k] * tc[(size_t)k * F];
    s = s + p;
  }
  out[e] = s;
}
