// kernels_ffbs_windows.h -- backward sampling for window batches x draws (svihmm_ffbs_windows): S draws of
// every window of a batch from ONE forward filter.  lalpha [B][Lm][K] is resident (launch_fb / the chain scan);
// a draw walks one window backwards,
//     z[Lm-1] ~ softmax_k lalpha[Lm-1][k],   z[t] ~ softmax_k (lalpha[t][k] + logA[k][z[t+1]]),
// by the inverse-CDF draw every FFBS kernel shares (kernels_ffbs_draw.h):  lp_k the sum above,
// m = max_k lp_k, p_k = exp(lp_k - m), c_k the running sum in state order, the draw the smallest k with
// u * c_{K-1} <= c_k (K - 1 if none).
//
// The S * B walks are independent and each is sequential in t, so the parallel axis is the (window, draw)
// pair: ONE LANE PER PAIR, pairs p = b * S + s packed densely into waves of 64 -- 3891 windows x 1 draw and
// 1 window x 4096 draws fill the lanes alike, and the lanes of a wave that share a window are neighbours.
// A pair's arithmetic involves nothing of its neighbours, so a path does not depend on S, B or its lane.
//
// K <= 64 (k_ffbs_win<KMAX>, one wave per workgroup), LDS:
//   lAT  [K][KMAX + 1]            logA transposed, lAT[z_next][k] = logA[k][z_next]; the row a lane reads is
//                                 chosen by its own z[t+1]: row stride KMAX + 1 doubles = 2 (mod 64) dwords, so
//                                 the 32 lanes of a ds_read_b64 group hit 32 different bank pairs (or, on the
//                                 same row, broadcast)
//   rows [RT][nwmax][KMAX + 1]    the lalpha rows of RT steps of the wave's windows (at most nwmax distinct
//                                 ones), staged with coalesced loads, all RT * nw rows in flight together;
//                                 lanes of one window broadcast, lanes of different windows are KMAX + 1 apart.
//                                 RT = as many steps as fit FFW_ROW_BYTES (at least one): the load latency is
//                                 paid once per RT steps, not once per step of the dependent chain
//   zt   [64][FFW_ZT + 1] int32   the last FFW_ZT states of every lane, flushed so that consecutive lanes
//                                 write consecutive steps of one path (128-byte runs) instead of 64 scattered
//                                 4-byte stores per step
// At KMAX = 64 that is 33 KB + max(16 KB, one step of the wave's windows: up to 33 KB) + 9 KB: two workgroups
// per CU, one when a wave spans 32 windows or more.
// Registers: lp[KMAX] doubles per lane as in k_ffbs_paths (128 VGPRs at KMAX = 64; 256 VGPRs + 44 AGPRs in all,
// one wave per SIMD, no scratch; 190 at KMAX = 32, 118 at KMAX = 16).
// A step costs KMAX exps per lane: 8.7 us at KMAX = 64 on an MI355X ("FFBS for windows"),
// 15.6 us where a wave spans 64 windows and stages 64 rows for every step; the uniform of the next step is
// fetched (or computed: Philox) before the draw of the current one.
//
// 64 < K <= 256 (k_ffbs_win_wide): the three passes of ffbs_draw_wide (maximum, total, inverse CDF) per lane; the lalpha row (same address in the lanes of one window) and the transition column
// come from L2, only the z tile uses LDS.
#pragma once

constexpr int FFW_ZT = 32;              // steps of z parked in LDS between two flushes
constexpr int FFW_ROW_BYTES = 16384;    // LDS budget of the staged lalpha rows (one step is always staged)
constexpr int FFW_SWITCH = 2048;        // windows of at least this many rows take the blocked composition

// distinct windows among 64 consecutive pairs p = b * S + s
inline int ffw_windows_per_wave(int B, int S) {
  const int n = 63 / S + 2;
  return n < B ? (n < 64 ? n : 64) : (B < 64 ? B : 64);
}
inline int ffw_row_tile(int nwmax, int KMAX, int Lm) {
  int rt = FFW_ROW_BYTES / (nwmax * (KMAX + 1) * (int)sizeof(double));
  rt = rt < 1 ? 1 : rt > FFW_ZT ? FFW_ZT : rt;
  return rt < Lm ? rt : Lm;
}
inline size_t ffw_lds_bytes(int K, int KMAX, int nwmax, int RT) {
  return ((size_t)K * (KMAX + 1) + (size_t)RT * nwmax * (KMAX + 1) + 64) * sizeof(double) +
         (size_t)64 * (FFW_ZT + 1) * sizeof(int);
}

// u of flattened output index g = (s * B + b) * Lm + t: the caller's, or Philox row g, stream 0
__device__ __forceinline__ double ffw_uniform(const double* __restrict__ unif, unsigned long long seed, int64_t g) {
  if (unif) return unif[g];
  unsigned w[4];
  philox4x32_10(seed, (unsigned long long)g, 0u, w);
  return u53(w[0], w[1]);
}

template <int KMAX>
__global__ __launch_bounds__(64) void k_ffbs_win(
    const double* __restrict__ la, const double* __restrict__ logA, const double* __restrict__ unif,
    unsigned long long seed, int B, int S, int Lm, int K, int nwmax, int RT, int32_t* __restrict__ z) {
  extern __shared__ double fws[];
  double* lAT = fws;                                             // [K][KMAX + 1]
  double* rows = lAT + K * (KMAX + 1);                           // [RT][nwmax][KMAX + 1]
  long long* gb = (long long*)(rows + (size_t)RT * nwmax * (KMAX + 1));   // [64] output offset of the lane's path
  int* zt = (int*)(gb + 64);                                     // [64][FFW_ZT + 1]
  const int lane = threadIdx.x;
  ffbs_stage_logAT<KMAX>(lAT, logA, K, lane);
  const int64_t npairs = (int64_t)B * S;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const bool valid = p0 + lane < npairs;
  const int64_t p = valid ? p0 + lane : npairs - 1;              // (idle lanes shadow the last pair, store nothing)
  const int b = (int)(p / S), s = (int)(p - (int64_t)b * S);
  const int b0 = (int)(p0 / S);
  const int64_t plast = p0 + 63 < npairs ? p0 + 63 : npairs - 1;
  const int nw = (int)(plast / S) - b0 + 1;                      // <= nwmax
  const int w = b - b0;
  const int64_t g0 = ((int64_t)s * B + b) * Lm;
  gb[lane] = valid ? (long long)g0 : -1;
  int cur = 0;
  double unext = ffw_uniform(unif, seed, g0 + Lm - 1);
  for (int thi = Lm; thi > 0; thi -= FFW_ZT) {
    const int tlo = thi > FFW_ZT ? thi - FFW_ZT : 0;
    for (int rhi = thi; rhi > tlo; rhi -= RT) {
      const int rlo = rhi - RT > tlo ? rhi - RT : tlo;
      __syncthreads();                                           // (lAT staged; the previous tile's readers are done)
      // the wave copies 64 / KMAX rows per pass (lane = (row of the pass, state)), eight passes' loads in flight;
      // row r of the tile = (step r / nw, window r % nw): r < 2048 and nw <= 64, so the float quotient of
      // r + 0.5 is at least 1 / 128 away from an integer and truncates to the exact one
      constexpr int RPI = 64 / KMAX;
      const int sub = lane / KMAX, k = lane & (KMAX - 1), kc = k < K ? k : 0;
      const int nrows = (rhi - rlo) * nw;
      const float inv_nw = 1.0f / (float)nw;
      for (int r0 = 0; r0 < nrows; r0 += 8 * RPI) {
        double v[8];
        int off[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) {
          const int r = r0 + j * RPI + sub, rc = r < nrows ? r : nrows - 1;
          const int tt = (int)(((float)rc + 0.5f) * inv_nw), ww = rc - tt * nw;
          off[j] = (tt * nwmax + ww) * (KMAX + 1) + k;
          v[j] = la[((int64_t)(b0 + ww) * Lm + rlo + tt) * K + kc];
        }
#pragma unroll
        for (int j = 0; j < 8; ++j)
          if (r0 + j * RPI + sub < nrows) rows[off[j]] = k < K ? v[j] : -INFINITY;
      }
      __syncthreads();
      for (int t = rhi - 1; t >= rlo; --t) {
        const double r = unext;
        if (t > 0) unext = ffw_uniform(unif, seed, g0 + t - 1);
        const bool first = t == Lm - 1;                          // no transition term
        const double* rw = rows + ((size_t)(t - rlo) * nwmax + w) * (KMAX + 1);
        const double* tr = lAT + cur * (KMAX + 1);
        FFBS_DRAW(cur, KMAX, rw[k], tr, first, K, r);
        zt[lane * (FFW_ZT + 1) + (t - tlo)] = cur;
      }
    }
    __syncthreads();
    const int nt = thi - tlo;
    for (int e = lane; e < 64 * nt; e += 64) {
      const int pl = e / nt, tt = e - pl * nt;
      const long long g = gb[pl];
      if (g >= 0) z[g + tlo + tt] = zt[pl * (FFW_ZT + 1) + tt];
    }
  }
}

__global__ __launch_bounds__(64) void k_ffbs_win_wide(
    const double* __restrict__ la, const double* __restrict__ logA, const double* __restrict__ unif,
    unsigned long long seed, int B, int S, int Lm, int K, int32_t* __restrict__ z) {
  __shared__ long long gb[64];
  __shared__ int zt[64 * (FFW_ZT + 1)];
  const int lane = threadIdx.x;
  const int64_t npairs = (int64_t)B * S;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const bool valid = p0 + lane < npairs;
  const int64_t p = valid ? p0 + lane : npairs - 1;
  const int b = (int)(p / S), s = (int)(p - (int64_t)b * S);
  const int64_t g0 = ((int64_t)s * B + b) * Lm;
  gb[lane] = valid ? (long long)g0 : -1;
  int cur = 0;
  double unext = ffw_uniform(unif, seed, g0 + Lm - 1);
  for (int thi = Lm; thi > 0; thi -= FFW_ZT) {
    const int tlo = thi > FFW_ZT ? thi - FFW_ZT : 0;
    __syncthreads();                                             // (the previous flush has read zt)
    for (int t = thi - 1; t >= tlo; --t) {
      const double r = unext;
      if (t > 0) unext = ffw_uniform(unif, seed, g0 + t - 1);
      const bool first = t == Lm - 1;
      const double* __restrict__ rw = la + ((int64_t)b * Lm + t) * K;
      cur = ffbs_draw_wide(rw, logA + cur, first, K, r);
      zt[lane * (FFW_ZT + 1) + (t - tlo)] = cur;
    }
    __syncthreads();
    const int nt = thi - tlo;
    for (int e = lane; e < 64 * nt; e += 64) {
      const int pl = e / nt, tt = e - pl * nt;
      const long long g = gb[pl];
      if (g >= 0) z[g + tlo + tt] = zt[pl * (FFW_ZT + 1) + tt];
    }
  }
}

// long windows (blocked composition per (window, draw)): the Philox uniforms of one path, and its states
// into the int32 [S][B][Lm] output
__global__ __launch_bounds__(256) void k_ffw_fill_uniforms(unsigned long long seed, int64_t g0, int64_t n,
                                                           double* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) out[t] = ffw_uniform(nullptr, seed, g0 + t);
}
__global__ __launch_bounds__(256) void k_ffw_store_path(const int64_t* __restrict__ zin, int64_t n,
                                                        int32_t* __restrict__ out) {
  const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (t < n) out[t] = (int32_t)zin[t];
}
