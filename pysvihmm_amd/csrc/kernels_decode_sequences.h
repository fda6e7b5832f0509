// kernels_decode_sequences.h -- decoding all declared sequences in one call (svihmm_viterbi_sequences,
// svihmm_ffbs_sequences): what is truly RAGGED about it.  Included by tu_recursion.hip after kernels_ffbs_draw.h (the
// draw), kernels_viterbi.h (the Viterbi kernels and their VitSequences policy), kernels_ffbs_windows.h (ffw_uniform,
// FFW_ZT) and kernels_sequences.h (whose sweeps, launched with one direction, are the forward filter of the sampler).
//
// The resident rows are N chains laid end to end (seq_off[N + 1]); ll / lalpha are ONE [T][K] array addressed by the
// resident row.  The unit of work is a sequence taken from an `order` array (longest first, as k_seq_wave does), so a
// sequence's result never depends on what else is declared or where it lies.
//
// Viterbi.  The forward sweeps and k_vit_paths are kernels_viterbi.h's, instantiated with VitSequences; only the
// gather differs in shape (k_vitseq_gather below: a workgroup per chunk of the long sequences' padded run).
//
// FFBS.  k_ffbs_seq<KMAX> / k_ffbs_seq_wide: ONE LANE PER (sequence, draw) pair, p = rank(s) * S + draw with rank
// the longest-first order, so the lanes of a wave walk sequences of similar length.  Step i counts back from each
// lane's own last row; a lane idles once i >= len; the wave runs to the longest of its lanes (its first).  logA
// transposed in LDS and the z tile flush are k_ffbs_win's; the lalpha row of a step is read from L2 by the lane
// itself (not staged in LDS: lanes of one sequence broadcast, a row's K doubles are contiguous), so the draw is
// FFBS_DRAW over a guarded row.  The uniform of (draw, resident row r) is entry draw * T + r.
#pragma once

// one workgroup per chunk: z[resident row] = path[padded row][entry of the chunk]
__global__ __launch_bounds__(256) void k_vitseq_gather(
    const unsigned char* __restrict__ path, const unsigned char* __restrict__ entry, VitSequences units, int Ls,
    int KS, int32_t* __restrict__ z) {
  const int c = blockIdx.x;
  int u, cw;
  units.chunk(c, Ls, u, cw);
  const VitUnit w = units.unit<false>(u);
  const int lo = cw * Ls;
  const int n = w.len - lo < Ls ? w.len - lo : Ls;
  const size_t row0 = w.prow + lo;
  const int en = entry[c];
  for (int r = threadIdx.x; r < n; r += 256) z[w.row0 + lo + r] = path[(row0 + r) * KS + en];
}

// ---- backward sampling -------------------------------------------------------------------------
inline size_t ffs_lds_bytes(int K, int KMAX) {
  return ((size_t)K * (KMAX + 1) + 64) * sizeof(double) + (size_t)64 * (FFW_ZT + 2) * sizeof(int);
}

template <int KMAX>
__global__ __launch_bounds__(64) void k_ffbs_seq(
    const double* __restrict__ la, const double* __restrict__ logA, const double* __restrict__ unif,
    unsigned long long seed, const int64_t* __restrict__ seq_off, const int32_t* __restrict__ order, int nseq, int S,
    int64_t T, int K, int32_t* __restrict__ z) {
  extern __shared__ double fss[];
  double* lAT = fss;                                             // [K][KMAX + 1]
  long long* gb = (long long*)(lAT + K * (KMAX + 1));            // [64] output offset of row 0 of the lane's path
  int* lenL = (int*)(gb + 64);                                   // [64] rows of the lane's sequence
  int* zt = lenL + 64;                                           // [64][FFW_ZT + 1]
  const int lane = threadIdx.x;
  ffbs_stage_logAT<KMAX>(lAT, logA, K, lane);
  const int64_t npairs = (int64_t)nseq * S;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const bool valid = p0 + lane < npairs;
  const int64_t p = valid ? p0 + lane : npairs - 1;              // (idle lanes shadow the last pair, store nothing)
  const int rank = (int)(p / S), draw = (int)(p - (int64_t)rank * S);
  const int s = order[rank];
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  const int s0 = order[(int)(p0 / S)];                           // the wave's first pair: its longest sequence
  const int len0 = (int)(seq_off[s0 + 1] - seq_off[s0]);
  const int64_t g0 = (int64_t)draw * T + r0;
  gb[lane] = valid ? (long long)g0 : -1;
  lenL[lane] = len;
  const double* __restrict__ lseq = la + (size_t)r0 * K;
  int cur = 0;
  double unext = ffw_uniform(unif, seed, g0 + len - 1);
  for (int i0 = 0; i0 < len0; i0 += FFW_ZT) {
    const int nt = len0 - i0 < FFW_ZT ? len0 - i0 : FFW_ZT;
    __syncthreads();                                             // (lAT staged; the previous flush has read zt)
    for (int ii = 0; ii < nt; ++ii) {
      const int t = len - 1 - (i0 + ii);
      if (t >= 0) {                                              // (a shorter sequence's lane idles)
        const double r = unext;
        if (t > 0) unext = ffw_uniform(unif, seed, g0 + t - 1);
        const bool first = t == len - 1;                         // no transition term
        const double* __restrict__ rw = lseq + (size_t)t * K;
        const double* tr = lAT + cur * (KMAX + 1);
        FFBS_DRAW(cur, KMAX, (k < K ? rw[k] : -INFINITY), tr, first, K, r);
        zt[lane * (FFW_ZT + 1) + ii] = cur;
      }
    }
    __syncthreads();
    for (int e = lane; e < 64 * nt; e += 64) {
      const int pl = e / nt, ii = e - pl * nt;
      const long long g = gb[pl];
      const int t = lenL[pl] - 1 - (i0 + ii);
      if (g >= 0 && t >= 0) z[g + t] = zt[pl * (FFW_ZT + 1) + ii];
    }
  }
}

__global__ __launch_bounds__(64) void k_ffbs_seq_wide(
    const double* __restrict__ la, const double* __restrict__ logA, const double* __restrict__ unif,
    unsigned long long seed, const int64_t* __restrict__ seq_off, const int32_t* __restrict__ order, int nseq, int S,
    int64_t T, int K, int32_t* __restrict__ z) {
  __shared__ long long gb[64];
  __shared__ int lenL[64];
  __shared__ int zt[64 * (FFW_ZT + 1)];
  const int lane = threadIdx.x;
  const int64_t npairs = (int64_t)nseq * S;
  const int64_t p0 = (int64_t)blockIdx.x * 64;
  const bool valid = p0 + lane < npairs;
  const int64_t p = valid ? p0 + lane : npairs - 1;
  const int rank = (int)(p / S), draw = (int)(p - (int64_t)rank * S);
  const int s = order[rank];
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  const int s0 = order[(int)(p0 / S)];
  const int len0 = (int)(seq_off[s0 + 1] - seq_off[s0]);
  const int64_t g0 = (int64_t)draw * T + r0;
  gb[lane] = valid ? (long long)g0 : -1;
  lenL[lane] = len;
  const double* __restrict__ lseq = la + (size_t)r0 * K;
  int cur = 0;
  double unext = ffw_uniform(unif, seed, g0 + len - 1);
  for (int i0 = 0; i0 < len0; i0 += FFW_ZT) {
    const int nt = len0 - i0 < FFW_ZT ? len0 - i0 : FFW_ZT;
    __syncthreads();                                             // (the previous flush has read zt)
    for (int ii = 0; ii < nt; ++ii) {
      const int t = len - 1 - (i0 + ii);
      if (t >= 0) {
        const double r = unext;
        if (t > 0) unext = ffw_uniform(unif, seed, g0 + t - 1);
        const bool first = t == len - 1;
        const double* __restrict__ rw = lseq + (size_t)t * K;
        cur = ffbs_draw_wide(rw, logA + cur, first, K, r);
        zt[lane * (FFW_ZT + 1) + ii] = cur;
      }
    }
    __syncthreads();
    for (int e = lane; e < 64 * nt; e += 64) {
      const int pl = e / nt, ii = e - pl * nt;
      const long long g = gb[pl];
      const int t = lenL[pl] - 1 - (i0 + ii);
      if (g >= 0 && t >= 0) z[g + t] = zt[pl * (FFW_ZT + 1) + ii];
    }
  }
}
