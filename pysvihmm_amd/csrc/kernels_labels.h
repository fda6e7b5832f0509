// kernels_labels.h -- partially labelled rows (svihmm_set_labels, include/svihmm.h)
//   k_label_clamp     the clamp of the lliks behind launch_emission: ll[g][k] = -inf wherever row g carries a label
//                     other than k.  A select applied after the family's llik: the kept entry is never touched, so it
//                     has its original bits, and a free row costs its label load alone.
//   k_label_gather    svihmm_estep_sequence_subset: the listed sequences' labels into the compact copy's order
//                     (k_seq_gather's sibling, launched with its grid)
// and allowed-state sets (svihmm_set_state_sets): a K-bit mask per resident row, uint64 [T][W], W = (K + 63) / 64,
// bit k % 64 of word k / 64 set where state k is allowed
//   k_set_clamp       k_label_clamp's sibling in the same frame: ll[g][k] = -inf wherever bit k of row g is clear
//   k_set_gather      k_label_gather's sibling: W words per row
// Each kernel is compiled into the one translation unit that launches it: tu_emission.hip defines
// SVIHMM_LABELS_CLAMP, tu_recursion.hip SVIHMM_LABELS_GATHER (as kernels_mcat.h splits its halves).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#ifdef SVIHMM_LABELS_CLAMP
constexpr int LC_ROWS = 64;      // rows per workgroup of k_label_clamp: 16 per wave

// grid ceil(n / LC_ROWS), block 256.  Row g of the batch is row starts[g / Lm] + g % Lm of the resident copy (the
// whole-T passes of the sequence calls are one window: starts = {0}, Lm = T).  The workgroup's LC_ROWS labels are read
// once, by its first wave, into LDS; each wave then walks its 16 rows and stores -inf over the forbidden entries of the
// labelled ones, 64 consecutive states per store.  Nothing is read from ll.  64-bit element offsets throughout.
__global__ __launch_bounds__(256) void k_label_clamp(const int32_t* __restrict__ labels,
                                                     const int64_t* __restrict__ starts, int64_t n, int Lm, int K,
                                                     double* __restrict__ ll) {
  __shared__ int32_t lab[LC_ROWS];
  const int64_t g0 = (int64_t)blockIdx.x * LC_ROWS;
  if (threadIdx.x < LC_ROWS) {
    const int64_t g = g0 + threadIdx.x;
    int32_t v = -1;
    if (g < n) {
      const int64_t w = g / Lm;
      v = labels[starts[w] + (g - w * Lm)];
    }
    lab[threadIdx.x] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const double ninf = -__builtin_huge_val();
  for (int r = wave * (LC_ROWS / 4); r < (wave + 1) * (LC_ROWS / 4); ++r) {
    const int32_t l = lab[r];          // (uniform over the wave; rows past n read -1)
    if (l < 0) continue;
    double* __restrict__ row = ll + (g0 + r) * (int64_t)K;
    for (int k = lane; k < K; k += 64)
      if (k != l) row[k] = ninf;
  }
}

// grid ceil(n / LC_ROWS), block 256, rows found as in k_label_clamp.  W = (K + 63) / 64 <= SC_WMAX words per row.  The
// workgroup's LC_ROWS * W mask words are read once into LDS, one word per thread.  Each wave owns 16 rows: its lanes
// 0 .. 15 test one row each for a word that is not all ones within K, and the ballot of those tests is the wave's list
// of constrained rows -- a free row costs its word loads and that one test, no trip of a loop.  The wave then visits
// the listed rows only, lane = state within a group of 64: the group's word is uniform over the wave, the lane tests
// its own bit and stores -inf where it is clear.  The bits of the last word at or beyond K are zero by contract; the
// k < K test keeps those lanes from storing.  A row past n is never listed.  Nothing is read from ll.  64-bit element
// offsets throughout.
constexpr int SC_WMAX = 4;       // K <= 256
__global__ __launch_bounds__(256) void k_set_clamp(const unsigned long long* __restrict__ sets,
                                                   const int64_t* __restrict__ starts, int64_t n, int Lm, int K, int W,
                                                   double* __restrict__ ll) {
  __shared__ unsigned long long msk[LC_ROWS * SC_WMAX];
  const int64_t g0 = (int64_t)blockIdx.x * LC_ROWS;
  if ((int)threadIdx.x < LC_ROWS * W) {
    const int r = threadIdx.x / W, j = threadIdx.x - r * W;
    const int64_t g = g0 + r;
    unsigned long long v = ~0ull;
    if (g < n) {
      const int64_t w = g / Lm;
      v = sets[(starts[w] + (g - w * Lm)) * (int64_t)W + j];
    }
    msk[threadIdx.x] = v;
  }
  __syncthreads();
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int r0 = wave * (LC_ROWS / 4);
  const int tail = K - (W - 1) * 64;            // states of the last word: 1 .. 64
  const unsigned long long full_tail = tail == 64 ? ~0ull : (1ull << tail) - 1ull;
  bool constrained = false;
  if (lane < LC_ROWS / 4 && g0 + r0 + lane < n) {
    const unsigned long long* m = msk + (r0 + lane) * W;
    for (int j = 0; j < W; ++j) constrained |= m[j] != (j == W - 1 ? full_tail : ~0ull);
  }
  unsigned long long todo = __ballot(constrained);       // (uniform over the wave: bit i stands for row r0 + i)
  const double ninf = -__builtin_huge_val();
  while (todo) {
    const int r = r0 + __builtin_ctzll(todo);
    todo &= todo - 1;
    double* __restrict__ row = ll + (g0 + r) * (int64_t)K;
    for (int j = 0; j < W; ++j) {
      const unsigned long long word = msk[r * W + j];
      const int k = j * 64 + lane;
      if (k < K && !((word >> lane) & 1ull)) row[k] = ninf;
    }
  }
}

#endif  // SVIHMM_LABELS_CLAMP

#ifdef SVIHMM_LABELS_GATHER
// grid (M occurrences, segments), block 256: occurrence m is rows [src_off[m], src_off[m] + len) of the resident
// labels, len = dst_off[m + 1] - dst_off[m], and becomes rows [dst_off[m], dst_off[m + 1]) of the compact ones.
__global__ __launch_bounds__(256) void k_label_gather(const int32_t* __restrict__ labels,
                                                      const int64_t* __restrict__ dst_off,
                                                      const int64_t* __restrict__ src_off,
                                                      int32_t* __restrict__ labels_out) {
  const int m = blockIdx.x;
  const int64_t d0 = dst_off[m], len = dst_off[m + 1] - d0, s0 = src_off[m];
  const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthr = (int64_t)gridDim.y * 256;
  for (int64_t i = tid; i < len; i += nthr) labels_out[d0 + i] = labels[s0 + i];
}
// the same grid; occurrence m's len * W words are contiguous in both copies
__global__ __launch_bounds__(256) void k_set_gather(const unsigned long long* __restrict__ sets,
                                                    const int64_t* __restrict__ dst_off,
                                                    const int64_t* __restrict__ src_off, int W,
                                                    unsigned long long* __restrict__ sets_out) {
  const int m = blockIdx.x;
  const int64_t d0 = dst_off[m] * W, len = dst_off[m + 1] * W - d0, s0 = src_off[m] * W;
  const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthr = (int64_t)gridDim.y * 256;
  for (int64_t i = tid; i < len; i += nthr) sets_out[d0 + i] = sets[s0 + i];
}
#endif  // SVIHMM_LABELS_GATHER
