// kernels_labels.h -- partially labelled rows (svihmm_set_labels, include/svihmm.h)
//   k_label_clamp     the clamp of the lliks behind launch_emission: ll[g][k] = -inf wherever row g carries a label
//                     other than k.  A select applied after the family's llik: the kept entry is never touched, so it
//                     has its original bits, and a free row costs its label load alone.
//   k_label_gather    svihmm_estep_sequence_subset: the listed sequences' labels into the compact copy's order
//                     (k_seq_gather's sibling, launched with its grid)
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
#endif  // SVIHMM_LABELS_GATHER
