// kernels_msg_layout.h -- where row (window w, step t) of the scaled messages Eh / ah / bh lives.
//  Row-major (every path but one): row w * Lq + t -- a window's steps are adjacent.
//  Step-major (the tiled fp64 epoch at K = 64, k_sweeps_lin<4, true, 0>): inside each group of 16 windows -- one
//  sweep workgroup -- the rows of one step are adjacent,
//      row = 16 g Lq + t nw + (w - 16 g),   g = w / 16,   nw = min(16, B - 16 g) windows in the group,
//  so that a workgroup's loads / stores of a step are ONE contiguous block of nw * K values instead of nw rows
//  Lq * K apart.  A partial last group packs its nw windows (stride nw), so the buffers keep their B * Lq rows.
//  The per-row scalars (kexp, hx, gx) and the per-window ones stay row-major in both layouts.
//  smB: the batch's window count B under the step-major layout, 0 = row-major.
#pragma once
#include <stdint.h>
__host__ __device__ __forceinline__ int msg_group_windows(int smB, int64_t w) {
  const int64_t left = (int64_t)smB - (w & ~(int64_t)15);
  return left < 16 ? (int)left : 16;
}
__host__ __device__ __forceinline__ int64_t msg_row(int smB, int Lq, int64_t w, int64_t t) {
  if (!smB) return w * Lq + t;
  return (w & ~(int64_t)15) * Lq + t * msg_group_windows(smB, w) + (w & 15);
}
