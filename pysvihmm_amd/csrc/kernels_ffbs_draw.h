// kernels_ffbs_draw.h -- the backward-sampling draw, written ONCE for every FFBS kernel.  Included by tu_recursion.hip
// before kernels_recursion.h (k_ffbs_paths / k_ffbs_paths_wide, uncoupled branch), kernels_ffbs_windows.h
// (k_ffbs_win / k_ffbs_win_wide) and kernels_decode_sequences.h (k_ffbs_seq / k_ffbs_seq_wide).
//
//   z ~ softmax_k lp_k,   lp_k = lalpha[t][k] + logA[k][z_next]   (no transition term on a path's first draw)
// by the inverse-CDF rule: m = max_k lp_k, p_k = exp(lp_k - m), c_k the running sum in state order, the draw the
// smallest k with u * c_{K-1} <= c_k (K - 1 if none).  The operation order is part of the contract
// (include/svihmm.h): a change here changes every sampler alike.
#pragma once

// logA transposed into LDS, lAT[s * (KMAX + 1) + k] = logA[k * K + s]: the row a lane reads is chosen by its own
// z_next; row stride KMAX + 1 doubles = 2 (mod 64) dwords, so the 32 lanes of a ds_read_b64 group hit 32 different
// bank pairs (or, on the same row, broadcast).  One wave; the caller's barrier publishes it.
template <int KMAX>
__device__ __forceinline__ void ffbs_stage_logAT(double* lAT, const double* logA, int K, int lane) {
  for (int e = lane; e < K * K; e += 64) {
    const int k = e / K, sidx = e - k * K;
    lAT[sidx * (KMAX + 1) + k] = logA[e];
  }
}

// K <= 64: the K terms in registers, one exp per state.  out = the drawn state; ROWK: entry k of the lalpha row as an
// expression in k (a row padded with -inf in LDS: rw[k]; a row of K entries read where it lies: the k < K guard
// supplies the -inf); tr: row z_next of lAT.
// A macro, not a function: the compiler simplifies a function on its own before it inlines it and the result, though
// the same arithmetic, costs the kernels registers (k_ffbs_win<32>: 190 -> 191 VGPRs; <64>: 44 -> 46 AGPRs).
#define FFBS_DRAW(out, KMAX, ROWK, tr, first, K, r)                              \
  do {                                                                           \
    double lp[KMAX], m = -INFINITY;                                              \
    _Pragma("unroll") for (int k = 0; k < KMAX; ++k) {                           \
      lp[k] = (ROWK) + (((first) || k >= (K)) ? 0.0 : (tr)[k]);                  \
      m = fmax(m, lp[k]);                                                        \
    }                                                                            \
    double tot = 0.0;                                                            \
    _Pragma("unroll") for (int k = 0; k < KMAX; ++k) {                           \
      lp[k] = k < (K) ? exp(lp[k] - m) : 0.0;                                    \
      tot += lp[k];                                                              \
    }                                                                            \
    const double thr = (r) * tot;                                                \
    double c = 0.0;                                                              \
    int zz = (K) - 1;                                                            \
    bool found = false;                                                          \
    _Pragma("unroll") for (int k = 0; k < KMAX; ++k) {                           \
      c += lp[k];                                                                \
      const bool hit = !found && k < (K) && thr <= c;                            \
      zz = hit ? k : zz;                                                         \
      found = found || hit;                                                      \
    }                                                                            \
    (out) = zz;                                                                  \
  } while (0)

// 64 < K <= 256: three passes over the K source states (maximum, total, inverse CDF with early exit), the terms
// recomputed in each.  rw: the lalpha row (K entries, LDS or L2); col = logA + z_next: logA[k][z_next] = col[k * K].
__device__ __forceinline__ int ffbs_draw_wide(const double* rw, const double* __restrict__ col, bool first, int K,
                                              double r) {
  double m = -INFINITY;
  for (int k = 0; k < K; ++k) m = fmax(m, rw[k] + (first ? 0.0 : col[(size_t)k * K]));
  double tot = 0.0;
  for (int k = 0; k < K; ++k) tot += exp(rw[k] + (first ? 0.0 : col[(size_t)k * K]) - m);
  const double thr = r * tot;
  double c = 0.0;
  int zz = K - 1;
  for (int k = 0; k < K; ++k) {
    c += exp(rw[k] + (first ? 0.0 : col[(size_t)k * K]) - m);
    if (thr <= c) { zz = k; break; }
  }
  return zz;
}
