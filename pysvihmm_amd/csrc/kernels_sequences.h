// kernels_sequences.h -- svihmm_estep_sequences: forward / backward sweeps over RAGGED sequences, their posterior
// pass and the boundary correction of the transition statistic.  Included by tu_recursion.hip after
// kernels_recursion.h (block_max, the posterior's row arithmetic and the wave helpers are shared).
//
// The resident rows are N chains laid end to end; seq_off[N + 1] are their offsets.  The unit of work of the
// sweeps is a (sequence, direction) pair: blockIdx.x indexes `order` (the sequences this launch serves, longest
// first, so that the launch's tail is short), blockIdx.y is the direction.  Sequence s reads rows
// [seq_off[s], seq_off[s+1]) of ONE [rows, K] llik array whose row 0 is global row `row_base`, and writes lalpha /
// lbeta at the same rows of two scratch arrays.  Nothing a unit computes depends on another unit: a sequence's
// messages, posterior rows and local_lb are the same bits whatever else is declared, in whatever order.
//   k_seq_wave<KMAX>   K <= KMAX <= 64: one wavefront per unit, lane = state, the transition column (forward) /
//                      row (backward) of exp(ltran) in registers, the shifted probabilities exchanged through LDS:
//                      per state and step one exp, KMAX fused multiply-adds, one log (k_fb_wave's step); the ll
//                      rows are off the dependent chain, loaded eight steps ahead (k_vit_wave's prefetch).
//   k_seq_block        64 < K <= 256: one workgroup per unit, thread = state (k_fb_generic's step).
//   k_seq_exact        transition expectations below exp()'s range: the literal logaddexp recursion, one exp per
//                      (source, target) pair and step (k_fb_exact's step), any K <= 256.
//   k_seq_posterior    q = softmax_k(lalpha + lbeta) at the concatenated row index and LSE_k lalpha per row,
//                      one wave per row (k_posterior's row arithmetic);
//   k_seq_lb           local_lb[s] = sum_t LSE_k lalpha_t[k] (quirk Q4): one wave per sequence, lane-strided
//                      partial sums and one butterfly -- the order depends on the sequence's length alone.
//   k_seq_fix          A_raw of ONE window over all T rows -> sum over the sequences: the N - 1 join pairs
//                      (last row of s, first row of s + 1) come out, under SVIHMM_TRANS_WRAP each sequence's own
//                      (last row, first row) pair goes in; q0 = sum_s q[seq_off[s]].  One thread per entry,
//                      ascending s: no atomics, one fixed order.
//   k_seq_gather       svihmm_estep_sequence_subset: the listed sequences' rows (and mask bytes) copied bit for
//                      bit into a compact copy laid end to end in the order of the list; everything above then
//                      runs on that copy with the compact offsets, so its cost follows the listed rows.
#pragma once

#define SEQ_PREFETCH 8

template <int KMAX>
__global__ __launch_bounds__(64) void k_seq_wave(
    const double* __restrict__ ll, int64_t row_base, const int64_t* __restrict__ seq_off,
    const int32_t* __restrict__ order, const double* __restrict__ Aexp, const double* __restrict__ mod_init,
    int K, double* __restrict__ la_out, double* __restrict__ lb_out) {
  __shared__ double p_s[2][KMAX];
  const int s = order[blockIdx.x], dir = blockIdx.y, j = threadIdx.x;
  const bool valid = j < K;
  const int jc = valid ? j : 0;
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  double a[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) {
    double v = 0.0;
    if (valid && i < K) v = (dir == 0) ? Aexp[i * K + j] : Aexp[j * K + i];
    a[i] = v;
  }
  const size_t base = (size_t)(r0 - row_base) * K;
  const double* __restrict__ lw = ll + base + jc;
  const double NEG_INF = -INFINITY;
  constexpr int U = SEQ_PREFETCH;
  double cur[U], nxt[U];
  int pc = 0;
  if (dir == 0) {
    double* out = la_out + base;
    double la = valid ? mod_init[jc] + lw[0] : NEG_INF;
    if (valid) out[j] = la;
#pragma unroll
    for (int u = 0; u < U; ++u) { const int t = 1 + u < len ? 1 + u : len - 1; cur[u] = lw[(size_t)t * K]; }
    for (int t0 = 1; t0 < len; t0 += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) { const int t = t0 + U + u < len ? t0 + U + u : len - 1; nxt[u] = lw[(size_t)t * K]; }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int t = t0 + u;
        if (t < len) {                                   // (uniform)
          const double m = wave64_max_fast(la);
          const double p = valid ? fast_exp(la - m) : 0.0;
          if (j < KMAX) p_s[pc][j] = p;
          __syncthreads();
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int i = 0; i < KMAX; i += 2) {
            s0 = fma(p_s[pc][i], a[i], s0);
            s1 = fma(p_s[pc][i + 1], a[i + 1], s1);
          }
          pc ^= 1;
          la = valid ? fast_log(s0 + s1) + m + cur[u] : NEG_INF;
          if (valid) out[(size_t)t * K + j] = la;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
  } else {
    double* out = lb_out + base;
    double lb = 0.0;
    if (valid) out[(size_t)(len - 1) * K + j] = 0.0;
    // step i = 0 .. len - 2 forms lbeta[len - 2 - i] from row len - 1 - i
#pragma unroll
    for (int u = 0; u < U; ++u) { const int t = len - 1 - u > 0 ? len - 1 - u : 0; cur[u] = lw[(size_t)t * K]; }
    for (int i0 = 0; i0 < len - 1; i0 += U) {
#pragma unroll
      for (int u = 0; u < U; ++u) { const int t = len - 1 - (i0 + U + u) > 0 ? len - 1 - (i0 + U + u) : 0; nxt[u] = lw[(size_t)t * K]; }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int i = i0 + u;
        if (i < len - 1) {                               // (uniform)
          const int t = len - 2 - i;
          const double v = valid ? lb + cur[u] : NEG_INF;
          const double m = wave64_max_fast(v);
          const double p = valid ? fast_exp(v - m) : 0.0;
          if (j < KMAX) p_s[pc][j] = p;
          __syncthreads();
          double s0 = 0.0, s1 = 0.0;
#pragma unroll
          for (int ii = 0; ii < KMAX; ii += 2) {
            s0 = fma(p_s[pc][ii], a[ii], s0);
            s1 = fma(p_s[pc][ii + 1], a[ii + 1], s1);
          }
          pc ^= 1;
          lb = fast_log(s0 + s1) + m;
          if (valid) out[(size_t)t * K + j] = lb;
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) cur[u] = nxt[u];
    }
  }
}

// 64 < K <= 256: block = roundup(K, 64) threads, thread = state; the transition matrix (forward: A, backward: A^T)
// in LDS when it fits, else streamed from L2.  Dynamic LDS: [2][K] probabilities | [16] reduction | [K][K] matrix.
__global__ void k_seq_block(const double* __restrict__ ll, int64_t row_base, const int64_t* __restrict__ seq_off,
                            const int32_t* __restrict__ order, const double* __restrict__ Aexp,
                            const double* __restrict__ AexpT, const double* __restrict__ mod_init, int K,
                            int m_in_lds, double* __restrict__ la_out, double* __restrict__ lb_out) {
  extern __shared__ double seq_sm[];
  double* p_s = seq_sm;            // [2][K]
  double* red = seq_sm + 2 * K;    // [16]
  double* M_s = red + 16;          // [K][K] if m_in_lds
  const int s = order[blockIdx.x], dir = blockIdx.y, j = threadIdx.x;
  const int nw = (blockDim.x + 63) >> 6;
  const bool valid = j < K;
  const int jc = valid ? j : 0;
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  const double* Mg = (dir == 0) ? Aexp : AexpT;
  const double* M = Mg;
  if (m_in_lds) {
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) M_s[e] = Mg[e];
    M = M_s;
  }
  __syncthreads();
  const size_t base = (size_t)(r0 - row_base) * K;
  const double* __restrict__ lw = ll + base + jc;
  const double NEG_INF = -INFINITY;
  int pc = 0;
  if (dir == 0) {
    double* out = la_out + base;
    double la = valid ? mod_init[jc] + lw[0] : NEG_INF;
    if (valid) out[j] = la;
    double llnext = lw[(size_t)(1 < len ? 1 : len - 1) * K];
    for (int t = 1; t < len; ++t) {
      const double llt = llnext;
      llnext = lw[(size_t)(t + 1 < len ? t + 1 : len - 1) * K];
      const double m = block_max(la, red, nw);
      if (valid) p_s[pc * K + j] = exp(la - m);
      __syncthreads();
      double sum = 0.0;
      if (valid)
        for (int i = 0; i < K; ++i) sum = fma(p_s[pc * K + i], M[(size_t)i * K + j], sum);
      pc ^= 1;
      la = valid ? log(sum) + m + llt : NEG_INF;
      if (valid) out[(size_t)t * K + j] = la;
    }
  } else {
    double* out = lb_out + base;
    double lb = 0.0;
    if (valid) out[(size_t)(len - 1) * K + j] = 0.0;
    double llnext = lw[(size_t)(len - 1) * K];
    for (int t = len - 2; t >= 0; --t) {
      const double v = valid ? lb + llnext : NEG_INF;
      llnext = lw[(size_t)(t > 0 ? t : 0) * K];
      const double m = block_max(v, red, nw);
      if (valid) p_s[pc * K + j] = exp(v - m);
      __syncthreads();
      double sum = 0.0;
      if (valid)
        for (int i = 0; i < K; ++i) sum = fma(p_s[pc * K + i], M[(size_t)i * K + j], sum);
      pc ^= 1;
      lb = log(sum) + m;
      if (valid) out[(size_t)t * K + j] = lb;
    }
  }
}

// Sparse globals: np.logaddexp.reduce over (message + ltran) literally (hmmbase.py:295, 319).  Block =
// roundup(K, 64) threads, thread = state; ltran in LDS (row stride K + 1) when it fits.
// Dynamic LDS: [2][K] messages | [K][K + 1] ltran.
__global__ void k_seq_exact(const double* __restrict__ ll, int64_t row_base, const int64_t* __restrict__ seq_off,
                            const int32_t* __restrict__ order, const double* __restrict__ ltran,
                            const double* __restrict__ mod_init, int K, int lt_in_lds,
                            double* __restrict__ la_out, double* __restrict__ lb_out) {
  extern __shared__ double seq_sm[];
  double* v_s = seq_sm;              // [2][K]
  double* lt_s = seq_sm + 2 * K;     // [K][K + 1] if lt_in_lds
  const int s = order[blockIdx.x], dir = blockIdx.y, j = threadIdx.x;
  const bool valid = j < K;
  const int jc = valid ? j : 0;
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  const int ls = lt_in_lds ? K + 1 : K;
  const double* lt = ltran;
  if (lt_in_lds) {
    for (int e = threadIdx.x; e < K * K; e += blockDim.x) lt_s[(e / K) * (K + 1) + e % K] = ltran[e];
    lt = lt_s;
  }
  const size_t base = (size_t)(r0 - row_base) * K;
  const double* __restrict__ lw = ll + base + jc;
  // element (source i, target j) as seen from thread j: forward lt[i][j], backward (thread = source) lt[j][i]
  const size_t si = dir == 0 ? (size_t)ls : 1, sj = dir == 0 ? 1 : (size_t)ls;
  const double* mycol = lt + (size_t)jc * sj;
  int pc = 0;
  auto lse = [&](const double* v) {
    double m = -INFINITY;
    for (int i = 0; i < K; ++i) m = fmax(m, v[i] + mycol[i * si]);
    if (!(m > -INFINITY)) return m;            // all terms -inf (or NaN): as np.logaddexp.reduce
    if (!(m < INFINITY)) return m;
    double sum = 0.0;                          // (terms 50 nats below the maximum cannot change the sum)
    for (int i = 0; i < K; ++i) {
      const double d = v[i] + mycol[i * si] - m;
      if (d > -50.0) sum += exp(d);
    }
    return m + log(sum);
  };
  if (dir == 0) {
    double* out = la_out + base;
    double la = valid ? mod_init[jc] + lw[0] : -INFINITY;
    if (valid) out[j] = la;
    for (int t = 1; t < len; ++t) {
      if (valid) v_s[pc * K + j] = la;
      __syncthreads();
      if (valid) {
        la = lse(v_s + pc * K) + lw[(size_t)t * K];
        out[(size_t)t * K + j] = la;
      }
      pc ^= 1;
    }
  } else {
    double* out = lb_out + base;
    double lb = 0.0;
    if (valid) out[(size_t)(len - 1) * K + j] = 0.0;
    for (int t = len - 2; t >= 0; --t) {
      if (valid) v_s[pc * K + j] = lb + lw[(size_t)(t + 1) * K];
      __syncthreads();
      if (valid) {
        lb = lse(v_s + pc * K);
        out[(size_t)t * K + j] = lb;
      }
      pc ^= 1;
    }
  }
}

// Posterior rows of the sequences in `order`: grid (sequences, segments), block 256 = 4 waves, one wave per
// row; the rows of a sequence are dealt round-robin to the gridDim.y * 4 waves that serve it.  q goes to the
// CONCATENATED row (global row index), the row's LSE_k lalpha to row_lse at the scratch row.
template <int KPL>  // states per lane (K <= 64 * KPL)
__global__ __launch_bounds__(256) void k_seq_posterior(
    const double* __restrict__ la, const double* __restrict__ lb, int64_t row_base,
    const int64_t* __restrict__ seq_off, const int32_t* __restrict__ order, int K,
    double* __restrict__ q, double* __restrict__ row_lse) {
  const int s = order[blockIdx.x];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  const int stride = 4 * gridDim.y;
  for (int t = blockIdx.y * 4 + wave; t < len; t += stride) {
    const size_t srow = (size_t)(r0 - row_base) + t;
    const size_t base = srow * K, qbase = ((size_t)r0 + t) * K;
    double u[KPL], a[KPL];
    double mu = -INFINITY, ma = -INFINITY;
#pragma unroll
    for (int c = 0; c < KPL; ++c) {
      const int k = lane + 64 * c;
      if (k < K) {
        a[c] = la[base + k];
        u[c] = a[c] + lb[base + k];
      } else {
        a[c] = -INFINITY;
        u[c] = -INFINITY;
      }
      mu = fmax(mu, u[c]);
      ma = fmax(ma, a[c]);
    }
    mu = wave_max(mu);
    ma = wave_max(ma);
    double su = 0.0, sa = 0.0;
#pragma unroll
    for (int c = 0; c < KPL; ++c) {
      u[c] = exp(u[c] - mu);
      su += u[c];
      sa += exp(a[c] - ma);
    }
    su = wave_sum(su);
    sa = wave_sum(sa);
#pragma unroll
    for (int c = 0; c < KPL; ++c) {
      const int k = lane + 64 * c;
      if (k < K) q[qbase + k] = u[c] / su;
    }
    if (lane == 0) row_lse[srow] = ma + log(sa);
  }
}

// local_lb of the sequences in `order`: grid (sequences), block 64
__global__ __launch_bounds__(64) void k_seq_lb(const double* __restrict__ row_lse, int64_t row_base,
                                               const int64_t* __restrict__ seq_off,
                                               const int32_t* __restrict__ order, double* __restrict__ seq_lb) {
  const int s = order[blockIdx.x], lane = threadIdx.x;
  const int64_t r0 = seq_off[s];
  const int len = (int)(seq_off[s + 1] - r0);
  const double* __restrict__ r = row_lse + (size_t)(r0 - row_base);
  double acc = 0.0;
  for (int t = lane; t < len; t += 64) acc += r[t];
  acc = wave_sum(acc);
  if (lane == 0) seq_lb[s] = acc;
}

// Boundary correction of A_raw (see the head of this file) and q0.  grid (ceil(K * K / 256) + 1), block 256:
// the last workgroup forms q0.
__global__ __launch_bounds__(256) void k_seq_fix(const double* __restrict__ q, const int64_t* __restrict__ seq_off,
                                                 int N, int K, int wrap, double* __restrict__ A_raw,
                                                 double* __restrict__ q0) {
  if (blockIdx.x == gridDim.x - 1) {
    const int k = threadIdx.x;
    if (k < K) {
      double acc = 0.0;
      for (int s = 0; s < N; ++s) acc += q[(size_t)seq_off[s] * K + k];
      q0[k] = acc;
    }
    return;
  }
  const int e = blockIdx.x * 256 + threadIdx.x;
  if (e >= K * K) return;
  const int i = e / K, j = e - i * K;
  double acc = A_raw[e];
  for (int s = 0; s < N; ++s) {
    const double ql = q[(size_t)(seq_off[s + 1] - 1) * K + i];
    if (s + 1 < N) acc -= ql * q[(size_t)seq_off[s + 1] * K + j];
    if (wrap) acc += ql * q[(size_t)seq_off[s] * K + j];
  }
  A_raw[e] = acc;
}

// svihmm_estep_sequence_subset's gather.  grid (M occurrences, segments), block 256: occurrence m is rows
// [src_off[m], src_off[m] + len) of the resident copy, len = dst_off[m + 1] - dst_off[m], and becomes rows
// [dst_off[m], dst_off[m + 1]) of the compact one.  A sequence's rows are one contiguous run of len * D doubles on
// both sides; they travel as 64-bit words (a NaN keeps its payload), two per lane where source and destination
// share their 16-byte phase, dealt round-robin to the gridDim.y workgroups that serve the occurrence.  64-bit
// element offsets throughout.  mask / mask_out may be NULL (no mask resident).
__global__ __launch_bounds__(256) void k_seq_gather(
    const unsigned long long* __restrict__ obs, const uint8_t* __restrict__ mask,
    const int64_t* __restrict__ dst_off, const int64_t* __restrict__ src_off, int D,
    unsigned long long* __restrict__ obs_out, uint8_t* __restrict__ mask_out) {
  const int m = blockIdx.x;
  const int64_t d0 = dst_off[m], len = dst_off[m + 1] - d0, s0 = src_off[m];
  const int64_t n = len * (int64_t)D;
  const int64_t tid = (int64_t)blockIdx.y * 256 + threadIdx.x, nthr = (int64_t)gridDim.y * 256;
  const unsigned long long* __restrict__ src = obs + s0 * (int64_t)D;
  unsigned long long* __restrict__ dst = obs_out + d0 * (int64_t)D;
  if ((((s0 ^ d0) * (int64_t)D) & 1) == 0) {
    // the same phase: one leading word where the runs start on an odd element, then pairs, then the odd tail
    const int64_t lead = (s0 * (int64_t)D) & 1;
    const int64_t n2 = (n - lead) >> 1;
    const ulonglong2* __restrict__ s2 = reinterpret_cast<const ulonglong2*>(src + lead);
    ulonglong2* __restrict__ d2 = reinterpret_cast<ulonglong2*>(dst + lead);
    int64_t i = tid;
    for (; i + 3 * nthr < n2; i += 4 * nthr) {
      const ulonglong2 a = s2[i], b = s2[i + nthr], c = s2[i + 2 * nthr], d = s2[i + 3 * nthr];
      d2[i] = a; d2[i + nthr] = b; d2[i + 2 * nthr] = c; d2[i + 3 * nthr] = d;
    }
    for (; i < n2; i += nthr) d2[i] = s2[i];
    if (tid == 0) {
      if (lead) dst[0] = src[0];
      if ((n - lead) & 1) dst[n - 1] = src[n - 1];
    }
  } else {
    for (int64_t i = tid; i < n; i += nthr) dst[i] = src[i];
  }
  if (mask != nullptr)
    for (int64_t i = tid; i < len; i += nthr) mask_out[d0 + i] = mask[s0 + i];
}
