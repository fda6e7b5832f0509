// kernels_decode_sequences.h -- decoding all declared sequences in one call (svihmm_viterbi_sequences,
// svihmm_ffbs_sequences): the RAGGED forms of the window decoders.  Included by tu_recursion.hip after
// kernels_viterbi.h (vit_lds_rows, the step body restated here), kernels_ffbs_windows.h (ffw_uniform, FFW_ZT) and
// kernels_sequences.h (whose sweeps, launched with one direction, are the forward filter of the sampler).
//
// The resident rows are N chains laid end to end (seq_off[N + 1]); ll / lalpha are ONE [T][K] array addressed by the
// resident row.  The unit of work is a sequence taken from an `order` array (longest first, as k_seq_wave does), so a
// sequence's result never depends on what else is declared or where it lies.
//
// Viterbi.  k_vitseq_wave<16|32|64, LDSBT> / k_vitseq_wide<LDSBT> are k_vit_wave / k_vit_wide with rows addressed
// through seq_off instead of b * Lm: same add / compare / select order, ll rows prefetched eight steps ahead.
//   LDSBT: len <= vit_lds_rows(KS) (or no path wanted): psi in LDS, backtrack inside the launch, z at the resident rows.
//          The launch's dynamic LDS is sized by the longest sequence it serves.
//   else:  psi rows at padded rows pad_off[u] + t of ONE run shared by all long sequences (u = the unit's index in the
//          launch; pad_off = prefix sum of Cw * Ls): k_vitseq_paths / k_vitseq_gather find a chunk's sequence through
//          the chunk table ctab[c] = (u, cw), k_ffbs_compose runs unchanged over the run -- a sequence's last chunk
//          map is constant, so nothing is carried across a join.
//   score[s] and zlast[u] are written by the unit that owns s: no atomics, no reductions across units.
//
// FFBS.  k_ffbs_seq<KMAX> / k_ffbs_seq_wide: ONE LANE PER (sequence, draw) pair, p = rank(s) * S + draw with rank
// the longest-first order, so the lanes of a wave walk sequences of similar length.  Step i counts back from each
// lane's own last row; a lane idles once i >= len; the wave runs to the longest of its lanes (its first).  logA
// transposed in LDS and the z tile flush are k_ffbs_win's; the lalpha row of a step is read from L2 by the lane
// itself (not staged in LDS: lanes of one sequence broadcast, a row's K doubles are contiguous).
// The uniform of (draw, resident row r) is entry draw * T + r.
#pragma once

template <int KMAX, bool LDSBT>
__global__ __launch_bounds__(64) void k_vitseq_wave(
    const double* __restrict__ ll, const double* __restrict__ ltran, const double* __restrict__ mod_init,
    const int64_t* __restrict__ seq_off, const int32_t* __restrict__ order, const int64_t* __restrict__ pad_off,
    int K, unsigned char* __restrict__ psi_g, int32_t* __restrict__ z, int32_t* __restrict__ zlast,
    double* __restrict__ score) {
  extern __shared__ __align__(16) unsigned char vit_sm[];
  double* drow = (double*)vit_sm;                    // [2][64]
  unsigned char* psiL = vit_sm + 2 * 64 * 8;         // [Lm][64] (LDSBT with z wanted)
  const int lane = threadIdx.x, u = blockIdx.x, s = order[u];
  const int64_t r0 = seq_off[s];
  const int Lm = (int)(seq_off[s + 1] - r0);
  const size_t prow = LDSBT ? 0 : (size_t)pad_off[u];
  const bool vj = lane < K;
  const int jc = vj ? lane : 0;
  double lt[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) lt[i] = (i < K && vj) ? ltran[(size_t)i * K + jc] : -INFINITY;
  const double* __restrict__ lw = ll + (size_t)r0 * K + jc;
  double d = vj ? mod_init[jc] + lw[0] : -INFINITY;
  drow[lane] = d;
  drow[64 + lane] = -INFINITY;
  __builtin_amdgcn_wave_barrier();
  constexpr int U = 8;
  double cur[U], nxt[U];
#pragma unroll
  for (int q = 0; q < U; ++q) { const int t = 1 + q < Lm ? 1 + q : Lm - 1; cur[q] = lw[(size_t)t * K]; }
  for (int t0 = 1; t0 < Lm; t0 += U) {
#pragma unroll
    for (int q = 0; q < U; ++q) { const int t = t0 + U + q < Lm ? t0 + U + q : Lm - 1; nxt[q] = lw[(size_t)t * K]; }
#pragma unroll
    for (int q = 0; q < U; ++q) {
      const int t = t0 + q;
      if (t < Lm) {                                  // (uniform)
        const double* dp = drow + ((t - 1) & 1) * 64;
        double best = dp[0] + lt[0];
        int arg = 0;
#pragma unroll
        for (int i = 1; i < KMAX; ++i) {
          const double v = dp[i] + lt[i];
          const bool gt = v > best;
          best = gt ? v : best;
          arg = gt ? i : arg;
        }
        d = vj ? best + cur[q] : -INFINITY;
        drow[(t & 1) * 64 + lane] = d;
        if (LDSBT) { if (z) psiL[(size_t)t * 64 + lane] = (unsigned char)arg; }
        else psi_g[(prow + t) * 64 + lane] = (unsigned char)arg;
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int q = 0; q < U; ++q) cur[q] = nxt[q];
  }
  const double m = wave_max(d);                      // (lanes >= K hold -inf)
  const unsigned long long bal = __ballot(vj && d == m);
  const int zl = bal ? __ffsll((long long)bal) - 1 : 0;
  if (lane == 0 && score) score[s] = m;
  if (!LDSBT) {
    if (lane == 0) zlast[u] = zl;
    return;
  }
  if (!z) return;
  if (lane == 0) {                                   // chase psi in LDS; z[t] is parked in column 0 of row t
    int zc = zl;
    for (int t = Lm - 1; t >= 1; --t) {
      const int zp = psiL[(size_t)t * 64 + zc];
      psiL[(size_t)t * 64] = (unsigned char)zc;
      zc = zp;
    }
    psiL[0] = (unsigned char)zc;
  }
  __builtin_amdgcn_wave_barrier();
  for (int t = lane; t < Lm; t += 64) z[(size_t)r0 + t] = psiL[(size_t)t * 64];
}

template <bool LDSBT>
__global__ __launch_bounds__(256) void k_vitseq_wide(
    const double* __restrict__ ll, const double* __restrict__ ltran, const double* __restrict__ mod_init,
    const int64_t* __restrict__ seq_off, const int32_t* __restrict__ order, const int64_t* __restrict__ pad_off,
    int K, unsigned char* __restrict__ psi_g, int32_t* __restrict__ z, int32_t* __restrict__ zlast,
    double* __restrict__ score) {
  extern __shared__ __align__(16) unsigned char vit_sm[];
  double* drow = (double*)vit_sm;                    // [2][256]
  unsigned char* psiL = vit_sm + 2 * 256 * 8;        // [Lm][256] (LDSBT with z wanted)
  const int tid = threadIdx.x, u = blockIdx.x, s = order[u];
  const int64_t r0 = seq_off[s];
  const int Lm = (int)(seq_off[s + 1] - r0);
  const size_t prow = LDSBT ? 0 : (size_t)pad_off[u];
  const bool vj = tid < K;
  const int jc = vj ? tid : 0;
  const double* __restrict__ col = ltran + jc;       // ltran[i][j] = col[i * K]
  const double* __restrict__ lw = ll + (size_t)r0 * K + jc;
  double d = vj ? mod_init[jc] + lw[0] : -INFINITY;
  drow[tid] = d;
  double lnext = lw[(size_t)(1 < Lm ? 1 : Lm - 1) * K];
  __syncthreads();
  for (int t = 1; t < Lm; ++t) {
    const double lcur = lnext;
    lnext = lw[(size_t)(t + 1 < Lm ? t + 1 : Lm - 1) * K];
    const double* dp = drow + ((t - 1) & 1) * 256;
    double best = dp[0] + col[0];
    int arg = 0;
#pragma unroll 8
    for (int i = 1; i < K; ++i) {
      const double v = dp[i] + col[(size_t)i * K];
      const bool gt = v > best;
      best = gt ? v : best;
      arg = gt ? i : arg;
    }
    d = vj ? best + lcur : -INFINITY;
    drow[(t & 1) * 256 + tid] = d;
    if (LDSBT) { if (z) psiL[(size_t)t * 256 + tid] = (unsigned char)arg; }
    else psi_g[(prow + t) * 256 + tid] = (unsigned char)arg;
    __syncthreads();
  }
  if (tid == 0) {                                    // first maximum of the final row, then the chase
    const double* dl = drow + ((Lm - 1) & 1) * 256;
    double m = dl[0];
    int zc = 0;
    for (int j = 1; j < K; ++j) if (dl[j] > m) { m = dl[j]; zc = j; }
    if (score) score[s] = m;
    if (!LDSBT) zlast[u] = zc;
    else if (z) {
      for (int t = Lm - 1; t >= 1; --t) {
        const int zp = psiL[(size_t)t * 256 + zc];
        psiL[(size_t)t * 256] = (unsigned char)zc;
        zc = zp;
      }
      psiL[0] = (unsigned char)zc;
    }
  }
  if (!LDSBT || !z) return;
  __syncthreads();
  for (int t = tid; t < Lm; t += 256) z[(size_t)r0 + t] = psiL[(size_t)t * 256];
}

// k_vit_paths over the chunk run of the long sequences: chunk c = ctab[2 c] (unit u of the forward launch) and
// ctab[2 c + 1] (its index cw inside the sequence); the chunk's rows are padded rows pad_off[u] + cw * Ls ..
__global__ __launch_bounds__(256) void k_vitseq_paths(
    const unsigned char* __restrict__ psi, const int32_t* __restrict__ zlast, const int64_t* __restrict__ seq_off,
    const int32_t* __restrict__ order, const int64_t* __restrict__ pad_off, const int32_t* __restrict__ ctab,
    int Ls, int KS, int K, unsigned char* __restrict__ path) {
  extern __shared__ __align__(16) unsigned char vit_ps[];     // [Ls][KS]: row r = psi row lo + 1 + r
  const int tid = threadIdx.x;
  const int c = blockIdx.x, u = ctab[2 * c], cw = ctab[2 * c + 1], s = order[u];
  const int Lm = (int)(seq_off[s + 1] - seq_off[s]);
  const int Cw = (Lm + Ls - 1) / Ls;
  const int lo = cw * Ls;
  const bool last = cw == Cw - 1;
  const int hi = last ? Lm : lo + Ls;                          // the chunk's rows: lo .. hi - 1
  const int nst = (last ? Lm - 1 : hi) - lo;                   // psi rows lo + 1 .. lo + nst
  const size_t row0 = (size_t)pad_off[u] + lo;
  const unsigned char* __restrict__ src = psi + (row0 + 1) * KS;
  const int nvec = nst * (KS / 16);
  for (int e = tid; e < nvec; e += KS) ((uint4*)vit_ps)[e] = ((const uint4*)src)[e];
  __syncthreads();
  int cur = tid < K ? tid : 0;
  cur = last ? zlast[u] : vit_ps[(size_t)(Ls - 1) * KS + cur];  // state at row hi - 1
  path[(row0 + (hi - 1 - lo)) * KS + tid] = (unsigned char)cur;
  for (int r = hi - 2 - lo; r >= 0; --r) {                     // state at row lo + r = psi[lo + r + 1][state above]
    cur = vit_ps[(size_t)r * KS + cur];
    path[(row0 + r) * KS + tid] = (unsigned char)cur;
  }
}

// one workgroup per chunk: z[resident row] = path[padded row][entry of the chunk]
__global__ __launch_bounds__(256) void k_vitseq_gather(
    const unsigned char* __restrict__ path, const unsigned char* __restrict__ entry,
    const int64_t* __restrict__ seq_off, const int32_t* __restrict__ order, const int64_t* __restrict__ pad_off,
    const int32_t* __restrict__ ctab, int Ls, int KS, int32_t* __restrict__ z) {
  const int c = blockIdx.x, u = ctab[2 * c], cw = ctab[2 * c + 1], s = order[u];
  const int64_t r0 = seq_off[s];
  const int Lm = (int)(seq_off[s + 1] - r0);
  const int lo = cw * Ls;
  const int n = Lm - lo < Ls ? Lm - lo : Ls;
  const size_t row0 = (size_t)pad_off[u] + lo;
  const int en = entry[c];
  for (int r = threadIdx.x; r < n; r += 256) z[(size_t)r0 + lo + r] = path[(row0 + r) * KS + en];
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
  for (int e = lane; e < K * K; e += 64) {
    const int k = e / K, sidx = e - k * K;
    lAT[sidx * (KMAX + 1) + k] = logA[e];
  }
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
        // the draw of k_ffbs_win, operation for operation
        double lp[KMAX], m = -INFINITY;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          lp[k] = (k < K ? rw[k] : -INFINITY) + ((first || k >= K) ? 0.0 : tr[k]);
          m = fmax(m, lp[k]);
        }
        double tot = 0.0;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) { lp[k] = k < K ? exp(lp[k] - m) : 0.0; tot += lp[k]; }
        const double thr = r * tot;
        double c = 0.0;
        int zz = K - 1;
        bool found = false;
#pragma unroll
        for (int k = 0; k < KMAX; ++k) {
          c += lp[k];
          const bool hit = !found && k < K && thr <= c;
          zz = hit ? k : zz;
          found = found || hit;
        }
        cur = zz;
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
        const double* __restrict__ col = logA + cur;             // logA[k][cur] = col[k * K]
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
        cur = zz;
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
