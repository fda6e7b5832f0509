// kernels_viterbi.h -- Viterbi / MAP state paths (svihmm_viterbi): the max-plus forward recursion and its
// backtrack.  Included by tu_recursion.hip after kernels_recursion.h (the long-window backtrack reuses
// k_ffbs_compose).
//
//   delta[0][j] = mod_init[j] + ll[0][j]
//   delta[t][j] = max_i (delta[t-1][i] + ltran[i][j]) + ll[t][j]      psi[t][j] = the first maximising i
//   z[Lm-1] = first argmax_j delta[Lm-1][j];  z[t-1] = psi[t][z[t]];  score = max_j delta[Lm-1][j]
//
// Operation order (part of the contract, include/svihmm.h): one add per (i, j), a strict `>` scan over i
// in ascending order (the lowest index wins ties, an all -inf column keeps predecessor 0), one add of ll.
// No multiplication, hence nothing for the compiler to contract: delta, score and the path are bit-identical
// to the same three steps written in NumPy.  (max,+) has no matrix instruction: everything here is fp64 VALU.
//
// LDS budget: a workgroup claims at most VIT_LDS_BUDGET = 64 KiB (what a launch gets without raising the
// function's dynamic-LDS attribute; two such workgroups still share a CU's 160 KiB).  Two delta rows of KS
// doubles come off the top, the rest holds psi at KS bytes per row (KS = 64 for K <= 64, 256 above):
//   vit_lds_rows(64) = 1008, vit_lds_rows(256) = 240.
// Windows up to that length keep psi in LDS and backtrack inside the forward launch; longer windows write
// psi to HBM and are backtracked in chunks of the same length (k_vit_paths stages one chunk of psi in LDS).
//
// ONE body serves svihmm_viterbi (windows of equal length) and svihmm_viterbi_sequences (declared sequences of
// unequal length): the kernels take a `Units` policy by value that says where unit u of the launch finds its rows
// (VitWindows / VitSequences below).  The policy is a template parameter: nothing about the caller is decided at
// run time, and the step, the tie rule and the chase exist once per width.
#pragma once

#define VIT_LDS_BUDGET 65536
__host__ __device__ constexpr int vit_lds_rows(int KS) { return (VIT_LDS_BUDGET - 2 * KS * 8) / KS; }

// What a unit of work (one workgroup of a forward launch) decodes: `len` rows of ll from row0 on, z back to the same
// rows; psi at padded rows prow + t when it goes to HBM; the score into score[si].  zlast is indexed by the unit.
struct VitUnit { size_t row0; int len; size_t prow; int si; };

// B windows of Lm rows each, window u at rows u * Lm; padded to Lpad = Cw * Ls rows each for the chunked backtrack
struct VitWindows {
  int Lm;
  int64_t Lpad;
  template <bool LDSBT>
  __device__ __forceinline__ VitUnit unit(int u) const {
    return {(size_t)u * Lm, Lm, (size_t)u * Lpad, u};
  }
  // chunk c of the padded run = chunk cw of window u
  __device__ __forceinline__ void chunk(int c, int Ls, int& u, int& cw) const {
    const int Cw = (Lm + Ls - 1) / Ls;
    u = c / Cw;
    cw = c - u * Cw;
  }
};

// The resident rows as N chains laid end to end (seq_off[N + 1]).  Unit u is sequence order[u] (longest first), so a
// sequence's result never depends on what else is declared or where it lies.  Long sequences share ONE padded run of
// chunks: pad_off[u] = prefix sum of Cw * Ls over the launch's units (read only when psi goes to HBM), and the chunk
// table ctab[c] = (u, cw) finds a chunk's sequence.  score[s] and zlast[u] are written by the unit that owns s.
struct VitSequences {
  const int64_t* __restrict__ seq_off;
  const int32_t* __restrict__ order;
  const int64_t* __restrict__ pad_off;
  const int32_t* __restrict__ ctab;
  template <bool LDSBT>
  __device__ __forceinline__ VitUnit unit(int u) const {
    const int s = order[u];
    const int64_t r0 = seq_off[s];
    return {(size_t)r0, (int)(seq_off[s + 1] - r0), LDSBT ? 0 : (size_t)pad_off[u], s};
  }
  __device__ __forceinline__ void chunk(int c, int, int& u, int& cw) const {
    u = ctab[2 * c];
    cw = ctab[2 * c + 1];
  }
};

// ------------------------------------------------------------------------------------
//  V1: forward max-plus sweep, K <= 64: one wave per unit, lane = destination state j, column j of
//  ltran in registers, the delta row exchanged through a double-buffered LDS row (one wave: LDS
//  operations retire in order, a wave barrier keeps the compiler from reordering them).  The ll rows
//  are not on the dependent chain: they are loaded U steps ahead.
//  LDSBT: psi stays in LDS, the backtrack runs at the end of the launch and only z is written.
//  Otherwise psi goes to HBM (rows of 64 bytes at padded row prow + t) with the final argmax in zlast.
//  The launch's dynamic LDS is sized by the longest unit it serves.
// ------------------------------------------------------------------------------------
template <int KMAX, bool LDSBT, class Units>
__global__ __launch_bounds__(64) void k_vit_wave(
    const double* __restrict__ ll, const double* __restrict__ ltran, const double* __restrict__ mod_init,
    Units units, int K, unsigned char* __restrict__ psi_g, int32_t* __restrict__ z,
    int32_t* __restrict__ zlast, double* __restrict__ score) {
  extern __shared__ __align__(16) unsigned char vit_sm[];
  double* drow = (double*)vit_sm;                    // [2][64]
  unsigned char* psiL = vit_sm + 2 * 64 * 8;         // [Lm][64] (LDSBT with z wanted)
  const int lane = threadIdx.x, b = blockIdx.x;
  const VitUnit w = units.template unit<LDSBT>(b);
  const int Lm = w.len;
  const bool vj = lane < K;
  const int jc = vj ? lane : 0;
  double lt[KMAX];
#pragma unroll
  for (int i = 0; i < KMAX; ++i) lt[i] = (i < K && vj) ? ltran[(size_t)i * K + jc] : -INFINITY;
  const double* __restrict__ lw = ll + w.row0 * K + jc;
  double d = vj ? mod_init[jc] + lw[0] : -INFINITY;
  drow[lane] = d;
  drow[64 + lane] = -INFINITY;
  __builtin_amdgcn_wave_barrier();
  constexpr int U = 8;
  double cur[U], nxt[U];
#pragma unroll
  for (int u = 0; u < U; ++u) { const int t = 1 + u < Lm ? 1 + u : Lm - 1; cur[u] = lw[(size_t)t * K]; }
  for (int t0 = 1; t0 < Lm; t0 += U) {
#pragma unroll
    for (int u = 0; u < U; ++u) { const int t = t0 + U + u < Lm ? t0 + U + u : Lm - 1; nxt[u] = lw[(size_t)t * K]; }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int t = t0 + u;
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
        d = vj ? best + cur[u] : -INFINITY;
        drow[(t & 1) * 64 + lane] = d;
        if (LDSBT) { if (z) psiL[(size_t)t * 64 + lane] = (unsigned char)arg; }
        else psi_g[(w.prow + t) * 64 + lane] = (unsigned char)arg;
        __builtin_amdgcn_wave_barrier();
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) cur[u] = nxt[u];
  }
  const double m = wave_max(d);                      // (lanes >= K hold -inf)
  const unsigned long long bal = __ballot(vj && d == m);
  const int zl = bal ? __ffsll((long long)bal) - 1 : 0;
  if (lane == 0 && score) score[w.si] = m;
  if (!LDSBT) {
    if (lane == 0) zlast[b] = zl;
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
  for (int t = lane; t < Lm; t += 64) z[w.row0 + t] = psiL[(size_t)t * 64];
}

// ------------------------------------------------------------------------------------
//  V2: forward max-plus sweep, 64 < K <= 256: one workgroup of 256 threads per unit, thread =
//  destination state, delta row double-buffered in LDS (one barrier per step), the transition column
//  streamed from L2 (coalesced over the threads, as k_ffbs_paths_wide reads it).  psi rows of 256 bytes.
// ------------------------------------------------------------------------------------
template <bool LDSBT, class Units>
__global__ __launch_bounds__(256) void k_vit_wide(
    const double* __restrict__ ll, const double* __restrict__ ltran, const double* __restrict__ mod_init,
    Units units, int K, unsigned char* __restrict__ psi_g, int32_t* __restrict__ z,
    int32_t* __restrict__ zlast, double* __restrict__ score) {
  extern __shared__ __align__(16) unsigned char vit_sm[];
  double* drow = (double*)vit_sm;                    // [2][256]
  unsigned char* psiL = vit_sm + 2 * 256 * 8;        // [Lm][256] (LDSBT with z wanted)
  const int tid = threadIdx.x, b = blockIdx.x;
  const VitUnit w = units.template unit<LDSBT>(b);
  const int Lm = w.len;
  const bool vj = tid < K;
  const int jc = vj ? tid : 0;
  const double* __restrict__ col = ltran + jc;       // ltran[i][j] = col[i * K]
  const double* __restrict__ lw = ll + w.row0 * K + jc;
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
    else psi_g[(w.prow + t) * 256 + tid] = (unsigned char)arg;
    __syncthreads();
  }
  if (tid == 0) {                                    // first maximum of the final row, then the chase
    const double* dl = drow + ((Lm - 1) & 1) * 256;
    double m = dl[0];
    int zc = 0;
    for (int j = 1; j < K; ++j) if (dl[j] > m) { m = dl[j]; zc = j; }
    if (score) score[w.si] = m;
    if (!LDSBT) zlast[b] = zc;
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
  for (int t = tid; t < Lm; t += 256) z[w.row0 + t] = psiL[(size_t)t * 256];
}

// ------------------------------------------------------------------------------------
//  V3: backtrack of long windows without a sequential pass (the FFBS scheme, K6b in kernels_recursion.h):
//  z[t-1] = psi[t][z[t]] is a composition of maps.  Every unit is cut into Cw chunks of Ls rows (the
//  last one ragged) and stored at padded rows prow + t, Cw * Ls of them, so that the chunks of all
//  units form one uniform sequence (Units::chunk maps a chunk of that run to its unit).
//    k_vit_paths: one workgroup of KS threads per chunk, thread = the chunk's entry state s (the state at
//      the first row of the next chunk); path[t][s] = the state at row t.  The chunk's psi rows are staged
//      in LDS once (coalesced), then every thread chases its own path there.  The last chunk of a window
//      starts from the argmax of the final delta for every entry: its map is constant, so
//    k_ffbs_compose, run unchanged over all the chunks, never carries anything across a unit's boundary;
//    k_vit_gather: z[b][t] = path[t][entry of t's chunk], int32, back in the unpadded order (a thread per row of
//      the windows; the ragged form, a workgroup per chunk, is k_vitseq_gather in kernels_decode_sequences.h).
// ------------------------------------------------------------------------------------
template <class Units>
__global__ __launch_bounds__(256) void k_vit_paths(
    const unsigned char* __restrict__ psi, const int32_t* __restrict__ zlast, Units units, int Ls, int KS, int K,
    unsigned char* __restrict__ path) {
  extern __shared__ __align__(16) unsigned char vit_ps[];     // [Ls][KS]: row r = psi row lo + 1 + r
  const int tid = threadIdx.x;
  int b, cw;
  units.chunk(blockIdx.x, Ls, b, cw);
  const VitUnit w = units.template unit<false>(b);
  const int Lm = w.len, Cw = (Lm + Ls - 1) / Ls;
  const int lo = cw * Ls;
  const bool last = cw == Cw - 1;
  const int hi = last ? Lm : lo + Ls;                          // the chunk's rows: lo .. hi - 1
  const int nst = (last ? Lm - 1 : hi) - lo;                   // psi rows lo + 1 .. lo + nst
  const size_t row0 = w.prow + lo;
  const unsigned char* __restrict__ src = psi + (row0 + 1) * KS;
  const int nvec = nst * (KS / 16);
  for (int e = tid; e < nvec; e += KS) ((uint4*)vit_ps)[e] = ((const uint4*)src)[e];
  __syncthreads();
  int cur = tid < K ? tid : 0;
  cur = last ? zlast[b] : vit_ps[(size_t)(Ls - 1) * KS + cur];  // state at row hi - 1
  path[(row0 + (hi - 1 - lo)) * KS + tid] = (unsigned char)cur;
  for (int r = hi - 2 - lo; r >= 0; --r) {                     // state at row lo + r = psi[lo + r + 1][state above]
    cur = vit_ps[(size_t)r * KS + cur];
    path[(row0 + r) * KS + tid] = (unsigned char)cur;
  }
}

__global__ __launch_bounds__(256) void k_vit_gather(
    const unsigned char* __restrict__ path, const unsigned char* __restrict__ entry, int Lm, int Ls, int Cw,
    int64_t Lpad, int KS, int64_t n, int32_t* __restrict__ z) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t b = i / Lm;
  const int t = (int)(i - b * Lm);
  z[i] = path[((size_t)b * Lpad + t) * KS + entry[b * Cw + t / Ls]];
}
