// kernels_grow.h -- growing adaptive windows / buffers on the device (svihmm_grow_windows).
// Part of libsvihmm_hip.so; compiled in tu_recursion.hip.
//
// The candidates of a centre c are nested windows [c - b, c + b].  With G_t = A diag(e_t), A = exp(ltran),
// e_t = exp(ll_t - max_k ll_t) and m the probe offset, the posterior of the two probe rows c - m, c + m is
//     q_left  ~ alpha (.) (Mid beta)        q_right ~ (alpha Mid) (.) beta
//     alpha = v' F_b,  beta = R_b 1,  v = exp(mod_init + ll_s) (s = c - b, any scale)
//     F_b = G_{s+1} ... G_{c-m}    grows on the left:   F_{b+1} = G_s F_b
//     R_b = G_{c+m+1} ... G_{c+b}  grows on the right:  R_{b+1} = R_b G_{c+b+1}
//     Mid = G_{c-m+1} ... G_{c+m}  built once: its halves G_{c-m+1} .. G_c and G_{c+1} .. G_{c+m} grow side by side
//           in the buffers of F and R (m products each), one more product joins them
// Only normalised q is used, so every matrix carries a free scale: a power of two taken from the largest entry
// the matrix had one product earlier (exact; entries of G are <= 1, so a product never grows past that scale).
//
// k_grow_products<NT>: one workgroup of 8 waves per centre, K <= KP = 16 NT.  Waves 0-3 own the left products
// (X <- A (diag(e) X): wave w the 16 columns w of X), waves 4-7 the right products (X <- (X A) diag(e): wave w the
// 16 rows w - 4 of X); a wave reads its whole block of X into registers before it writes it back, so a product needs
// no barrier inside.  Operand layout of v_mfma_f64_16x16x4_f64: A operand lane l -> [i = l & 15][k = l >> 4], B operand
// [k = l >> 4][j = l & 15], C register r -> [row = (l >> 4) + 4 r][col = l & 15].
// LDS: F, R, Mid and A, KP rows of KP + 4 doubles each (A-operand reads of 16 rows x 4 columns then touch every bank
// pair twice, the minimum for 64 lanes x 8 bytes), 4 x 34 KB at K = 64.  The probe vectors are O(K^2) on the VALU:
// wave 0 carries the alpha chain, wave 4 the beta chain, vectors pass between lanes by shuffles.  Residuals and the
// stop decision are taken from LDS values every thread reads alike: the loop is uniform across the workgroup, its trip
// count is bounded by smax[c] (the steps the sequence ends and the cutoff allow, computed by the host), and nothing
// depends on another workgroup -- a centre's result is the same whatever the batch.
#pragma once
#include <cfloat>

#define GROW_THREADS 512
__host__ __device__ constexpr int grow_ld(int NT) { return 16 * NT + 4; }
__host__ __device__ constexpr size_t grow_lds_bytes(int NT) {
  return ((size_t)4 * 16 * NT * grow_ld(NT) + 4 * 64 + 16 + 2) * sizeof(double);
}

// X <- sc * A (diag(e) X) for the 16 columns `blk` of X (left product, waves 0-3), e from the lliks row llr;
// returns the lane's largest new entry
template <int NT>
__device__ __forceinline__ double grow_mult_left(double* __restrict__ X, const double* __restrict__ Al,
                                                 const double* __restrict__ llr, int K, int blk, int li, int lk,
                                                 double sc) {
  constexpr int LD = grow_ld(NT);
  double bf[4 * NT];
  double mx = -INFINITY;
#pragma unroll
  for (int kk = 0; kk < 4 * NT; ++kk) {
    const int k = 4 * kk + lk;
    bf[kk] = k < K ? llr[k] : -INFINITY;
    mx = fmax(mx, bf[kk]);
  }
  mx = fmax(mx, __shfl_xor(mx, 16, 64));
  mx = fmax(mx, __shfl_xor(mx, 32, 64));
#pragma unroll
  for (int kk = 0; kk < 4 * NT; ++kk) {
    const int k = 4 * kk + lk;
    const double e = k < K ? exp(bf[kk] - mx) : 0.0;
    bf[kk] = X[k * LD + 16 * blk + li] * e;
  }
  double4_t acc[NT];
#pragma unroll
  for (int I = 0; I < NT; ++I) acc[I] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 4 * NT; ++kk)
#pragma unroll
    for (int I = 0; I < NT; ++I)
      acc[I] = __builtin_amdgcn_mfma_f64_16x16x4f64(Al[(16 * I + li) * LD + 4 * kk + lk], bf[kk], acc[I], 0, 0, 0);
  double lm = 0.0;
#pragma unroll
  for (int I = 0; I < NT; ++I)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = acc[I][r] * sc;
      X[(16 * I + lk + 4 * r) * LD + 16 * blk + li] = v;
      lm = fmax(lm, v);
    }
  return lm;
}

// OUT <- (X Bm) diag(ej) for the 16 rows `blk` (waves 4-7): the right product with Bm = A, OUT = X, and the product
// that joins the halves of Mid (ej = 1).  ej[J] belongs to column 16 J + li.
template <int NT>
__device__ __forceinline__ double grow_mult_rows(const double* X, const double* Bm, double* OUT, const double (&ej)[NT],
                                                 int blk, int li, int lk) {
  constexpr int LD = grow_ld(NT);
  double af[4 * NT];
#pragma unroll
  for (int kk = 0; kk < 4 * NT; ++kk) af[kk] = X[(16 * blk + li) * LD + 4 * kk + lk];
  double4_t acc[NT];
#pragma unroll
  for (int J = 0; J < NT; ++J) acc[J] = (double4_t){0.0, 0.0, 0.0, 0.0};
#pragma unroll
  for (int kk = 0; kk < 4 * NT; ++kk)
#pragma unroll
    for (int J = 0; J < NT; ++J)
      acc[J] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[kk], Bm[(4 * kk + lk) * LD + 16 * J + li], acc[J], 0, 0, 0);
  double lm = 0.0;
#pragma unroll
  for (int J = 0; J < NT; ++J)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const double v = acc[J][r] * ej[J];
      OUT[(16 * blk + lk + 4 * r) * LD + 16 * J + li] = v;
      lm = fmax(lm, v);
    }
  return lm;
}
// X <- sc * (X A) diag(e), e from the lliks row llr
template <int NT>
__device__ __forceinline__ double grow_mult_right(double* __restrict__ X, const double* __restrict__ Al,
                                                  const double* __restrict__ llr, int K, int blk, int li, int lk,
                                                  double sc) {
  double ej[NT];
  double mx = -INFINITY;
#pragma unroll
  for (int J = 0; J < NT; ++J) {
    const int j = 16 * J + li;
    ej[J] = j < K ? llr[j] : -INFINITY;
    mx = fmax(mx, ej[J]);
  }
#pragma unroll
  for (int o = 8; o >= 1; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 64));
#pragma unroll
  for (int J = 0; J < NT; ++J) ej[J] = (16 * J + li < K ? exp(ej[J] - mx) : 0.0) * sc;
  return grow_mult_rows<NT>(X, Al, X, ej, blk, li, lk);
}

// out[lane] = sum_i x[i] M[i][lane] (x held one entry per lane), lanes >= KP return 0
template <int NT>
__device__ __forceinline__ double grow_vec_mat(const double* __restrict__ M, double x, int lane) {
  constexpr int KP = 16 * NT, LD = grow_ld(NT);
  const int j = lane < KP ? lane : 0;
  double acc = 0.0;
  for (int i = 0; i < KP; ++i) acc = fma(__shfl(x, i, 64), M[i * LD + j], acc);
  return lane < KP ? acc : 0.0;
}
// out[lane] = sum_j M[lane][j] x[j]; lane i starts at column i (the row reads of all lanes then spread over the
// banks); ONES: x = 1 (row sums)
template <int NT, bool ONES>
__device__ __forceinline__ double grow_mat_vec(const double* __restrict__ M, double x, int lane) {
  constexpr int KP = 16 * NT, LD = grow_ld(NT);
  const int i = lane < KP ? lane : 0;
  double acc = 0.0;
  int j = i;
  for (int s = 0; s < KP; ++s) {
    const double xv = ONES ? 1.0 : __shfl(x, j, 64);
    acc = fma(M[i * LD + j], xv, acc);
    j = j + 1 == KP ? 0 : j + 1;
  }
  return lane < KP ? acc : 0.0;
}

template <int NT>
__global__ __launch_bounds__(GROW_THREADS) void k_grow_products(
    const double* __restrict__ ll, const double* __restrict__ Aexp, const double* __restrict__ mod_init,
    const int32_t* __restrict__ off, const int32_t* __restrict__ smax, int W, int K, int half0, int m, int inc,
    double eps, int rule, int32_t* __restrict__ out_half, int32_t* __restrict__ out_steps,
    double* __restrict__ trace, int trace_cap) {
  constexpr int KP = 16 * NT, LD = grow_ld(NT), MS = KP * LD;
  extern __shared__ double grow_sm[];
  double* F = grow_sm;
  double* R = F + MS;
  double* Mid = R + MS;
  double* Al = Mid + MS;       // A = exp(ltran), zero beyond K
  double* xa = Al + MS;        // alpha | w = alpha Mid | beta | u = Mid beta, 64 each
  double* xw = xa + 64;
  double* xb = xw + 64;
  double* xu = xb + 64;
  double* mxs = xu + 64;       // [2][8]: largest entry of each wave's block, double-buffered over the products
  double* dres = mxs + 16;     // d_left, d_right
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, role = wave >> 2, blk = wave & 3;
  const int li = lane & 15, lk = lane >> 4;
  const int c = blockIdx.x;
  const double* llc = ll + (size_t)c * W * K;
  const int o = off[c];
  const bool worker = blk < NT;

  auto identity = [&](double* X0, double* X1) {
    for (int idx = tid; idx < MS; idx += GROW_THREADS) {
      const int i = idx / LD, j = idx - i * LD;
      const double v = (i == j && i < K) ? 1.0 : 0.0;
      X0[idx] = v; X1[idx] = v;
    }
  };
  for (int idx = tid; idx < MS; idx += GROW_THREADS) {
    const int i = idx / LD, j = idx - i * LD;
    Al[idx] = (i < K && j < K) ? Aexp[i * K + j] : 0.0;
  }
  identity(F, R);
  __syncthreads();

  int par = 0;
  double sc = 1.0;
  // `cnt` rows onto (F on the left, R on the right) of the window of half-width b0 around local row o
  auto grow = [&](int b0, int cnt) {
    for (int t = 0; t < cnt; ++t) {
      if (worker) {
        const size_t row = role == 0 ? (size_t)(o - b0 - t) : (size_t)(o + b0 + 1 + t);
        double lm = role == 0 ? grow_mult_left<NT>(F, Al, llc + row * K, K, blk, li, lk, sc)
                              : grow_mult_right<NT>(R, Al, llc + row * K, K, blk, li, lk, sc);
        lm = wave_max(lm);
        if (lane == 0) mxs[par * 8 + wave] = lm;
      }
      __syncthreads();
      double mx = 0.0;
#pragma unroll
      for (int q = 0; q < NT; ++q) mx = fmax(mx, mxs[par * 8 + role * 4 + q]);
      sc = (mx > 0.0 && mx < INFINITY) ? ldexp(1.0, -ilogb(mx)) : 1.0;
      par ^= 1;
    }
  };
  // probe marginals of half-width b; residuals against the previous ones -> dres (when have_old)
  double qold = 0.0;   // wave 0: q_left[lane], wave 4: q_right[lane]
  auto probe = [&](int b, bool have_old) {
    if (wave == 0) {
      const double x = lane < K ? mod_init[lane] + llc[(size_t)(o - b) * K + lane] : -INFINITY;
      const double mx = wave_max(x);
      const double v = lane < K ? exp(x - mx) : 0.0;
      const double al = grow_vec_mat<NT>(F, v, lane);
      xa[lane] = al;
      xw[lane] = m > 0 ? grow_vec_mat<NT>(Mid, al, lane) : al;
    } else if (wave == 4) {
      const double be = grow_mat_vec<NT, true>(R, 0.0, lane);
      xb[lane] = be;
      xu[lane] = m > 0 ? grow_mat_vec<NT, false>(Mid, be, lane) : be;
    }
    __syncthreads();
    if (wave == 0 || wave == 4) {
      double q = wave == 0 ? xa[lane] * xu[lane] : xw[lane] * xb[lane];
      if (lane >= K) q = 0.0;
      q = q / wave_sum(q);
      if (have_old) {
        const double d = wave_sum(fabs(q - qold));
        if (lane == 0) dres[wave >> 2] = d;
      }
      qold = q;
    }
    __syncthreads();
  };

  if (m > 0) {
    // the halves of Mid in the buffers of F and R: G_{c-m+1} .. G_c (rows c, c - 1, ..) and G_{c+1} .. G_{c+m}
    grow(0, m);
    if (role == 1 && worker) {
      double one[NT];
#pragma unroll
      for (int J = 0; J < NT; ++J) one[J] = 1.0;
      grow_mult_rows<NT>(F, R, Mid, one, blk, li, lk);
    }
    __syncthreads();
    identity(F, R);
    __syncthreads();
    sc = 1.0;
  }
  grow(m, half0 - m);
  probe(half0, false);

  int b = half0, steps = 0, count = 0;
  double dl = DBL_MAX, dr = DBL_MAX, runl = 0.0, runr = 0.0, oldl = 0.0, oldr = 0.0;
  const int nmax = smax[c];
  for (int s = 0; s < nmax; ++s) {
    if (rule == 0) {
      if (dl < eps && dr < eps) break;
    } else {
      ++count;
      if (count > 1 && (runl - oldl) / (count - 1) < eps && (runr - oldr) / (count - 1) < eps) break;
    }
    grow(b, inc);
    b += inc;
    probe(b, true);
    dl = dres[0]; dr = dres[1];
    oldl = runl; oldr = runr;
    runl += dl; runr += dr;
    if (tid == 0 && trace && s < trace_cap) {
      trace[((size_t)c * trace_cap + s) * 2] = dl;
      trace[((size_t)c * trace_cap + s) * 2 + 1] = dr;
    }
    ++steps;
  }
  if (tid == 0) { out_half[c] = b; out_steps[c] = steps; }
  if (trace)
    for (int s = steps + (tid >> 1); s < trace_cap; s += GROW_THREADS / 2)
      trace[((size_t)c * trace_cap + s) * 2 + (tid & 1)] = NAN;
}

// The literal route's per-candidate kernel: the posteriors q [nact][Lm][K] of the candidate half-width b (window j
// belongs to centre idx[j]) -> the two probe rows, their residuals against the centre's previous probes, the rule's
// per-centre state and the decision whether the centre grows again.  One wave per active window.
//   qold [n][2][K];  st [n][6] = d_l d_r run_l run_r old_l old_r;  ist [n][3] = b, steps, count
__global__ __launch_bounds__(64) void k_grow_probe(
    const double* __restrict__ q, int Lm, int K, int b, int m, const int32_t* __restrict__ idx, int first,
    const int64_t* __restrict__ centers, int64_t T, int inc, int cutoff, double eps, int rule,
    double* __restrict__ qold, double* __restrict__ st, int32_t* __restrict__ ist, int32_t* __restrict__ active,
    double* __restrict__ trace, int trace_cap) {
  const int j = blockIdx.x, lane = threadIdx.x;
  const int i = idx[j];
  const double* ql = q + ((size_t)j * Lm + (b - m)) * K;
  const double* qr = q + ((size_t)j * Lm + (b + m)) * K;
  double* ol = qold + (size_t)i * 2 * K;
  double* orr = ol + K;
  double dl = 0.0, dr = 0.0;
  for (int k = lane; k < K; k += 64) {
    const double a = ql[k], r = qr[k];
    dl += fabs(a - ol[k]);
    dr += fabs(r - orr[k]);
    ol[k] = a; orr[k] = r;
  }
  dl = wave_sum(dl);
  dr = wave_sum(dr);
  if (lane != 0) return;
  double* s = st + (size_t)i * 6;
  int32_t* is = ist + (size_t)i * 3;
  if (!first) {
    s[0] = dl; s[1] = dr;
    s[4] = s[2]; s[5] = s[3];
    s[2] += dl; s[3] += dr;
    if (trace && is[1] < trace_cap) {
      trace[((size_t)i * trace_cap + is[1]) * 2] = dl;
      trace[((size_t)i * trace_cap + is[1]) * 2 + 1] = dr;
    }
    is[1] += 1;
  }
  is[0] = b;
  // the head of the rule's loop for this centre
  const int64_t c = centers[i];
  bool stop = c - b < 1 + (int64_t)inc || c + b + inc + 1 > T || b > cutoff;
  if (!stop) {
    if (rule == 0) stop = s[0] < eps && s[1] < eps;
    else {
      is[2] += 1;
      const int cnt = is[2];
      stop = cnt > 1 && (s[2] - s[4]) / (cnt - 1) < eps && (s[3] - s[5]) / (cnt - 1) < eps;
    }
  }
  active[i] = stop ? 0 : 1;
}
