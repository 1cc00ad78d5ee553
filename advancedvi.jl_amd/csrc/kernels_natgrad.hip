// The natural-gradient (variational online Newton) update of KLMinNaturalGradDescent (src/algorithms/klminnaturalgraddescent.jl:129-145) and
// the state of its `init` (:83-87), on the device-resident [m; vec C] and [S; Sigma] (precision and covariance, d x d column-major, both
// triangles bitwise mirrored):
//     ensure_posdef:  Gh = S + H                    S' = Hermitian(S - eta Gh + eta^2/2 Gh Sigma Gh)                        (:129-130)
//     otherwise:                                    S' = Hermitian((1 - eta) S - eta H)                                     (:132)
//     S' = Lr' Lr (Lr lower: the Cholesky factorisation run from the bottom-right corner)     C' = Lr^-1     Sigma' = C' C''
//     m' = m - eta C' (C'' (-g))                    entropy(q') = d/2 (1 + log 2 pi) + sum_i log C'_ii                       (:134-145)
// Hermitian(.) reads the UPPER triangle of its operand and mirrors it (H is not symmetric on the Stein branch).  DEVIATION from the
// reference: its new scale is the upper-triangular adjoint of the inverse of a lower Cholesky factor of S'; this library's full-rank family
// stores a lower-triangular C with exact zeros above the diagonal, so the iterate is q' = (m', C') with C' = Lr^-1 the LOWER Cholesky factor
// of Sigma' = S'^-1 -- the same distribution and the same recursion in (m, S, Sigma); only the pairing of draws with samples differs.
// g and H are read-only, H is used as it comes.  No floating-point atomics, one summation order: an update is bitwise repeatable.  A pivot
// that is not a positive finite number sets the sticky flag and is replaced by 1, so nothing divides by zero and no loop depends on a NaN.
//
// d <= MIVI_NATGRAD_SMALL_D: ONE workgroup keeps S, Sigma, Gh (in H's place) and one work matrix in LDS and does the whole update in one
// launch (k_natgrad_small).  Above it: 64 x 64 tiles on the matrix cores (ngd_tile.h) on context-owned scratch padded to whole tiles
// (ld = 64 nT).  The tile path's scratch and arithmetic are FLOAT64 for either context type (v_mfma_f64_16x16x4_f64); an f32 context's g,
// H, parameters and state are converted where they are loaded and stored: a factorisation of S' rounded to float32 leaves C' up to
// kappa(S') x 6e-8 from the exact result whichever order the sums take, S' held in float64 until C' is stored does not.  The padded S'
// carries the identity on the diagonal of its padding so that it factors as diag(Lr, I) and nothing masks its
// operands except where it reads the caller's unpadded g, H, parameters and state:
//     prep      Gh = S + H and Sigma, padded (ensure_posdef)  |  the mirrored upper triangle of (1 - eta) S - eta H into A (otherwise)
//     gw, sp    W = Sigma Gh over all tiles; the upper tiles of S - eta Gh + eta^2/2 Gh W, mirrored into both triangles of A (ensure_posdef)
//     upd(k)    k = nT-1 .. 0: A_kj -= sum_{i > k} Lr_ik' Lr_ij for j <= k; the workgroup of the diagonal tile then factors it in LDS
//               (A_kk = Lr_kk' Lr_kk), inverts the factor, writes Dinv_k = Lr_kk^-1 and the panel's sum_i log C'_ii (C'_ii = 1 / Lr_ii)
//     scale(k)  k > 0: Lr_kj = Dinv_k' A_kj for j < k, a tile product
//     mk        M_ik = Dinv_i Lr_ik for k < i (into W);  X_ii = Dinv_i
//     inv(i)    i = 1 .. nT-1: X_ij = -sum_{k = j}^{i-1} M_ik X_kj for j < i          (X = Lr^-1 = C')
//     fin       the lower tiles of Sigma' = X X', mirrored, into the state; C' into the parameter vector (zeros above the diagonal); S' (the
//               upper tiles of A, which no phase overwrites) into the state; trailing workgroups: v = C'' (-g)
//     mean 1-4  x = C' v;  r = -g - S' x;  w = C'' r;  m' = m - eta (x + C' w) by 64-row blocks, all sums in float64: the solve S' x = -g
//               through the explicit inverse with ONE step of iterative refinement (the inverse alone leaves kappa(S') x unit roundoff
//               in x, which the one-workgroup kernel of an f32 context cannot afford); the last launch's first workgroup adds the panels' log sums in
//               order and writes entropy / elbo / flags.  The one-workgroup kernel forms m' the same way.
// 3 nT + 5 (+ 2) launches: 55 at d = 1024 with ensure_posdef.  The only ordering between workgroups is the order of the launches.
// The chunked tile product, the mean's column-dot and row-matvec bodies, the tile geometry and the finish (entropy / elbo / flags) are
// ngd_tile.h's, shared with kernels_ngd.hip, as is the context's scratch pair (ms_work, ms_part).
#include "mivi_internal.h"
#include "ngd_tile.h"

namespace mivi {

constexpr int kNatgradSmallD = MIVI_NATGRAD_SMALL_D;   // 4 matrices of 44 x 45 doubles = 63360 bytes of LDS (+ 1.8 KB of vectors)

// T: the type of the scratch and of the arithmetic; TI: the context's type, that of the caller's buffers
template <typename T, typename TI>
struct NatgradArgs {
  int d, nT, ldp, ensure, k;   // k: the panel (upd, scale) / block row (inv) of this launch
  int keep;                    // upd: the factored diagonal tile Lr_kk goes back into the lower triangle of A_kk (launch_natgrad_factor)
  TI *params;                  // [m (d); vec C (d x d, column-major)] in / out
  TI *state;                   // [S (d x d); Sigma (d x d)] in / out
  const TI *grad;              // g (d)
  const TI *hess;              // H (d x d, column-major)
  T *G, *P, *W, *A, *X;        // ldp x ldp each: Gh, Sigma, W = Sigma Gh (later M), the work matrix (S', then Lr in its lower tiles), X = Lr^-1
  T *Dinv;                     // nT tiles of 64 x 64 (column-major): Lr_kk^-1
  double *part;                // [2][nT]: sum log C'_ii of a panel, its count of bad pivots
  double *vec;                 // [4][ldp]: v = C'' (-g), x = C' v, r = -g - S' x, w = C'' r
  double eta;
  NgdOut<TI> out;              // entropy / elbo / flags (ngd_tile.h)
};

// ---- a triangle of at most 64 rows in LDS (row-major, leading dimension ld): 256 threads, all of them call these ---------------------------
// The lower triangle of s holds a symmetric A.  On return it holds Lr with A = Lr' Lr: column c = n-1 .. 0 takes its pivot, scales ROW c of
// Lr (Lr_cr = A_cr / Lr_cc, r < c) and takes Lr_cr Lr_cr' off the leading (c x c) triangle.  *sbad (LDS) is set on a bad pivot.
template <typename T>
__device__ __forceinline__ void natgrad_factor(T *s, int ld, int n, int *sbad) {
  const int tid = threadIdx.x, c2 = tid & 63, r2 = tid >> 6;
  for (int c = n - 1; c >= 0; --c) {
    __syncthreads();
    T p = s[c * ld + c];
    const bool bad = ngd_bad((double)p);
    if (bad) p = T(1);
    const T l = (T)sqrt(p);
    __syncthreads();
    if (tid < c) s[c * ld + tid] = s[c * ld + tid] / l;
    else if (tid == c) {
      s[c * ld + c] = l;
      if (bad) *sbad = 1;
    }
    __syncthreads();
    for (int r = r2; r < c; r += 4)
      if (c2 <= r) s[r * ld + c2] -= s[c * ld + r] * s[c * ld + c2];
  }
  __syncthreads();
}

// The lower triangle of s holds L (left as it is).  On return X = L^-1 sits transposed in the strict upper triangle, s[j][i] = X_ij (i > j),
// and its diagonal in sd[i] = 1 / L_ii.  Thread j owns column j of X: substitution down the column, no thread reads what another writes.
template <typename T>
__device__ __forceinline__ void natgrad_invert(T *s, int ld, int n, T *sd) {
  const int j = threadIdx.x;
  if (j < n) sd[j] = T(1) / s[j * ld + j];
  __syncthreads();
  if (j < n) {
    for (int i = j + 1; i < n; ++i) {
      T acc = s[i * ld + j] * sd[j];
      for (int k = j + 1; k < i; ++k) acc += s[i * ld + k] * s[j * ld + k];
      s[j * ld + i] = -acc * sd[i];
    }
  }
  __syncthreads();
}

// X_ij of the pair (s, sd) natgrad_invert leaves
template <typename T>
__device__ __forceinline__ T natgrad_x(const T *s, int ld, const T *sd, int i, int j) {
  return i > j ? s[j * ld + i] : (i == j ? sd[i] : T(0));
}

// ---- d <= kNatgradSmallD: one workgroup, everything in LDS ----------------------------------------------------------------------------------
// the lower triangle of X X' (TRANS: X' X) for a lower-triangular X in LDS (row-major), mirrored into both triangles of dst (d x d)
template <bool TRANS, typename T, typename TI>
__device__ __forceinline__ void natgrad_syrk_small(const T *X, int ld, int d, TI *dst) {
  for (int t = threadIdx.x; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    if (i < j) continue;
    T s = T(0);
    if (TRANS) for (int k = i; k < d; ++k) s += X[k * ld + i] * X[k * ld + j];
    else for (int k = 0; k <= j; ++k) s += X[i * ld + k] * X[j * ld + k];
    dst[(size_t)j * d + i] = s;
    dst[(size_t)i * d + j] = s;
  }
}

template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_small(NatgradArgs<T, TI> a) {
  constexpr int LD = kNatgradSmallD + 1, N = kNatgradSmallD * LD;
  __shared__ T sS[N], sP[N], sG[N], sW[N];
  __shared__ T sd[kNatgradSmallD];
  __shared__ double sv[kNatgradSmallD], sx[kNatgradSmallD], sr[kNatgradSmallD];
  __shared__ int sbad;
  const int d = a.d, tid = threadIdx.x;
  TI *Sg = a.state, *Pg = a.state + (size_t)d * d;
  const T eta = (T)a.eta;
  if (tid == 0) sbad = 0;
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    const T s = (T)Sg[t], h = (T)a.hess[t];
    sS[i * LD + j] = s;
    sP[i * LD + j] = Pg[t];
    sG[i * LD + j] = a.ensure ? s + h : h;
  }
  __syncthreads();
  if (a.ensure) {
    for (int t = tid; t < d * d; t += 256) {   // W = Sigma Gh
      const int i = t % d, j = t / d;
      T s = T(0);
      for (int k = 0; k < d; ++k) s += sP[i * LD + k] * sG[k * LD + j];
      sW[i * LD + j] = s;
    }
    __syncthreads();
  }
  // S': the upper triangle of the expression, mirrored (an element of the upper triangle reads no S but its own)
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    if (i > j) continue;
    T val;
    if (a.ensure) {
      T s = T(0);
      for (int k = 0; k < d; ++k) s += sG[i * LD + k] * sW[k * LD + j];
      val = (sS[i * LD + j] - eta * sG[i * LD + j]) + (eta * eta / T(2)) * s;
    } else {
      val = (T(1) - eta) * sS[i * LD + j] - eta * sG[i * LD + j];
    }
    sS[i * LD + j] = val;
    sS[j * LD + i] = val;
  }
  __syncthreads();
  for (int t = tid; t < d * d; t += 256) {   // (S' also stays in sG, for the residual of the mean's solve)
    const T s = sS[(t % d) * LD + t / d];
    Sg[t] = s;
    sG[(t % d) * LD + t / d] = s;
  }
  natgrad_factor(sS, LD, d, &sbad);
  natgrad_invert(sS, LD, d, sd);
  for (int t = tid; t < d * d; t += 256) {   // C' = X, plain in sW and into the parameter vector
    const int i = t % d, j = t / d;
    const T x = natgrad_x(sS, LD, sd, i, j);
    sW[i * LD + j] = x;
    a.params[d + t] = x;
  }
  __syncthreads();
  natgrad_syrk_small<false>(sW, LD, d, Pg);   // Sigma' = C' C''
  // m' = m - eta x, S' x = -g: x = C' (C'' (-g)), r = -g - S' x, x += C' (C'' r), sums in float64
  double x = 0.0;
  for (int pass = 0; pass < 2; ++pass) {
    if (tid < d) {
      double s = 0.0;
      if (pass == 0) {
        for (int k = tid; k < d; ++k) s += (double)sW[k * LD + tid] * (double)a.grad[k];
        sv[tid] = -s;
      } else {
        for (int k = tid; k < d; ++k) s += (double)sW[k * LD + tid] * sr[k];
        sv[tid] = s;
      }
    }
    __syncthreads();
    if (tid < d) {
      double s = 0.0;
      for (int j = 0; j <= tid; ++j) s += (double)sW[tid * LD + j] * sv[j];
      x += s;
      if (pass == 0) sx[tid] = x;
    }
    __syncthreads();
    if (pass == 0 && tid < d) {
      double s = 0.0;
      for (int j = 0; j < d; ++j) s += (double)sG[tid * LD + j] * sx[j];
      sr[tid] = -(double)a.grad[tid] - s;
    }
    __syncthreads();
  }
  if (tid < d) a.params[tid] = a.params[tid] - eta * (T)x;
  if (tid == 0) {
    double ls = 0.0;
    int bad = sbad;
    for (int i = 0; i < d; ++i) {
      ls += log((double)sd[i]);
      bad |= ngd_bad((double)sd[i]) ? 1 : 0;
    }
    ngd_finish(d, ls, bad, a.out);
  }
}

// init (:83-87) at d <= kNatgradSmallD: S = C^-T C^-1, Sigma = C C'
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_init_small(NatgradArgs<T, TI> a) {
  constexpr int LD = kNatgradSmallD + 1, N = kNatgradSmallD * LD;
  __shared__ T sC[N], sX[N];
  __shared__ T sd[kNatgradSmallD];
  const int d = a.d, tid = threadIdx.x;
  const TI *Cg = a.params + d;
  TI *Sg = a.state, *Pg = a.state + (size_t)d * d;
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    sC[i * LD + j] = i >= j ? Cg[t] : T(0);
  }
  __syncthreads();
  if (tid == 0) {
    int bad = 0;
    for (int i = 0; i < d; ++i) bad |= ngd_bad((double)sC[i * LD + i]) ? 1 : 0;
    if (bad) atomicOr(a.out.status, 2);
  }
  natgrad_syrk_small<false>(sC, LD, d, Pg);   // Sigma = C C'
  __syncthreads();
  natgrad_invert(sC, LD, d, sd);
  for (int t = tid; t < d * d; t += 256) sX[(t % d) * LD + t / d] = natgrad_x(sC, LD, sd, t % d, t / d);
  __syncthreads();
  natgrad_syrk_small<true>(sX, LD, d, Sg);   // S = X' X
}

// ---- the tile path (NgdFrag, ngd_product, NGD_WAVE, ngd_tile_of: ngd_tile.h) -------------------------------------------------------------------------

// prep, one workgroup per tile of the padded square.  MODE 0: the update's operands; MODE 1: init's A = tril(C), identity on the padding
template <typename T, typename TI, int MODE>
__global__ __launch_bounds__(256) void k_natgrad_prep(NatgradArgs<T, TI> a) {
  const int d = a.d, nT = a.nT, ldp = a.ldp, tid = threadIdx.x;
  const int i0 = ((int)blockIdx.x % nT) * kNgdTile, j0 = ((int)blockIdx.x / nT) * kNgdTile;
  const TI *Sg = a.state, *Pg = a.state + (size_t)d * d, *Cg = a.params + d;
  const T eta = (T)a.eta;
  for (int t = tid; t < kNgdTile * kNgdTile; t += 256) {
    const int i = i0 + (t & 63), j = j0 + (t >> 6);
    const bool in = i < d && j < d;
    const size_t o = (size_t)j * ldp + i;
    const T eye = i == j ? T(1) : T(0);
    if (MODE == 1) {
      a.A[o] = in ? (i >= j ? (T)Cg[(size_t)j * d + i] : T(0)) : eye;
    } else if (a.ensure) {
      a.G[o] = in ? (T)Sg[(size_t)j * d + i] + (T)a.hess[(size_t)j * d + i] : T(0);
      a.P[o] = in ? Pg[(size_t)j * d + i] : T(0);
    } else {
      const size_t u = i <= j ? (size_t)j * d + i : (size_t)i * d + j;   // the upper triangle's element, mirrored
      a.A[o] = in ? (T(1) - eta) * (T)Sg[u] - eta * (T)a.hess[u] : eye;
    }
  }
}

// W = Sigma Gh, every tile
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_gw(NatgradArgs<T, TI> a) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  const int nT = a.nT, ldp = a.ldp;
  const int i0 = ((int)blockIdx.x % nT) * kNgdTile, j0 = ((int)blockIdx.x / nT) * kNgdTile;
  NGD_WAVE;
  NgdFrag<T> acc;
  acc.zero();
  ngd_product<T, false, true>(acc, a.P + i0, ldp, a.G + (size_t)j0 * ldp, ldp, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) { a.W[(size_t)(j0 + jj) * ldp + i0 + ii] = x; });
}

// the upper tiles of S - eta Gh + eta^2/2 Gh W, mirrored into both triangles of A; the identity on the diagonal of the padding
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_sp(NatgradArgs<T, TI> a) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  const int d = a.d, ldp = a.ldp;
  int tc, tr;
  ngd_tile_of((int)blockIdx.x, tc, tr);   // tr <= tc: an upper tile
  const int i0 = tr * kNgdTile, j0 = tc * kNgdTile;
  NGD_WAVE;
  NgdFrag<T> acc;
  acc.zero();
  ngd_product<T, false, true>(acc, a.G + i0, ldp, a.W + (size_t)j0 * ldp, ldp, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
  const T eta = (T)a.eta, h = eta * eta / T(2);
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) {
    const int i = i0 + ii, j = j0 + jj;
    if (i > j) return;
    T val = i == j ? T(1) : T(0);
    if (i < d && j < d) val = ((T)a.state[(size_t)j * d + i] - eta * a.G[(size_t)j * ldp + i]) + h * x;
    a.A[(size_t)j * ldp + i] = val;
    a.A[(size_t)i * ldp + j] = val;
  });
}

// Dinv_k and the panel's log sum from the (updated) diagonal tile in sT (row-major, kNgdLd); FACTOR: sT holds A_kk, otherwise Lr_kk itself
template <typename T, typename TI, bool FACTOR>
__device__ __forceinline__ void natgrad_diag_tile(const NatgradArgs<T, TI> &a, int k, T *sT, T *sd, int *sbad) {
  const int tid = threadIdx.x;
  if (FACTOR) natgrad_factor(sT, kNgdLd, kNgdTile, sbad);
  natgrad_invert(sT, kNgdLd, kNgdTile, sd);
  T *Dk = a.Dinv + (size_t)k * kNgdTile * kNgdTile;
  for (int t = tid; t < kNgdTile * kNgdTile; t += 256) Dk[t] = natgrad_x(sT, kNgdLd, sd, t & 63, t >> 6);
  if (tid == 0) {
    const int n = a.d - k * kNgdTile < kNgdTile ? a.d - k * kNgdTile : kNgdTile;
    double ls = 0.0;
    int bad = *sbad;
    for (int r = 0; r < n; ++r) {
      ls += log((double)sd[r]);
      bad |= ngd_bad((double)sd[r]) ? 1 : 0;
    }
    a.part[k] = ls;
    a.part[a.nT + k] = (double)bad;
    if (bad) atomicOr(a.out.status, 2);
  }
}

// panel k: A_kj -= sum_{i > k} Lr_ik' Lr_ij (j <= k); the diagonal tile's workgroup factors and inverts it
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_upd(NatgradArgs<T, TI> a) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  __shared__ T sd[kNgdTile];
  __shared__ int sbad;
  const int ldp = a.ldp, k = a.k, j = (int)blockIdx.x;
  const int k0 = k * kNgdTile, j0 = j * kNgdTile;
  NGD_WAVE;
  if (threadIdx.x == 0) sbad = 0;
  NgdFrag<T> acc;
  acc.zero();
  ngd_product<T, true, true>(acc, a.A + (size_t)k0 * ldp, ldp, a.A + (size_t)j0 * ldp, ldp, k0 + kNgdTile, ldp, sAB, sAB + kNgdKC * kNgdLd);
  if (j < k) {
    acc.each(wr, wc, lane, [&](int ii, int jj, T x) { a.A[(size_t)(j0 + jj) * ldp + k0 + ii] -= x; });
    return;
  }
  __syncthreads();
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) { sAB[ii * kNgdLd + jj] = a.A[(size_t)(k0 + jj) * ldp + k0 + ii] - x; });
  natgrad_diag_tile<T, TI, true>(a, k, sAB, sd, &sbad);
  if (a.keep)   // (natgrad_invert leaves Lr_kk in the lower triangle of the tile)
    for (int t = threadIdx.x; t < kNgdTile * kNgdTile; t += 256)
      if ((t >> 6) <= (t & 63)) a.A[(size_t)(k0 + (t >> 6)) * ldp + k0 + (t & 63)] = sAB[(t & 63) * kNgdLd + (t >> 6)];
}

// init: Dinv_k = C_kk^-1 from the diagonal tiles of A = tril(C)
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_dinv(NatgradArgs<T, TI> a) {
  __shared__ T sT[kNgdTile * kNgdLd];
  __shared__ T sd[kNgdTile];
  __shared__ int sbad;
  const int ldp = a.ldp, k = (int)blockIdx.x, k0 = k * kNgdTile;
  if (threadIdx.x == 0) sbad = 0;
  for (int t = threadIdx.x; t < kNgdTile * kNgdTile; t += 256) sT[(t & 63) * kNgdLd + (t >> 6)] = a.A[(size_t)(k0 + (t >> 6)) * ldp + k0 + (t & 63)];
  __syncthreads();
  natgrad_diag_tile<T, TI, false>(a, k, sT, sd, &sbad);
}

// Lr_kj = Dinv_k' A_kj, j < k, in place (a workgroup has read its whole tile before it writes it)
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_scale(NatgradArgs<T, TI> a) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  const int ldp = a.ldp, k0 = a.k * kNgdTile, j0 = (int)blockIdx.x * kNgdTile;
  NGD_WAVE;
  NgdFrag<T> acc;
  acc.zero();
  T *tile = a.A + (size_t)j0 * ldp + k0;
  ngd_product<T, true, true>(acc, a.Dinv + (size_t)a.k * kNgdTile * kNgdTile, kNgdTile, tile, ldp, 0, kNgdTile, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) { tile[(size_t)jj * ldp + ii] = x; });
}

// M_ik = Dinv_i Lr_ik (k < i) into W; X_ii = Dinv_i
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_mk(NatgradArgs<T, TI> a) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  const int ldp = a.ldp;
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  const T *Di = a.Dinv + (size_t)ti * kNgdTile * kNgdTile;
  if (ti == tj) {
    for (int t = threadIdx.x; t < kNgdTile * kNgdTile; t += 256) a.X[(size_t)(i0 + (t >> 6)) * ldp + i0 + (t & 63)] = Di[t];
    return;
  }
  NGD_WAVE;
  NgdFrag<T> acc;
  acc.zero();
  ngd_product<T, false, true>(acc, Di, kNgdTile, a.A + (size_t)j0 * ldp + i0, ldp, 0, kNgdTile, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) { a.W[(size_t)(j0 + jj) * ldp + i0 + ii] = x; });
}

// block row i = a.k: X_ij = -sum_{k = j}^{i-1} M_ik X_kj, j < i
template <typename T, typename TI>
__global__ __launch_bounds__(256) void k_natgrad_inv(NatgradArgs<T, TI> a) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  const int ldp = a.ldp, i0 = a.k * kNgdTile, j0 = (int)blockIdx.x * kNgdTile;
  NGD_WAVE;
  NgdFrag<T> acc;
  acc.zero();
  ngd_product<T, false, true>(acc, a.W + i0, ldp, a.X + (size_t)j0 * ldp, ldp, j0, i0, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) { a.X[(size_t)(j0 + jj) * ldp + i0 + ii] = -x; });
}

// The lower tiles of src src' (TRANS: src' src) for a lower-triangular padded src, mirrored into the unpadded dst.  FIN (the update's last
// product, src = X, dst = Sigma'): the tile's workgroup also writes C' into the parameter vector and S' into the state; trailing workgroups
// form v = C'' (-g).
template <typename T, typename TI, bool TRANS, bool FIN>
__global__ __launch_bounds__(256) void k_natgrad_syrk(NatgradArgs<T, TI> a, const T *src, TI *dst) {
  __shared__ T sAB[2 * kNgdKC * kNgdLd];
  const int d = a.d, nT = a.nT, ldp = a.ldp, tid = threadIdx.x;
  const int n_tiles = ngd_n_tiles(nT);
  if (FIN && (int)blockIdx.x >= n_tiles) {   // v_j = -sum_{k >= j} X_kj g_k for the 64 columns of tile b
    ngd_col_dots(src, ldp, a.grad, blockIdx.x - n_tiles, d, [&](int j, double s) { a.vec[j] = j < d ? -s : 0.0; });
    return;
  }
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  NGD_WAVE;
  NgdFrag<T> acc;
  acc.zero();
  if (TRANS) ngd_product<T, true, true>(acc, src + (size_t)i0 * ldp, ldp, src + (size_t)j0 * ldp, ldp, i0, ldp, sAB, sAB + kNgdKC * kNgdLd);
  else ngd_product<T, false, false>(acc, src + i0, ldp, src + j0, ldp, 0, j0 + kNgdTile, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, T x) {
    const int i = i0 + ii, j = j0 + jj;
    if (i >= d || j >= d || i < j) return;
    dst[(size_t)j * d + i] = (TI)x;
    dst[(size_t)i * d + j] = (TI)x;
  });
  if (FIN) {
    for (int t = tid; t < kNgdTile * kNgdTile; t += 256) {
      const int i = i0 + (t & 63), j = j0 + (t >> 6);
      if (i >= d || j >= d || i < j) continue;
      a.params[d + (size_t)j * d + i] = (TI)src[(size_t)j * ldp + i];
      if (i > j) a.params[d + (size_t)i * d + j] = TI(0);
      const TI s = (TI)a.A[(size_t)i * ldp + j];   // S'_ji, the upper triangle
      a.state[(size_t)j * d + i] = s;
      a.state[(size_t)i * d + j] = s;
    }
  }
}

// The mean by 64-row (STAGE 3: 64-column) blocks, float64 sums with one fixed order.  STAGE 1: x = X v;  2: r = -g - S' x (S' from the upper
// triangle of A);  3: w = X' r;  4: m' = m - eta (x + X w), and the first workgroup: entropy / elbo / flags from the panels' partials, in panel order
template <typename T, typename TI, int STAGE>
__global__ __launch_bounds__(256) void k_natgrad_mean(NatgradArgs<T, TI> a) {
  __shared__ double sred[4 * kNgdTile];
  const int d = a.d, ldp = a.ldp, tid = threadIdx.x, b = blockIdx.x;
  double *v = a.vec, *x = a.vec + ldp, *rr = a.vec + 2 * ldp, *w = a.vec + 3 * ldp;
  if (STAGE == 3) {   // w_j = sum_{k >= j} X_kj r_k
    ngd_col_dots(a.X, ldp, rr, b, d, [&](int j, double s) { w[j] = j < d ? s : 0.0; });
    return;
  }
  const double *u = STAGE == 1 ? v : w;
  ngd_row_matvec(
      b, d, STAGE == 2, sred,
      [&](int i, int j) {
        if (STAGE == 2) return (double)a.A[j >= i ? (size_t)j * ldp + i : (size_t)i * ldp + j] * x[j];   // S'_ij from A's upper triangle
        return (double)a.X[(size_t)j * ldp + i] * u[j];
      },
      [&](int i, double tot) {
        if (STAGE == 1) x[i] = tot;
        else if (STAGE == 2) rr[i] = -(double)a.grad[i] - tot;
        else a.params[i] = (TI)((T)a.params[i] - (T)a.eta * (T)(x[i] + tot));
      });
  if (STAGE == 4 && b == 0 && tid == 0) {
    double tot = 0.0, bad = 0.0;
    for (int p = 0; p < a.nT; ++p) {
      tot += a.part[p];
      bad += a.part[a.nT + p];
    }
    ngd_finish(d, tot, bad > 0.0 ? 1 : 0, a.out);
  }
}

template <typename T, typename TI>
static NatgradArgs<T, TI> natgrad_args(mivi_ctx *c, void *params, void *state) {
  NatgradArgs<T, TI> a{};
  const NgdGeom g(c->cfg.d);
  a.d = c->cfg.d;
  a.nT = g.nT;
  a.ldp = g.ldp;
  a.params = (TI *)params;
  a.state = (TI *)state;
  a.out.status = (int *)c->status.p;
  if (a.d > kNatgradSmallD) {
    T *w = (T *)c->ms_work.p;
    a.G = w;
    a.P = w + g.mat();
    a.W = w + 2 * g.mat();
    a.A = w + 3 * g.mat();
    a.X = w + 4 * g.mat();
    a.Dinv = w + 5 * g.mat();
    a.part = (double *)c->ms_part.p;
    a.vec = a.part + 2 * g.nT;
  }
  return a;
}

// X = Lr^-1 from the Dinv tiles and the strictly lower tiles of A
template <typename T, typename TI>
static void launch_natgrad_inverse(mivi_ctx *c, NatgradArgs<T, TI> a) {
  hipLaunchKernelGGL((k_natgrad_mk<T, TI>), dim3(ngd_n_tiles(a.nT)), dim3(256), 0, c->stream, a);
  for (int i = 1; i < a.nT; ++i) {
    a.k = i;
    hipLaunchKernelGGL((k_natgrad_inv<T, TI>), dim3(i), dim3(256), 0, c->stream, a);
  }
}

template <typename T, typename TI>
static NatgradArgs<T, TI> natgrad_update_args(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double eta, int ensure,
                                              const void *logpi, void *entropy, void *elbo) {
  NatgradArgs<T, TI> a = natgrad_args<T, TI>(c, params, state);
  a.grad = (const TI *)grad;
  a.hess = (const TI *)hess;
  a.eta = eta;
  a.ensure = ensure ? 1 : 0;
  a.out = NgdOut<TI>{(const TI *)logpi, (TI *)entropy, (TI *)elbo, a.out.status};
  return a;
}

// d > kNatgradSmallD.  The tile kernels are instantiated in float64 arithmetic only; TI is the context's type.
template <typename TI>
static void launch_natgrad_tiles(mivi_ctx *c, NatgradArgs<double, TI> a) {
  typedef double T;
  const int nT = a.nT, n_tiles = ngd_n_tiles(nT);
  hipLaunchKernelGGL((k_natgrad_prep<T, TI, 0>), dim3(nT * nT), dim3(256), 0, c->stream, a);
  if (a.ensure) {
    hipLaunchKernelGGL((k_natgrad_gw<T, TI>), dim3(nT * nT), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL((k_natgrad_sp<T, TI>), dim3(n_tiles), dim3(256), 0, c->stream, a);
  }
  for (int k = nT - 1; k >= 0; --k) {
    a.k = k;
    hipLaunchKernelGGL((k_natgrad_upd<T, TI>), dim3(k + 1), dim3(256), 0, c->stream, a);
    if (k > 0) hipLaunchKernelGGL((k_natgrad_scale<T, TI>), dim3(k), dim3(256), 0, c->stream, a);
  }
  launch_natgrad_inverse(c, a);
  hipLaunchKernelGGL((k_natgrad_syrk<T, TI, false, true>), dim3(n_tiles + nT), dim3(256), 0, c->stream, a, (const T *)a.X, a.state + (size_t)a.d * a.d);
  hipLaunchKernelGGL((k_natgrad_mean<T, TI, 1>), dim3(nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_natgrad_mean<T, TI, 2>), dim3(nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_natgrad_mean<T, TI, 3>), dim3(nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_natgrad_mean<T, TI, 4>), dim3(nT), dim3(256), 0, c->stream, a);
}

template <typename TI>
static void launch_natgrad_init_tiles(mivi_ctx *c, NatgradArgs<double, TI> a) {
  typedef double T;
  const int nT = a.nT, n_tiles = ngd_n_tiles(nT);
  hipLaunchKernelGGL((k_natgrad_prep<T, TI, 1>), dim3(nT * nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_natgrad_dinv<T, TI>), dim3(nT), dim3(256), 0, c->stream, a);
  launch_natgrad_inverse(c, a);
  hipLaunchKernelGGL((k_natgrad_syrk<T, TI, true, false>), dim3(n_tiles), dim3(256), 0, c->stream, a, (const T *)a.X, a.state);
  hipLaunchKernelGGL((k_natgrad_syrk<T, TI, false, false>), dim3(n_tiles), dim3(256), 0, c->stream, a, (const T *)a.A, a.state + (size_t)a.d * a.d);
}

// The factorisation alone, for kernels_bam.hip: the padded float64 A (identity on the diagonal of its padding; only its lower tiles and the
// lower triangles of its diagonal tiles are read) -> Lr with A = Lr' Lr in the same places, the diagonal tiles' factors included; Dinv
// (nT tiles) and part ([2][nT]: sum log 1 / Lr_ii of a panel, its count of bad pivots) as the update leaves them.  2 nT - 1 launches.
void launch_natgrad_factor(mivi_ctx *c, int d, double *A, double *Dinv, double *part) {
  NatgradArgs<double, double> a{};
  const NgdGeom g(d);
  a.d = d;
  a.nT = g.nT;
  a.ldp = g.ldp;
  a.A = A;
  a.Dinv = Dinv;
  a.part = part;
  a.keep = 1;
  a.out.status = (int *)c->status.p;
  for (int k = g.nT - 1; k >= 0; --k) {
    a.k = k;
    hipLaunchKernelGGL((k_natgrad_upd<double, double>), dim3(k + 1), dim3(256), 0, c->stream, a);
    if (k > 0) hipLaunchKernelGGL((k_natgrad_scale<double, double>), dim3(k), dim3(256), 0, c->stream, a);
  }
}

// The finish of an update that factored the index-REVERSED Sigma' (kernels_bam.hip, kernels_wass.hip): run from the bottom-right corner on the
// reversed matrix the factorisation IS the lower Cholesky factorisation, C'_pq = Lr_(d-1-q)(d-1-p).  C' into the parameter vector (exact zeros
// above the diagonal); the first workgroup adds the panels' partials in order: entropy(q'), elbo and the flags (ngd_finish).
template <typename TI>
__global__ __launch_bounds__(256) void k_natgrad_factor_fin(int d, int nT, int ldp, const double *A, const double *part, TI *params, NgdOut<TI> out) {
  const int i0 = ((int)blockIdx.x % nT) * kNgdTile, j0 = ((int)blockIdx.x / nT) * kNgdTile;
  for (int t = threadIdx.x; t < kNgdTile * kNgdTile; t += 256) {
    const int p = i0 + (t & 63), q = j0 + (t >> 6);
    if (p >= d || q >= d) continue;
    params[d + (size_t)q * d + p] = p >= q ? (TI)A[(size_t)(d - 1 - p) * ldp + (d - 1 - q)] : TI(0);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) {
    double tot = 0.0, bad = 0.0;
    for (int p = 0; p < nT; ++p) {
      tot += part[p];   // sum log 1 / Lr_ii
      bad += part[nT + p];
    }
    ngd_finish(d, -tot, bad > 0.0 ? 1 : 0, out);
  }
}

void launch_natgrad_factor_fin(mivi_ctx *c, const double *A, const double *part, void *params, const void *logpi, void *entropy, void *elbo) {
  const int d = c->cfg.d;
  const NgdGeom g(d);
  by_dtype(c, [&](auto t) {
    using TI = decltype(t);
    hipLaunchKernelGGL((k_natgrad_factor_fin<TI>), dim3(g.nT * g.nT), dim3(256), 0, c->stream, d, g.nT, g.ldp, A, part, (TI *)params,
                       NgdOut<TI>{(const TI *)logpi, (TI *)entropy, (TI *)elbo, (int *)c->status.p});
  });
}

size_t natgrad_work_bytes(const mivi_ctx *c) {
  const NgdGeom g(c->cfg.d);   // (float64 scratch whatever the context's type)
  return c->cfg.d <= kNatgradSmallD ? 0 : (5 * g.mat() + (size_t)g.nT * kNgdTile * kNgdTile) * sizeof(double);
}

size_t natgrad_part_bytes(const mivi_ctx *c) {
  const NgdGeom g(c->cfg.d);
  return c->cfg.d <= kNatgradSmallD ? 0 : (2 * (size_t)g.nT + 4 * (size_t)g.ldp) * sizeof(double);
}

void launch_natgrad_update(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double eta, int ensure_posdef, const void *logpi,
                           void *entropy, void *elbo) {
  if (c->cfg.d <= kNatgradSmallD) {   // one workgroup, in the context's type
    by_dtype(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_natgrad_small<T, T>), dim3(1), dim3(256), 0, c->stream,
                         natgrad_update_args<T, T>(c, params, state, grad, hess, eta, ensure_posdef, logpi, entropy, elbo));
    });
  } else {   // tiles: float64 scratch and arithmetic for either type, only the loads and stores of the caller's buffers differ
    by_dtype(c, [&](auto t) {
      launch_natgrad_tiles(c, natgrad_update_args<double, decltype(t)>(c, params, state, grad, hess, eta, ensure_posdef, logpi, entropy, elbo));
    });
  }
}

void launch_natgrad_init(mivi_ctx *c, void *params, void *state) {
  if (c->cfg.d <= kNatgradSmallD) {
    by_dtype(c, [&](auto t) {
      using T = decltype(t);
      hipLaunchKernelGGL((k_natgrad_init_small<T, T>), dim3(1), dim3(256), 0, c->stream, natgrad_args<T, T>(c, params, state));
    });
  } else {
    by_dtype(c, [&](auto t) { launch_natgrad_init_tiles(c, natgrad_args<double, decltype(t)>(c, params, state)); });
  }
}

}  // namespace mivi
