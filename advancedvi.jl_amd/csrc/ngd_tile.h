// What the measure-space update kernels share (kernels_ngd.hip, kernels_natgrad.hip).  The 64 x 64 tile product on the matrix cores: operands
// staged through LDS in K chunks of 32, K-major (sA[k][i], sB[k][j]); f32: v_mfma_f32_32x32x2_f32 with exact f32 operands, f64:
// v_mfma_f64_16x16x4_f64; 256 threads, one wave per 32 x 32 quadrant (NgdFrag, ngd_product).  The tile geometry (NgdGeom, ngd_tile_of), the
// column-dot and row-matvec bodies of the mean's riders, the bad-pivot predicate and the finish (entropy, elbo, sticky flags: NgdOut, ngd_finish).
#pragma once
#include <hip/hip_runtime.h>

#include "mivi_internal.h"

namespace mivi {

constexpr int kNgdTile = 64;
constexpr int kNgdKC = 32;
constexpr int kNgdLd = kNgdTile + 1;

__host__ __device__ constexpr int ngd_n_tiles(int nT) { return nT * (nT + 1) / 2; }   // the tiles of one triangle, diagonal included

// host side: d in whole tiles.  Every buffer between the launches is padded to ldp = 64 nT.
struct NgdGeom {
  int nT, ldp, n_tiles;
  explicit NgdGeom(int d) : nT((d + kNgdTile - 1) / kNgdTile), ldp(nT * kNgdTile), n_tiles(ngd_n_tiles(nT)) {}
  size_t mat() const { return (size_t)ldp * ldp; }
};

// lane, and the 32 x 32 quadrant (wr, wc) of the thread's wave
#define NGD_WAVE const int lane = threadIdx.x & 63, w_ = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), wr = w_ >> 1, wc = w_ & 1

// One wave owns a 32 x 32 quadrant (wr, wc) of the 64 x 64 tile.  sA[k][i], sB[k][j]: both operands K-major in LDS.
template <typename T>
struct NgdFrag;

template <>
struct NgdFrag<float> {
  typedef float acc_t __attribute__((ext_vector_type(16)));
  acc_t c;
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int r = 0; r < 16; ++r) c[r] = 0.f;
  }
  // A operand lane l: A[i = l & 31][k = l >> 5]; B: B[k = l >> 5][j = l & 31]
  __device__ __forceinline__ void chunk(const float *sA, const float *sB, int wr, int wc, int lane) {
    const int l31 = lane & 31, h = lane >> 5;
#pragma unroll
    for (int u = 0; u < kNgdKC / 2; ++u) {
      const float av = sA[(2 * u + h) * kNgdLd + 32 * wr + l31];
      const float bv = sB[(2 * u + h) * kNgdLd + 32 * wc + l31];
      c = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, c, 0, 0, 0);
    }
  }
  // D register r of lane l: row 8 (r / 4) + 4 (l >> 5) + (r & 3), column l & 31
  template <class F>
  __device__ __forceinline__ void each(int wr, int wc, int lane, F &&f) {
#pragma unroll
    for (int r = 0; r < 16; ++r) f(32 * wr + 8 * (r >> 2) + 4 * (lane >> 5) + (r & 3), 32 * wc + (lane & 31), c[r]);
  }
};

template <>
struct NgdFrag<double> {
  typedef double acc_t __attribute__((ext_vector_type(4)));
  acc_t c[2][2];
  __device__ __forceinline__ void zero() {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int r = 0; r < 4; ++r) c[x][y][r] = 0.0;
  }
  // A operand lane l: A[i = l & 15][k = l >> 4]; B: B[k = l >> 4][j = l & 15]
  __device__ __forceinline__ void chunk(const double *sA, const double *sB, int wr, int wc, int lane) {
    const int l15 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int u = 0; u < kNgdKC / 4; ++u) {
      const double *pa = sA + (4 * u + q) * kNgdLd + 32 * wr + l15, *pb = sB + (4 * u + q) * kNgdLd + 32 * wc + l15;
      const double a0 = pa[0], a1 = pa[16], b0 = pb[0], b1 = pb[16];
      c[0][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b0, c[0][0], 0, 0, 0);
      c[0][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b1, c[0][1], 0, 0, 0);
      c[1][0] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b0, c[1][0], 0, 0, 0);
      c[1][1] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b1, c[1][1], 0, 0, 0);
    }
  }
  // D register r of lane l: row (l >> 4) + 4 r, column l & 15
  template <class F>
  __device__ __forceinline__ void each(int wr, int wc, int lane, F &&f) {
#pragma unroll
    for (int x = 0; x < 2; ++x)
#pragma unroll
      for (int y = 0; y < 2; ++y)
#pragma unroll
        for (int r = 0; r < 4; ++r) f(32 * wr + 16 * x + (lane >> 4) + 4 * r, 32 * wc + 16 * y + (lane & 15), c[x][y][r]);
  }
};

// lower tile number -> (ti, tj), ti >= tj, rows in order
__device__ __forceinline__ void ngd_tile_of(int b, int &ti, int &tj) {
  int i = (int)((sqrtf(8.f * (float)b + 1.f) - 1.f) * 0.5f);
  while ((i + 1) * (i + 2) / 2 <= b) ++i;
  while (i * (i + 1) / 2 > b) --i;
  ti = i;
  tj = b - i * (i + 1) / 2;
}

// acc += sum_{k in [k_beg, k_end)} A(x, k) B(k, y) over one 64 x 64 tile, the operands given as element getters a(x, k), b(y, k) with x, y in
// [0, 64).  AK: A is read "k-fast" (K contiguous in memory), thread -> (x = (tid >> 5) + 8 r, k = k0 + (tid & 31)); otherwise "row-fast" (the
// tile's 64 rows contiguous), thread -> (x = tid & 63, k = k0 + (tid >> 6) + 4 r); r < 8.  BK the same for B.  The range is a multiple of 32
// and the same for the whole workgroup; sA / sB: kNgdKC x kNgdLd each.
template <typename T, bool AK, bool BK, class GA, class GB>
__device__ __forceinline__ void ngd_product(NgdFrag<T> &acc, GA &&a, GB &&b, int k_beg, int k_end, T *sA, T *sB) {
  const int tid = threadIdx.x;
  NGD_WAVE;
  if (k_beg >= k_end) return;
  T ra[8], rb[8];
  auto load = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      ra[r] = AK ? a((tid >> 5) + 8 * r, k0 + (tid & 31)) : a(tid & 63, k0 + (tid >> 6) + 4 * r);
      rb[r] = BK ? b((tid >> 5) + 8 * r, k0 + (tid & 31)) : b(tid & 63, k0 + (tid >> 6) + 4 * r);
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (AK) sA[(tid & 31) * kNgdLd + (tid >> 5) + 8 * r] = ra[r];
      else sA[((tid >> 6) + 4 * r) * kNgdLd + (tid & 63)] = ra[r];
      if (BK) sB[(tid & 31) * kNgdLd + (tid >> 5) + 8 * r] = rb[r];
      else sB[((tid >> 6) + 4 * r) * kNgdLd + (tid & 63)] = rb[r];
    }
  };
  load(k_beg);
  for (int k0 = k_beg; k0 < k_end; k0 += kNgdKC) {
    stash();
    __syncthreads();
    if (k0 + kNgdKC < k_end) load(k0 + kNgdKC);
    acc.chunk(sA, sB, wr, wc, lane);
    __syncthreads();
  }
}

// padded operands, nothing masked: A(x, k) = A[x lda + k] (AK) or A[k lda + x]; B the same
template <typename T, bool AK, bool BK>
__device__ __forceinline__ void ngd_product(NgdFrag<T> &acc, const T *A, size_t lda, const T *B, size_t ldb, int k_beg, int k_end, T *sA, T *sB) {
  ngd_product<T, AK, BK>(
      acc, [=](int x, int k) { return AK ? A[(size_t)x * lda + k] : A[(size_t)k * lda + x]; },
      [=](int y, int k) { return BK ? B[(size_t)y * ldb + k] : B[(size_t)k * ldb + y]; }, k_beg, k_end, sA, sB);
}

// s_j = sum_{k >= j} M[j ld + k] x[k] for the 64 columns j of block b (0 for j >= d), put(j, s_j): one wave per column, lanes along k, a
// fixed shuffle tree.  256 threads.
template <typename TM, typename TX, class Put>
__device__ __forceinline__ void ngd_col_dots(const TM *M, size_t ld, const TX *x, int b, int d, Put &&put) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int jj = w; jj < kNgdTile; jj += 4) {
    const int j = b * kNgdTile + jj;
    double s = 0.0;
    if (j < d)
      for (int k = j + lane; k < d; k += 64) s += (double)M[(size_t)j * ld + k] * (double)x[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
    if (lane == 0) put(j, s);
  }
}

// tot_i = sum_{j < (full ? d : i + 1)} term(i, j) for the 64 rows i of block b, put(i, tot_i) for i < d: a row per lane, four partial sums per
// row (j mod 4), added in order through sred (4 x 64 doubles of LDS).  256 threads, all of them call this.
template <class Term, class Put>
__device__ __forceinline__ void ngd_row_matvec(int b, int d, bool full, double *sred, Term &&term, Put &&put) {
  const int r = threadIdx.x & 63, q = threadIdx.x >> 6, i = b * kNgdTile + r;
  double s = 0.0;
  if (i < d) {
    const int n = full ? d : i + 1;
    for (int j = q; j < n; j += 4) s += term(i, j);
  }
  sred[q * kNgdTile + r] = s;
  __syncthreads();
  if (q == 0 && i < d) put(i, ((sred[r] + sred[kNgdTile + r]) + sred[2 * kNgdTile + r]) + sred[3 * kNgdTile + r]);
}

// a scale's diagonal entry / a Cholesky pivot that is not a positive finite number
__device__ __forceinline__ bool ngd_bad(double p) { return !(p > 0.0) || !isfinite(p); }

// where an update's last launch leaves its values; TI: the context's type
template <typename TI>
struct NgdOut {
  const TI *logpi;   // nullable: elbo = *logpi + entropy(q')
  TI *entropy_out;   // nullable
  TI *elbo_out;      // nullable
  int *status;       // bit 0: entropy / elbo not finite, bit 1: a C'_ii / pivot that is not a positive finite number
};

// entropy(q') = d/2 (1 + log 2 pi) + logsum, elbo and the sticky flags
template <typename TI>
__device__ __forceinline__ void ngd_finish(int d, double logsum, int bad, const NgdOut<TI> &o) {
  const double ent = 0.5 * (double)d * (1.0 + kLog2Pi) + logsum;
  const TI ent_t = (TI)ent;
  if (o.entropy_out) *o.entropy_out = ent_t;
  bool finite = isfinite((double)ent_t);
  if (o.elbo_out) {
    const TI e = (o.logpi ? *o.logpi : TI(0)) + ent_t;
    *o.elbo_out = e;
    finite = finite && isfinite((double)e);
  }
  const int bits = (bad ? 2 : 0) | (finite ? 0 : 1);
  if (bits) atomicOr(o.status, bits);
}

}  // namespace mivi
