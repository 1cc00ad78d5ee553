// The 64 x 64 tile product on the matrix cores that the measure-space update kernels share (kernels_ngd.hip, kernels_natgrad.hip): operands
// staged through LDS in K chunks of 32, K-major (sA[k][i], sB[k][j]); f32: v_mfma_f32_32x32x2_f32 with exact f32 operands, f64:
// v_mfma_f64_16x16x4_f64.  256 threads, one wave per 32 x 32 quadrant.
#pragma once
#include <hip/hip_runtime.h>

namespace mivi {

constexpr int kNgdTile = 64;
constexpr int kNgdKC = 32;
constexpr int kNgdLd = kNgdTile + 1;

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

}  // namespace mivi
