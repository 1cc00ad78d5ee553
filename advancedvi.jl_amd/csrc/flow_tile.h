// What the coupling-flow kernels share (kernels_flow.hip: RealNVP, kernels_nsf.hip: the neural spline flow): the tile of 16 samples as
// [row][16] blocks in LDS, the kernels' argument block, the draws of a tile, and the moves between a tile and a d x * plane.
#pragma once
#include "mivi_internal.h"
#include "device_common.h"

namespace mivi {

// (the forward pass saves ALL 16 columns of a tile to flow_X and the VJP reads them back: the planes hold cap_M columns, and ensure_work
//  rounds cap_M up to a multiple of 64, so a launch's last tile ends inside its own plane -- launch_flow_forward checks it)
constexpr int kFlowTile = 16;            // samples per tile
constexpr int kFlowBlk = 64 * kFlowTile;   // elements of one [64][16] block
constexpr int kFlowMaxSlices = 64;

template <typename T>
struct FlowArgs {
  FlowArch a;
  int M, capM;         // samples of this launch; columns of X's planes
  const T *params;
  RngArgs rng;
  T *X;                // [L + 1][capM][d]: x^0 = eps ... x^L = z (or nullptr: not saved)
  T *Z, *eps;          // d x M outputs, ld = d (or nullptr)
  const T *Zin;        // k_flow_inverse: the points, d x M
  T *logq;             // k_flow_inverse: log q per point
  const T *Wg;         // k_flow_vjp: grad_z ell, d x M (ld = d)
  double *lq;          // f64 log q per sample
  double *part;        // [n_slices][params_len] f64
  int kind;            // MIVI_ENT_MONTE_CARLO or MIVI_ENT_STL
  double invM;
};

__device__ __forceinline__ int round16(int x) { return (x + 15) & ~15; }

// c = x[B_l] -> H0 (zero rows up to a multiple of 16) from a [d][16] block
template <typename T>
__device__ __forceinline__ void flow_take_c(const T *XC, T *H0, int nB, int pa) {
  for (int e = threadIdx.x; e < round16(nB) * 16; e += 64) {
    const int j = e >> 4, m = e & 15;
    H0[e] = j < nB ? XC[(2 * j + 1 - pa) * 16 + m] : T(0);
  }
  __syncthreads();
}
// a tile of a d x * plane (ld = d) <-> a [d][16] block; columns from n_ok on read as zero / are not stored
template <typename T>
__device__ __forceinline__ void flow_load_tile(const T *src, T *blk, int d, int n_ok, T scale = T(1)) {
  for (int e = threadIdx.x; e < 16 * d; e += 64) {
    const int m = e / d, i = e - m * d;
    blk[i * 16 + m] = m < n_ok ? scale * src[(size_t)m * d + i] : T(0);
  }
  __syncthreads();
}
template <typename T>
__device__ __forceinline__ void flow_store_tile(T *dst, const T *blk, int d, int n_ok) {
  for (int e = threadIdx.x; e < 16 * d; e += 64) {
    const int m = e / d, i = e - m * d;
    if (m < n_ok) dst[(size_t)m * d + i] = blk[i * 16 + m];
  }
}
// the draws of the tile at sample m0 (the mean-field Philox stream) -> a [d][16] block; columns from n_ok on are zero
template <typename T>
__device__ __forceinline__ void flow_draw_tile(const RngArgs &rng, T *XC, int d, int m0, int n_ok) {
  const int d4 = (d + 3) >> 2;
  const uint64_t idx = rng_index(rng);
  for (int e = threadIdx.x; e < 16 * d4; e += 64) {
    const int m = e / d4, rq = e - m * d4;
    T ev[4] = {T(0), T(0), T(0), T(0)};
    if (m < n_ok) eps_block<T>(rng.seed, idx, (uint64_t)(rng.m_offset + m0 + m) * (uint64_t)d4 + (uint64_t)rq, ev);
#pragma unroll
    for (int r = 0; r < 4; ++r)
      if (4 * rq + r < d) XC[(4 * rq + r) * 16 + m] = ev[r];
  }
  __syncthreads();
}

extern __shared__ double flow_lds[];

// a kernel's dynamic LDS of `elems` elements: above 48 KB the runtime has to be told
template <typename T, typename K>
inline bool flow_lds_attr(K kern, int elems) {
  const size_t bytes = (size_t)elems * sizeof(T);
  if (bytes <= 48 * 1024) return true;
  return hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}

template <typename T>
inline FlowArgs<T> flow_args(mivi_ctx *c, const void *params, int M) {
  FlowArgs<T> g{};
  g.a = c->flow;
  g.M = M;
  g.capM = c->cap_M;
  g.params = (const T *)params;
  return g;
}

// kernels_nsf.hip: the neural spline flow's backward sweeps from the argument block launch_flow_vjp_finish (kernels_flow.hip) filled,
// which launches the finish kernel both families share; instantiated for float and double
template <typename T>
void launch_nsf_vjp(mivi_ctx *c, const FlowArgs<T> &g, int n_slices, long long plen);

}  // namespace mivi
