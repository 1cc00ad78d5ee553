// Kernels of a non-normal base distribution (mivi_set_base_dist; base_dist.h): the draw stage of both location-scale families and the
// mean-field family's sample and gradient on the draws in memory.  api_basedist.hip drives them; the full-rank family's product, solve
// and VJP are the first-generation kernels (kernels_fullrank.hip), which are base-free.
// No floating-point atomics, one summation order: results repeat bitwise.
#include "device_common.h"
#include "base_dist.h"

namespace mivi {

template <typename T>
struct BdDrawArgs {
  int d, M, dP, MP;
  RngArgs rng;
  T *U;       // U[i + m dP]: the draws laid out like eps, rows d .. 4 ceil(d/4) - 1 written as zeros
  T *UT;      // UT[m + i MP] (or nullptr)
  T *R;       // -psi(U), laid out like U (or nullptr)
  double *he_part;   // per workgroup: the sum of the variable part of -log phi(u) over its tile
  T nu;
};

__device__ __forceinline__ void store_quad(float *p, const float (&v)[4]) { *reinterpret_cast<float4 *>(p) = make_float4(v[0], v[1], v[2], v[3]); }
__device__ __forceinline__ void store_quad(double *p, const double (&v)[4]) {   // two 16-byte stores
  *reinterpret_cast<double2 *>(p) = make_double2(v[0], v[1]);
  *reinterpret_cast<double2 *>(p + 2) = make_double2(v[2], v[3]);
}

// One thread per row quad of one column (Laplace: one Philox block; TDist: two), lanes along the sample axis: a workgroup covers the
// 16 rows x 64 columns tile of k_eps, so the draw leaves eps_blocks(c, M) partials like the normal one.  Transcendental-bound (per
// element: Laplace one log; TDist log, expm1, sqrt, cospi, and log1p for the Monte-Carlo entropy), so the plain layout is kept:
// 16-byte stores of U / R from the thread that drew them, UT coalesced along m.
template <typename T, int BASE>
__global__ __launch_bounds__(256) void k_bd_draw(BdDrawArgs<T> a) {
  __shared__ double red[4];
  const int tid = threadIdx.x, d = a.d, d4 = (d + 3) >> 2;
  const int nrt = (d + 15) >> 4;
  const int tile = blockIdx.x;
  const int i0 = (tile % nrt) * 16, m0 = (tile / nrt) * 64;
  const int m = m0 + (tid & 63), rq = (i0 >> 2) + (tid >> 6);
  T he = 0;
  if (m < a.M && rq < d4) {
    T u[4], r[4];
    base_quad<T, BASE>(a.rng.seed, rng_index(a.rng), (uint64_t)(a.rng.m_offset + m), d, rq, a.nu, u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int i = 4 * rq + k;
      const bool ok = i < d;
      u[k] = ok ? u[k] : T(0);
      he += ok ? base_neg_logpdf_var<T, BASE>(u[k], a.nu) : T(0);
      r[k] = ok ? base_neg_psi<T, BASE>(u[k], a.nu) : T(0);
      if (a.UT && ok) a.UT[(size_t)i * a.MP + m] = u[k];
    }
    store_quad(a.U + (size_t)m * a.dP + 4 * rq, u);   // (4 rq + 3 < dP: dP is a multiple of 64)
    if (a.R) store_quad(a.R + (size_t)m * a.dP + 4 * rq, r);
  }
  const double s = block_sum<double, 256>((double)he, red);
  if (tid == 0) a.he_part[tile] = s;
}

void launch_bd_draw(mivi_ctx *c, const RngArgs &rng, int M, void *U, void *UT, void *R) {
  const int nblk = eps_blocks(c, M);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    BdDrawArgs<T> a;
    a.d = c->cfg.d;
    a.M = M;
    a.dP = c->dP;
    a.MP = c->MP;
    a.rng = rng;
    a.U = (T *)U;
    a.UT = (T *)UT;
    a.R = (T *)R;
    a.he_part = (double *)c->he_part[c->cur].p;
    a.nu = (T)c->base_nu;
    if (c->base == MIVI_BASE_LAPLACE)
      hipLaunchKernelGGL((k_bd_draw<T, MIVI_BASE_LAPLACE>), dim3(nblk), dim3(256), 0, c->stream, a);
    else
      hipLaunchKernelGGL((k_bd_draw<T, MIVI_BASE_TDIST>), dim3(nblk), dim3(256), 0, c->stream, a);
  });
}

// mean field: Z = sigma o U + m (Z: ld d; U: ld dP)
template <typename T>
__global__ __launch_bounds__(256) void k_bd_mf_sample(int d, int M, int dP, const T *__restrict__ params, const T *__restrict__ U, T *__restrict__ Z) {
  const int i = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (i < d && m < M) Z[(size_t)m * d + i] = params[d + i] * U[(size_t)m * dP + i] + params[i];
}

void launch_bd_mf_sample(mivi_ctx *c, const void *params, int M, const void *U, void *Z) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bd_mf_sample<T>, dim3((c->cfg.d + 255) / 256, M), dim3(256), 0, c->stream, c->cfg.d, M, c->dP, (const T *)params, (const T *)U, (T *)Z);
  });
}

// mean field: dm = -mean_m w, dsigma = -mean_m w o u - c_H / sigma with w = W (+ R / sigma: the sticking-the-landing term -psi(u) / sigma).
// A workgroup owns 64 rows (lanes along the rows: coalesced) and deals the sample axis to its four waves; f64 sums, the four waves'
// added in index order.
template <typename T>
__global__ __launch_bounds__(256) void k_bd_mf_grad(int d, int M, int dP, const T *__restrict__ params, const T *__restrict__ W, const T *__restrict__ U,
                                                    const T *__restrict__ R, OutArgs out) {
  __shared__ double red[2][4][64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int i = blockIdx.x * 64 + lane;
  double sW = 0.0, sWu = 0.0, sigma = 1.0;
  if (i < d) {
    sigma = (double)params[d + i];
    for (int m = w; m < M; m += 4) {
      double g = (double)W[(size_t)m * d + i];
      const double u = (double)U[(size_t)m * dP + i];
      if (R) g += (double)R[(size_t)m * dP + i] / sigma;
      sW += g;
      sWu += g * u;
    }
  }
  red[0][w][lane] = sW;
  red[1][w][lane] = sWu;
  __syncthreads();
  if (w == 0 && i < d) {
    const double a = ((red[0][0][lane] + red[0][1][lane]) + red[0][2][lane]) + red[0][3][lane];
    const double b = ((red[1][0][lane] + red[1][1][lane]) + red[1][2][lane]) + red[1][3][lane];
    const double invM = 1.0 / (double)out.M_total;
    T *gr = (T *)out.grad;
    gr[i] = mf_grad_entry<T>(a, invM, false, 0.0, 1.0);
    gr[d + i] = mf_grad_entry<T>(b, invM, true, direct_entropy_coeff(out.ent_kind), sigma);
  }
}

void launch_bd_mf_grad(mivi_ctx *c, const void *params, int M, const void *U, const void *R, const OutArgs &out) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bd_mf_grad<T>, dim3((c->cfg.d + 63) / 64), dim3(256), 0, c->stream, c->cfg.d, M, c->dP, (const T *)params, (const T *)c->W.p,
                       (const T *)U, (const T *)R, out);
  });
}

}  // namespace mivi
