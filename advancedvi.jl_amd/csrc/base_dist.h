// The non-normal base distributions of the location-scale families (mivi_set_base_dist; MvLocationScale(location, scale, dist),
// src/families/location_scale.jl:15-19, docs/src/families.md:72-101): per base the draw from Philox words, the variable part of
// -log phi and -psi = -(log phi)'.  The streams are part of the contract (philox.h, include/mivi.h); the constants of log phi and H(phi)
// are computed once on the host (api_basedist.hip).
//   Laplace : phi(x) = exp(-|x|) / 2;   -log phi = |x| + ln 2;   -psi(x) = sign(x)
//   TDist nu: -log phi = (nu + 1)/2 log1p(x^2 / nu) - [lgamma((nu+1)/2) - lgamma(nu/2) - 1/2 ln(nu pi)];   -psi(x) = (nu + 1) x / (nu + x^2)
// Every transform is evaluated in the context's element type T from uniforms that are exact in T.
#pragma once
#include "philox.h"

namespace mivi {

template <typename T>
struct BaseDraw;

template <>
struct BaseDraw<float> {
  // v = (((w >> 8) & 0x7fffff) + 0.5) 2^-23 in (0, 1), exact; the sign is the word's top bit (set: +)
  static __device__ __forceinline__ float laplace(uint32_t w) {
    const float v = ((float)((w >> 8) & 0x7fffffu) + 0.5f) * 1.1920928955078125e-07f;
    const float mag = -logf(v);
    return (w >> 31) ? mag : -mag;
  }
  // Bailey's polar form: sqrt(nu expm1(-(2/nu) ln U)) cos(2 pi V), uniforms as Box-Muller's; expm1 keeps U^(-2/nu) - 1 exact near U = 1
  static __device__ __forceinline__ float tdist(uint32_t wu, uint32_t wv, float nu) {
    const float u = ((float)(wu >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float v = ((float)(wv >> 9) + 0.5f) * 1.1920928955078125e-07f;
    const float r = sqrtf(nu * expm1f((-2.0f / nu) * logf(u)));
    float t = r * cospif(2.0f * v);
    asm volatile("" : "+v"(t));   // (a draw is a VALUE: no consumer contracts the product into its own arithmetic)
    return t;
  }
};

template <>
struct BaseDraw<double> {
  // v = ((w & 0x7fffffff) + 0.5) 2^-31
  static __device__ __forceinline__ double laplace(uint32_t w) {
    const double v = ((double)(w & 0x7fffffffu) + 0.5) * 4.656612873077392578125e-10;
    const double mag = -log(v);
    return (w >> 31) ? mag : -mag;
  }
  static __device__ __forceinline__ double tdist(uint32_t wu, uint32_t wv, double nu) {
    const double u = ((double)wu + 0.5) * 2.3283064365386962890625e-10;
    const double v = ((double)wv + 0.5) * 2.3283064365386962890625e-10;
    const double r = sqrt(nu * expm1((-2.0 / nu) * log(u)));
    double t = r * cospi(2.0 * v);
    asm volatile("" : "+v"(t));
    return t;
  }
};

__device__ __forceinline__ float bd_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double bd_log1p(double x) { return log1p(x); }

// the variable part of -log phi(x) (the constant is ValueIn::base_c0) and -psi(x)
template <typename T, int BASE>
__device__ __forceinline__ T base_neg_logpdf_var(T x, T nu) {
  if (BASE == MIVI_BASE_LAPLACE) return x < T(0) ? -x : x;
  return T(0.5) * (nu + T(1)) * bd_log1p(x * x / nu);
}
template <typename T, int BASE>
__device__ __forceinline__ T base_neg_psi(T x, T nu) {
  if (BASE == MIVI_BASE_LAPLACE) return x < T(0) ? T(-1) : T(1);
  return (nu + T(1)) * x / (nu + x * x);
}

// the four draws of row quad rq (rows 4 rq .. 4 rq + 3) of global column `col`
//   Laplace: ONE Philox block, q = col ceil(d/4) + rq, element r takes word r
//   TDist  : TWO blocks (a variate costs two words: its sine partner is not independent of it), q = col ceil(d/2) + 2 rq (+ 1);
//            the second one only if it holds a row < d
template <typename T, int BASE>
__device__ __forceinline__ void base_quad(uint64_t seed, uint64_t idx, uint64_t col, int d, int rq, T nu, T u[4]) {
  if (BASE == MIVI_BASE_LAPLACE) {
    const u32x4 b = eps_block_bits(seed, idx, col * (uint64_t)((d + 3) >> 2) + (uint64_t)rq);
    u[0] = BaseDraw<T>::laplace(b.x);
    u[1] = BaseDraw<T>::laplace(b.y);
    u[2] = BaseDraw<T>::laplace(b.z);
    u[3] = BaseDraw<T>::laplace(b.w);
  } else {
    const int d2 = (d + 1) >> 1;
    const u32x4 b0 = eps_block_bits(seed, idx, col * (uint64_t)d2 + (uint64_t)(2 * rq));
    u[0] = BaseDraw<T>::tdist(b0.x, b0.y, nu);
    u[1] = BaseDraw<T>::tdist(b0.z, b0.w, nu);
    u[2] = u[3] = T(0);
    if (2 * rq + 1 < d2) {
      const u32x4 b1 = eps_block_bits(seed, idx, col * (uint64_t)d2 + (uint64_t)(2 * rq + 1));
      u[2] = BaseDraw<T>::tdist(b1.x, b1.y, nu);
      u[3] = BaseDraw<T>::tdist(b1.z, b1.w, nu);
    }
  }
}

}  // namespace mivi
