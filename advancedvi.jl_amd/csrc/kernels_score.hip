// The score-gradient ELBO estimator's own kernels (ScoreGradELBO, src/algorithms/scoregradelbo.jl:87-117 -- the VarGrad objective
// (mean(f^2) - mean(f)^2) / 2, f_m = log q(z_m) - log pi(z_m), differentiated through log q only).  With eps_m = C^-1 (z_m - mu):
//   lq_m   = -|eps_m|^2 / 2 - sum_i log C_ii - (d / 2) log 2 pi
//   value  = mean((f - fbar)^2) / 2          elbo = -fbar
//   full rank : d/dmu = (1/M) C^-T E (f - fbar)              d/dC = (1/M) tril(C^-T E diag(f - fbar) E')
//   mean field: d/dmu_i = (1/M) sum_m (f_m - fbar) eps_im / sigma_i     d/dsigma_i = (1/M) sum_m (f_m - fbar) eps_im^2 / sigma_i
// (the direct -diag(1 / C_ii) term of d lq / dC is weighted by sum_m (f_m - fbar) = 0).  Everything between the per-sample target values
// and the weights is f64 whatever the context's dtype, summed in fixed trees: no floating-point atomics, two calls agree bit for bit.
// The full-rank gradient is the library's solve (W = -C^-T E diag(f - fbar)) and VJP; what is here are the per-sample statistics, the
// column scaling in front of the solve, the dense-Gaussian target's per-sample values and the mean-field gradient.
#include "device_common.h"

namespace mivi {

// he[m] = |eps_m|^2.  One workgroup per sample.  FR: read from the draw (leading dimension ld); mean-field: drawn again from Philox
// (the same words and the same Box-Muller as k_mf_sample: bitwise the eps behind Z).
template <typename T, bool FR>
__global__ __launch_bounds__(256) void k_sg_norms(int d, int ld, const T *eps, RngArgs rng, double *he) {
  __shared__ double red[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  double acc = 0.0;
  if (FR) {
    const T *e = eps + (size_t)m * ld;
    for (int i = tid; i < d; i += 256) {
      const double v = (double)e[i];
      acc += v * v;
    }
  } else {
    const int d4 = (d + 3) >> 2;
    const uint64_t idx = rng_index(rng);
    for (int rq = tid; rq < d4; rq += 256) {
      T e[4];
      eps_block<T>(rng.seed, idx, (uint64_t)(rng.m_offset + m) * (uint64_t)d4 + (uint64_t)rq, e);
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * rq + r < d) acc += (double)e[r] * (double)e[r];
    }
  }
  const double s = block_sum<double, 256>(acc, red);
  if (tid == 0) he[m] = s;
}

// dense-Gaussian target, per sample: ell_m = r_m' g_m / 2 with r = z - mean and g = -P r as the dense-target product left it in W
// (its own epilogue only keeps per-tile sums of this).  One workgroup per sample.
template <typename T>
__global__ __launch_bounds__(256) void k_sg_dense_ell(int d, const T *Z, const T *G, const T *t_mean, double *ell) {
  __shared__ double red[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const T *z = Z + (size_t)m * d, *g = G + (size_t)m * d;
  double acc = 0.0;
  for (int i = tid; i < d; i += 256) acc += 0.5 * (double)(z[i] - t_mean[i]) * (double)g[i];
  const double s = block_sum<double, 256>(acc, red);
  if (tid == 0) ell[m] = s;
}

// One workgroup: sum_i log C_ii, f_m, fbar, the centred weights w_m = f_m - fbar (centre first, then square), value, elbo and the
// sticky status flags (bit 0: value or elbo not finite; bit 1: a non-positive scale diagonal), as the value kernels set them.
template <typename T>
struct SgStatsArgs {
  int d, M, fullrank;
  const T *params;
  const double *he;      // |eps_m|^2
  const T *ell;          // per-sample target values (generic targets) ...
  const double *ell64;   // ... or the dense-Gaussian target's (f64); exactly one of the two is set
  const T *bij_ld;       // logabsdetjac per sample (Stacked bijector) or nullptr
  double ell_const;
  double *w;
  T *value, *elbo;
  int *status;
};
template <typename T>
__global__ __launch_bounds__(256) void k_sg_stats(SgStatsArgs<T> a) {
  __shared__ double red[8];
  const int tid = threadIdx.x, d = a.d, M = a.M;
  double v2[2] = {0.0, 0.0};   // sum log C_ii, #non-positive
  for (int i = tid; i < d; i += 256) {
    const T cii = a.fullrank ? a.params[(size_t)d + (size_t)i * d + i] : a.params[d + i];
    v2[0] += log((double)cii);
    v2[1] += (cii > T(0)) ? 0.0 : 1.0;
  }
  block_sum_n<double, 256, 2>(v2, red);
  const double lq0 = -v2[0] - 0.5 * (double)d * kLog2Pi;
  double acc = 0.0;
  for (int m = tid; m < M; m += 256) {
    double lp = (a.ell64 ? a.ell64[m] : (double)a.ell[m]) + a.ell_const;
    if (a.bij_ld) lp += (double)a.bij_ld[m];
    const double f = (lq0 - 0.5 * a.he[m]) - lp;
    a.w[m] = f;
    acc += f;
  }
  __syncthreads();
  const double fbar = block_sum<double, 256>(acc, red) / (double)M;
  acc = 0.0;
  for (int m = tid; m < M; m += 256) {   // (every thread re-reads what it wrote itself)
    const double w = a.w[m] - fbar;
    a.w[m] = w;
    acc += w * w;
  }
  __syncthreads();
  const double var = block_sum<double, 256>(acc, red) / (double)M;
  if (tid == 0) {
    const double value = 0.5 * var, elbo = -fbar;
    *a.value = (T)value;
    if (a.elbo) *a.elbo = (T)elbo;
    const int st = ((isfinite(value) && isfinite(elbo)) ? 0 : 1) | (v2[1] > 0.0 ? 2 : 0);
    if (st && a.status) atomicOr(a.status, st);
  }
}

// full rank: S = -eps diag(w) laid out like the draw (leading dimension dP; rows >= d and columns >= M zero) -- scaling the columns
// commutes with C^-T, which is what lets the existing solve run on it -- and W = 0 (the solve adds into it).  blockIdx.y = column.
template <typename T>
__global__ __launch_bounds__(256) void k_sg_scale(int d, int dP, int M, const T *eps, const double *w, T *S, T *W) {
  const int i = blockIdx.x * 256 + threadIdx.x, m = blockIdx.y;
  if (i >= dP) return;
  const bool in = i < d && m < M;
  S[(size_t)m * dP + i] = in ? -(eps[(size_t)m * dP + i] * (T)w[m]) : T(0);
  if (in) W[(size_t)m * d + i] = T(0);
}

// mean field: a workgroup owns 16 row quads; its 16 groups of 16 threads deal the samples among them, every thread redraws its
// quad's eps from Philox (no d x M intermediate besides Z), the weights come from LDS in chunks; the groups' sums are added in
// group order.
constexpr int kSgChunk = 2048;
template <typename T>
__global__ __launch_bounds__(256) void k_sg_mf_grad(int d, int M, const T *params, RngArgs rng, const double *w, T *grad) {
  __shared__ double ws[kSgChunk];
  __shared__ double red[16][16][8];
  const int tid = threadIdx.x, q = tid & 15, g = tid >> 4, d4 = (d + 3) >> 2;
  const int rq = blockIdx.x * 16 + q;
  const uint64_t idx = rng_index(rng);
  double a1[4] = {0, 0, 0, 0}, a2[4] = {0, 0, 0, 0};
  for (int m0 = 0; m0 < M; m0 += kSgChunk) {
    const int n = min(kSgChunk, M - m0);
    __syncthreads();
    for (int k = tid; k < n; k += 256) ws[k] = w[m0 + k];
    __syncthreads();
    if (rq < d4)
      for (int k = g; k < n; k += 16) {
        T e[4];
        eps_block<T>(rng.seed, idx, (uint64_t)(rng.m_offset + m0 + k) * (uint64_t)d4 + (uint64_t)rq, e);
        const double wm = ws[k];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const double we = wm * (double)e[r];
          a1[r] += we;
          a2[r] += we * (double)e[r];
        }
      }
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    red[g][q][r] = a1[r];
    red[g][q][4 + r] = a2[r];
  }
  __syncthreads();
  if (tid < 128) {
    const int qq = tid >> 3, k = tid & 7, r = k & 3, i = 4 * (blockIdx.x * 16 + qq) + r;
    if (i < d) {
      double s = 0.0;
#pragma unroll
      for (int gg = 0; gg < 16; ++gg) s += red[gg][qq][k];
      const double sigma = (double)params[d + i];
      grad[(k < 4 ? 0 : d) + i] = (T)(s / sigma / (double)M);
    }
  }
}

// ---------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------
template <typename T>
static void sg_norms_impl(mivi_ctx *c, const RngArgs &rng, int M) {
  double *he = (double *)c->sg_d.p;
  if (c->cfg.family == MIVI_FULLRANK)
    hipLaunchKernelGGL((k_sg_norms<T, true>), dim3(M), dim3(256), 0, c->stream, c->cfg.d, c->dP, (const T *)c->eps[0].p, rng, he);
  else
    hipLaunchKernelGGL((k_sg_norms<T, false>), dim3(M), dim3(256), 0, c->stream, c->cfg.d, 0, (const T *)nullptr, rng, he);
}
void launch_sg_norms(mivi_ctx *c, const RngArgs &rng, int M) {
  by_dtype(c, [&](auto t) { sg_norms_impl<decltype(t)>(c, rng, M); });
}

void launch_sg_dense_ell(mivi_ctx *c, int M) {
  double *ell = (double *)c->sg_d.p + c->sg_cap;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_sg_dense_ell<T>, dim3(M), dim3(256), 0, c->stream, c->cfg.d, (const T *)c->Z.p, (const T *)c->W.p, (const T *)c->t_mean.p, ell);
  });
}

template <typename T>
static void sg_stats_impl(mivi_ctx *c, const void *params, int M, bool ell_f64, void *value, void *elbo) {
  SgStatsArgs<T> a;
  a.d = c->cfg.d;
  a.M = M;
  a.fullrank = c->cfg.family == MIVI_FULLRANK;
  a.params = (const T *)params;
  a.he = (const double *)c->sg_d.p;
  a.ell = ell_f64 ? nullptr : (const T *)c->ell.p;
  a.ell64 = ell_f64 ? (const double *)c->sg_d.p + c->sg_cap : nullptr;
  a.bij_ld = c->bij_on ? (const T *)c->bij_ld.p : nullptr;
  a.ell_const = c->t_const;
  a.w = (double *)c->sg_d.p + 2 * (size_t)c->sg_cap;
  a.value = (T *)value;
  a.elbo = (T *)elbo;
  a.status = (int *)c->status.p;
  hipLaunchKernelGGL(k_sg_stats<T>, dim3(1), dim3(256), 0, c->stream, a);
}
void launch_sg_stats(mivi_ctx *c, const void *params, int M, bool ell_f64, void *value, void *elbo) {
  by_dtype(c, [&](auto t) { sg_stats_impl<decltype(t)>(c, params, M, ell_f64, value, elbo); });
}

void launch_sg_scale(mivi_ctx *c, int M) {
  const int Mr = (M + 63) / 64 * 64;   // (<= MP: the solves read whole blocks of up to 64 columns)
  const dim3 grid((c->dP + 255) / 256, Mr);
  const double *w = (const double *)c->sg_d.p + 2 * (size_t)c->sg_cap;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_sg_scale<T>, grid, dim3(256), 0, c->stream, c->cfg.d, c->dP, M, (const T *)c->eps[0].p, w, (T *)c->sg_S.p, (T *)c->W.p);
  });
}

void launch_sg_mf_grad(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *grad) {
  const int d = c->cfg.d, d4 = (d + 3) / 4;
  const dim3 grid((d4 + 15) / 16);
  const double *w = (const double *)c->sg_d.p + 2 * (size_t)c->sg_cap;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_sg_mf_grad<T>, grid, dim3(256), 0, c->stream, d, M, (const T *)params, rng, w, (T *)grad);
  });
}

}  // namespace mivi
