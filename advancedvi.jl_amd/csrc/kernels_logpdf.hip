// Distributions.logpdf(q, z) at the caller's points (mivi_logpdf; api_logpdf.hip drives these kernels): src/families/location_scale.jl:59-63,
// src/families/location_scale_low_rank.jl:45-68.  log q(z) = sum_i log phi(u_i) - log det C with u = C^-1 (z - mu), phi the context's base.
//   k_lp_logdet   sum_i log C_ii in f64 and the non-positive-scale flag, once per call (mean-field and full-rank)
//   k_lp_mf       mean-field: one wave per column streams u = (z - mu) / sigma, sums log phi(u) in f64
//   k_lp_fwd16    full-rank: the forward block substitution C X = Z - mu, the left-looking mirror of k_stl_solve_la16 (kernels_fullrank.hip).
//                 A workgroup owns 16 columns of Z and walks the 32-row block rows of C top down:
//                     X_b = Dinv_b (R_b - sum_{j<b} C(b, j) X_j),   Dinv_b = C_bb^-1 from k_stl_prep's diagonal workgroups (launch_stl_dinv32)
//                 Only the term j = b - 1 needs the block solved just before, so wave 0 is the sequential chain (that term, the right-hand side,
//                 the product with Dinv_b) while waves 1 .. NW-1 already accumulate the terms j < b of block row b + 1: one barrier per block
//                 row.  Every product is v_mfma_f64_16x16x4_f64 on operands stored in the element type: the products of f32 operands are
//                 exact and every sum -- the off-diagonal terms, R = z - mu, the product with Dinv_b -- is accumulated in f64; X is kept in f64
//                 and rounded to the element type once, on its way out.  (A column may hold one huge standardised value -- the Student-t bases
//                 draw them -- and every later row then cancels large terms down to O(1): sums or an X in f32 lose those rows.  DESIGN.md
//                 section 8 has the figures.)  C's 32 x 32 units are read straight from the
//                 parameter vector (the A operand's lanes run along a column of C: no transposed copy).  X stays in LDS while 16 columns of
//                 it fit beside the partials (XLDS); past that it lives in the workgroup's own 16 columns of an f64 scratch of a chunk's shape,
//                 which its waves re-read through their CU's L1.  There is no size at which the kernel does not run.  The tail
//                 sums log phi(u) per column in f64.
//   k_lp_lowr_t   low-rank: t = D^-1 (z - m), what k_lowr_s / k_lowr_xv (kernels_lowrank.hip) take in place of the estimators' own t
//   k_lp_store    low-rank: the f64 log q of the Woodbury stage -> the element type
// No floating-point atomics, one summation order: results are bitwise repeatable.
#include "device_common.h"

namespace mivi {

// -log phi(u) without its constant (LpBase::c0), evaluated in f64 from the element-type u
struct LpBase {
  int base;
  double nu, c0;   // TDist's degrees of freedom; -(constant of log phi) per element
};
__device__ __forceinline__ double lp_neg_logphi_var(const LpBase &b, double u) {
  if (b.base == MIVI_BASE_LAPLACE) return fabs(u);
  if (b.base == MIVI_BASE_TDIST) return 0.5 * (b.nu + 1.0) * log1p(u * u / b.nu);
  return 0.5 * u * u;
}

// scal[0] = sum_i log diag[i * stride] (f64); a diagonal entry that is not a positive finite number sets status bit 1
template <typename T>
__global__ __launch_bounds__(256) void k_lp_logdet(int d, const T *__restrict__ diag, size_t stride, double *__restrict__ scal, int *status) {
  __shared__ double red[2 * 4];
  double v[2] = {0.0, 0.0};
  for (int i = threadIdx.x; i < d; i += 256) {
    const double c = (double)diag[(size_t)i * stride];
    if (!(c > 0.0) || !isfinite(c)) v[1] = 1.0;
    v[0] += log(c);
  }
  block_sum_n<double, 256, 2>(v, red);
  if (threadIdx.x == 0) {
    scal[0] = v[0];
    if (v[1] > 0.0 && status) atomicOr(status, 2);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_lp_mf(int d, int n, const T *__restrict__ params, const T *__restrict__ Z, T *__restrict__ logq,
                                               T *__restrict__ std, const double *__restrict__ scal, LpBase bs) {
  const int lane = threadIdx.x & 63;
  const long long m = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (m >= n) return;
  const T *z = Z + (size_t)m * d;
  double s = 0.0;
  for (int i = lane; i < d; i += 64) {
    const T u = (z[i] - params[i]) / params[d + i];
    if (std) std[(size_t)m * d + i] = u;
    s += lp_neg_logphi_var(bs, (double)u);
  }
  s = wave_sum(s);
  if (lane == 0) logq[m] = (T)(-(s + d * bs.c0) - scal[0]);
}

// LDS of k_lp_fwd16, all f64: [partials: 2 x (NW-1) x 512] [the chain's right-hand side: 512] [X: 16 dP (XLDS)]
constexpr int kLpNW = 4;
static size_t lp_fwd_lds_bytes(int dP, bool xlds) { return (2 * (kLpNW - 1) * 512 + 512 + (xlds ? (size_t)dP * 16 : 0)) * sizeof(double); }

template <typename T, int NW, bool XLDS>
__global__ __launch_bounds__(NW * 64) void k_lp_fwd16(int d, int n, const T *__restrict__ params, const T *__restrict__ Z, const T *__restrict__ Dinv,
                                                      T *__restrict__ logq, T *__restrict__ std, double *__restrict__ xg,
                                                      const double *__restrict__ scal, LpBase bs) {
  typedef Mfma16<double> MM;
  typedef MM::acc_t acc4;
  extern __shared__ __attribute__((aligned(16))) char smem_raw[];
  const int nb = (d + 31) >> 5, dP = nb * 32;
  double *part = (double *)smem_raw;                      // part[parity][w - 1][8 * 64]: the bulk of block row b from wave w, parity b & 1
  double *rb = part + 2 * (NW - 1) * 512;                 // rb[k * 16 + m]: R_b - S_b, the B operand of the product with Dinv_b
  double *x = rb + 512;                                   // XLDS: x[k * 16 + m], k < dP -- z until block row k / 32 is solved, then X
  const int tid = threadIdx.x, lane = tid & 63, c16 = lane & 15, kq = lane >> 4;
  const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
  const long long m0 = (long long)blockIdx.x * 16;
  const T *C = params + d;
  // X(k, m) of this workgroup's 16 columns, f64: LDS, or the workgroup's own columns of the scratch xg (d x n; rows >= d and columns >= n
  // do not exist there: they read 0)
  auto ldx = [&](int k, int m) -> double {
    if (XLDS) return x[k * 16 + m];
    return (k < d && m0 + m < n) ? xg[(size_t)(m0 + m) * d + k] : 0.0;
  };
  auto stx = [&](int k, int m, double v) {
    if (XLDS) x[k * 16 + m] = v;
    else if (k < d && m0 + m < n) xg[(size_t)(m0 + m) * d + k] = v;
  };
  // z into X's place, exact (lanes along k: coalesced); mu is taken off in f64 where the right-hand side is formed
  for (int t = tid; t < dP * 16; t += NW * 64) {
    const int k = t % dP, m = t / dP;
    const bool in = k < d && m0 + m < n;
    if (XLDS) x[k * 16 + m] = in ? (double)Z[(size_t)(m0 + m) * d + k] : 0.0;
    else if (in) xg[(size_t)(m0 + m) * d + k] = (double)Z[(size_t)(m0 + m) * d + k];
  }
  for (int t = tid; t < 2 * (NW - 1) * 512; t += NW * 64) part[t] = 0.0;   // (block rows 0 and 1 have no bulk)
  __syncthreads();
  // acc0 / acc1 (rows 0..15 / 16..31 of block row brow) += C(brow, j) X_j: A[row = 16 hb + c16][k = 4 g + kq] = C[32 brow + row, 32 j + k]
  auto unit = [&](int brow, int j, acc4 &acc0, acc4 &acc1) {
    const int r0 = brow * 32 + c16, r1 = r0 + 16;
    const T *Acol = C + (size_t)(j * 32 + kq) * d;
    T av[16];
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      av[2 * g] = r0 < d ? Acol[(size_t)(4 * g) * d + r0] : T(0);
      av[2 * g + 1] = r1 < d ? Acol[(size_t)(4 * g) * d + r1] : T(0);
    }
#pragma unroll
    for (int g = 0; g < 8; ++g) {
      const double bv = ldx(j * 32 + 4 * g + kq, c16);
      acc0 = MM::mma((double)av[2 * g], bv, acc0);
      acc1 = MM::mma((double)av[2 * g + 1], bv, acc1);
    }
  };
  for (int b = 0; b < nb; ++b) {
    if (w == 0) {
      // ---- the sequential chain: the term j = b - 1, R_b - S_b, X_b = Dinv_b (R_b - S_b) ----
      T dv[16];   // A[i = 16 hb + c16][k = 4 g + kq] = Dinv_b[i, k], stored at [k + 32 i]
      const T *Di = Dinv + (size_t)b * 1024 + kq + 32 * c16;
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        dv[2 * g] = Di[4 * g];
        dv[2 * g + 1] = Di[4 * g + 32 * 16];
      }
      double mu0[4], mu1[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int k0 = b * 32 + MM::row(kq, r), k1 = k0 + 16;
        mu0[r] = k0 < d ? (double)params[k0] : 0.0;
        mu1[r] = k1 < d ? (double)params[k1] : 0.0;
      }
      acc4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
      if (b > 0) unit(b, b - 1, acc0, acc1);
      const double *pb = part + (size_t)(b & 1) * (NW - 1) * 512;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = MM::row(kq, r);
        double s0 = acc0[r], s1 = acc1[r];
        for (int ww = 0; ww < NW - 1; ++ww) {
          s0 += pb[ww * 512 + r * 64 + lane];
          s1 += pb[ww * 512 + (4 + r) * 64 + lane];
        }
        rb[row * 16 + c16] = (ldx(b * 32 + row, c16) - mu0[r]) - s0;
        rb[(row + 16) * 16 + c16] = (ldx(b * 32 + 16 + row, c16) - mu1[r]) - s1;
      }
      // rb goes from lane to lane of this one wave: its stores are released to the wave and no load is moved in front of them
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_wave_barrier();
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      acc4 xa0 = {0, 0, 0, 0}, xa1 = {0, 0, 0, 0};
#pragma unroll
      for (int g = 0; g < 8; ++g) {
        const double bv = rb[(4 * g + kq) * 16 + c16];
        xa0 = MM::mma((double)dv[2 * g], bv, xa0);
        xa1 = MM::mma((double)dv[2 * g + 1], bv, xa1);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        stx(b * 32 + MM::row(kq, r), c16, xa0[r]);
        stx(b * 32 + 16 + MM::row(kq, r), c16, xa1[r]);
      }
    } else if (b + 1 < nb) {
      // ---- the bulk of block row b + 1: units j < b dealt to waves 1 .. NW-1 ----
      acc4 acc0 = {0, 0, 0, 0}, acc1 = {0, 0, 0, 0};
      for (int j = w - 1; j < b; j += NW - 1) unit(b + 1, j, acc0, acc1);
      double *pn = part + ((size_t)((b + 1) & 1) * (NW - 1) + (w - 1)) * 512;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        pn[r * 64 + lane] = acc0[r];
        pn[(4 + r) * 64 + lane] = acc1[r];
      }
    }
    __syncthreads();
  }
  // ---- the tail: sum_i log phi(u_i) per column from the f64 X (one wave per column, lanes along i), and u rounded to the element type ----
  for (int m = w; m < 16; m += NW) {
    if (m0 + m >= n) break;
    double s = 0.0;
    for (int k = lane; k < d; k += 64) {
      const double u = ldx(k, m);
      s += lp_neg_logphi_var(bs, u);
      if (std) std[(size_t)(m0 + m) * d + k] = (T)u;
    }
    s = wave_sum(s);
    if (lane == 0) logq[m0 + m] = (T)(-(s + d * bs.c0) - scal[0]);
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_lp_lowr_t(int d, int n, const T *__restrict__ params, const T *__restrict__ Z, T *__restrict__ tbuf) {
  const size_t total = (size_t)d * n;
  for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
    const int i = (int)(t % d);
    tbuf[t] = (Z[t] - params[i]) / params[d + i];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_lp_store(int n, const double *__restrict__ lq, T *__restrict__ logq) {
  const int m = blockIdx.x * 256 + threadIdx.x;
  if (m < n) logq[m] = (T)lq[m];
}

// ---- launchers (n <= kSampleChunk columns per call) ------------------------------------------------------------------------------------
static LpBase lp_base_of(const mivi_ctx *c) {
  return LpBase{c->base, c->base_nu, c->base == MIVI_BASE_NORMAL ? 0.5 * kLog2Pi : c->base_c0};
}

void launch_lp_logdet(mivi_ctx *c, const void *params, double *scal) {
  const int d = c->cfg.d;
  const size_t stride = c->cfg.family == MIVI_FULLRANK ? (size_t)d + 1 : 1;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_lp_logdet<T>, dim3(1), dim3(256), 0, c->stream, d, (const T *)params + d, stride, scal, (int *)c->status.p);
  });
}

void launch_lp_mf(mivi_ctx *c, const void *params, const void *Z, int n, void *logq, void *std, const double *scal) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_lp_mf<T>, dim3((n + 3) / 4), dim3(256), 0, c->stream, c->cfg.d, n, (const T *)params, (const T *)Z, (T *)logq, (T *)std, scal,
                       lp_base_of(c));
  });
}

bool lp_fwd_x_in_lds(const mivi_ctx *c) { return lp_fwd_lds_bytes((c->cfg.d + 31) / 32 * 32, true) <= 160 * 1024; }

// xg: the f64 d x n home of X when it does not stay in LDS (lp_fwd_x_in_lds false; not read otherwise)
void launch_lp_fwd(mivi_ctx *c, const void *params, const void *Z, int n, const void *Dinv, void *logq, void *std, double *xg, const double *scal) {
  const int d = c->cfg.d, dP = (d + 31) / 32 * 32;
  const bool xlds = lp_fwd_x_in_lds(c);
  const size_t sh = lp_fwd_lds_bytes(dP, xlds);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    auto go = [&](auto kern) {
      if (sh > 64 * 1024) (void)hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize, (int)sh);
      hipLaunchKernelGGL(kern, dim3((n + 15) / 16), dim3(kLpNW * 64), sh, c->stream, d, n, (const T *)params, (const T *)Z, (const T *)Dinv, (T *)logq, (T *)std,
                         xg, scal, lp_base_of(c));
    };
    if (xlds) go(&k_lp_fwd16<T, kLpNW, true>);
    else go(&k_lp_fwd16<T, kLpNW, false>);
  });
}

void launch_lp_lowr_t(mivi_ctx *c, const void *params, const void *Z, int n, void *tbuf) {
  const size_t total = (size_t)c->cfg.d * n;
  const unsigned grid = (unsigned)((total + 255) / 256 < 4096 ? (total + 255) / 256 : 4096);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_lp_lowr_t<T>, dim3(grid), dim3(256), 0, c->stream, c->cfg.d, n, (const T *)params, (const T *)Z, (T *)tbuf);
  });
}

void launch_lp_store(mivi_ctx *c, int n, const double *lq, void *logq) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_lp_store<T>, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, lq, (T *)logq);
  });
}

}  // namespace mivi
