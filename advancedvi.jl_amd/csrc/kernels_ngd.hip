// The square-root natural-gradient update of KLMinSqrtNaturalGradDescent (src/algorithms/klminsqrtnaturalgraddescent.jl:108-119):
//     A  = C' (-H) C - I                     T = tril(A) - diag(A) / 2
//     m' = m - eta C (C' (-g))               C' = C - eta C T               entropy(q') = d/2 (1 + log 2 pi) + sum_i log C'_ii
// H is used as it comes (not symmetrised, not transposed); only the lower triangle of A is formed; C' has exact zeros above the
// diagonal; g and H are read-only.
//
// d <= kNgdSmallD: ONE workgroup keeps C, H and A in LDS and does the whole update in one launch (k_ngd_small; the reference's own tests
// and benchmark run at d = 5 .. 10).  Above it: three launches of 64 x 64 output tiles on the matrix cores, operands staged through LDS in
// K chunks of 32 (f32: v_mfma_f32_32x32x2_f32, exact f32 inputs; f64: v_mfma_f64_16x16x4_f64), evaluated as C' ((-H) C):
//     stage 1   G = -(H C)      lower tiles (ti >= tj) only, K from tile tj on (C is lower triangular);  riders: every tile workgroup copies
//                               its tile of tril(C) into the padded second buffer Cc, trailing workgroups form v = C' (-g)
//     stage 2   A = Cc' G - I   lower tiles, K from tile ti on;  epilogue: T = tril(A) - diag(A) / 2;  trailing workgroups: m' = m - eta Cc v
//     stage 3   C' = Cc - eta Cc T   lower tiles, K over tiles tj .. ti; written into the parameter vector (stages 2 and 3 read the copy Cc,
//                               so no tile reads what another one has overwritten), the mirrored strictly-upper entries as zeros;  epilogue
//                               of the diagonal tiles: sum_i log C'_ii and the count of C'_ii that are not positive finite numbers; the last
//                               diagonal tile to finish (an integer ticket) adds the nT partials in tile order and writes entropy / elbo / flags
// All buffers between the stages are padded to whole tiles (ld = 64 nT) and hold zeros in the padding, so no tile masks its operands except
// where it reads the caller's unpadded g, H and parameters.  No floating-point atomics; every sum has one fixed order.
#include "mivi_internal.h"
#include "ngd_tile.h"

namespace mivi {

constexpr int kNgdSmallD = 48;   // 3 matrices of 48 x 49 doubles = 55 KB of LDS

template <typename T>
struct NgdArgs {
  int d, nT, ldp;
  T *params;            // [m (d); vec C (d x d, column-major)] in / out
  const T *grad;        // g (d)
  const T *hess;        // H (d x d, column-major)
  T *Cc, *G, *Tm;       // ldp x ldp each: tril(C) copy, -(H C), T
  T *v;                 // ldp: C' (-g)
  double *part;         // [2][nT]: sum log C'_ii of a diagonal tile, count of bad C'_ii
  unsigned *ticket;
  double eta;
  const T *logpi;       // nullable: elbo = *logpi + entropy(q')
  T *entropy_out;       // nullable
  T *elbo_out;          // nullable
  int *status;          // bit 0: entropy / elbo not finite, bit 1: a C'_ii that is not a positive finite number
};

__device__ __forceinline__ bool ngd_bad_diag(double c) { return !(c > 0.0) || !isfinite(c); }

template <typename T>
__device__ __forceinline__ void ngd_finish(const NgdArgs<T> &a, double logsum, int bad) {
  const double ent = 0.5 * (double)a.d * (1.0 + kLog2Pi) + logsum;
  const T ent_t = (T)ent;
  if (a.entropy_out) *a.entropy_out = ent_t;
  bool finite = isfinite((double)ent_t);
  if (a.elbo_out) {
    const T e = (a.logpi ? *a.logpi : T(0)) + ent_t;
    *a.elbo_out = e;
    finite = finite && isfinite((double)e);
  }
  const int bits = (bad ? 2 : 0) | (finite ? 0 : 1);
  if (bits) atomicOr(a.status, bits);
}

// ---- d <= kNgdSmallD: one workgroup, everything in LDS ------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_ngd_small(NgdArgs<T> a) {
  constexpr int LD = kNgdSmallD + 1;
  __shared__ T sC[kNgdSmallD * LD], sH[kNgdSmallD * LD], sA[kNgdSmallD * LD];
  __shared__ T sv[kNgdSmallD];
  __shared__ double slog[kNgdSmallD];
  __shared__ int sbad[kNgdSmallD];
  const int d = a.d, tid = threadIdx.x;
  const T *Cg = a.params + d;
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    sC[i * LD + j] = i >= j ? Cg[t] : T(0);
    sH[i * LD + j] = a.hess[t];
  }
  __syncthreads();
  // G = -(H C), lower triangle:  G_ij = -sum_{k >= j} H_ik C_kj
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    if (i < j) continue;
    T s = T(0);
    for (int k = j; k < d; ++k) s += sH[i * LD + k] * sC[k * LD + j];
    sA[i * LD + j] = -s;
  }
  // v = C' (-g)
  if (tid < d) {
    T s = T(0);
    for (int k = tid; k < d; ++k) s += sC[k * LD + tid] * -a.grad[k];
    sv[tid] = s;
  }
  __syncthreads();
  // T = tril(A) - diag(A) / 2 with A_ij = sum_{k >= i} C_ki G_kj - delta_ij (j <= i); kept where H was
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    T r = T(0);
    if (i >= j) {
      T s = T(0);
      for (int k = i; k < d; ++k) s += sC[k * LD + i] * sA[k * LD + j];
      r = i == j ? (s - T(1)) / T(2) : s;
    }
    sH[i * LD + j] = r;
  }
  __syncthreads();
  const T eta = (T)a.eta;
  for (int t = tid; t < d * d; t += 256) {
    const int i = t % d, j = t / d;
    T r = T(0);
    if (i >= j) {
      T s = T(0);
      for (int k = j; k <= i; ++k) s += sC[i * LD + k] * sH[k * LD + j];
      r = sC[i * LD + j] - eta * s;
    }
    a.params[d + t] = r;
    if (i == j) {
      slog[i] = log((double)r);
      sbad[i] = ngd_bad_diag((double)r) ? 1 : 0;
    }
  }
  if (tid < d) {
    T s = T(0);
    for (int j = 0; j <= tid; ++j) s += sC[tid * LD + j] * sv[j];
    a.params[tid] = a.params[tid] - eta * s;
  }
  __syncthreads();
  if (tid == 0) {
    double ls = 0.0;
    int bad = 0;
    for (int i = 0; i < d; ++i) { ls += slog[i]; bad += sbad[i]; }
    ngd_finish(a, ls, bad);
  }
}

// ---- the tile products: NgdFrag<T> and ngd_tile_of (ngd_tile.h) ----------------------------------------------------------------------------

// STAGE 1: G = -(H C); 2: T from A = Cc' G - I; 3: C' = Cc - eta Cc T
template <typename T, int STAGE>
__global__ __launch_bounds__(256) void k_ngd_stage(NgdArgs<T> a) {
  __shared__ T sA[kNgdKC * kNgdLd], sB[kNgdKC * kNgdLd];
  __shared__ double sred[4 * kNgdTile];
  __shared__ int slast;
  const int d = a.d, nT = a.nT, ldp = a.ldp, tid = threadIdx.x;
  const int n_tiles = nT * (nT + 1) / 2;
  const T *Cg = a.params + d;
  if ((int)blockIdx.x >= n_tiles) {   // riders (stages 1 and 2 only)
    const int b = blockIdx.x - n_tiles;
    if (STAGE == 1) {
      // v_j = -sum_{k >= j} C_kj g_k for the 64 columns of tile b: one wave per column, lanes along k, a fixed shuffle tree
      const int lane = tid & 63, w = tid >> 6;
      for (int jj = w; jj < kNgdTile; jj += 4) {
        const int j = b * kNgdTile + jj;
        double s = 0.0;
        if (j < d)
          for (int k = j + lane; k < d; k += 64) s += (double)Cg[(size_t)j * d + k] * (double)a.grad[k];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o, 64);
        if (lane == 0) a.v[j] = j < d ? (T)(-s) : T(0);
      }
    } else if (STAGE == 2) {
      // m'_i = m_i - eta sum_{j <= i} Cc_ij v_j for the 64 rows of tile b: four partial sums per row (j mod 4), added in order
      const int r = tid & 63, q = tid >> 6, i = b * kNgdTile + r;
      double s = 0.0;
      if (i < d)
        for (int j = q; j <= i; j += 4) s += (double)a.Cc[(size_t)j * ldp + i] * (double)a.v[j];
      sred[q * kNgdTile + r] = s;
      __syncthreads();
      if (q == 0 && i < d) {
        const double tot = ((sred[r] + sred[kNgdTile + r]) + sred[2 * kNgdTile + r]) + sred[3 * kNgdTile + r];
        a.params[i] = a.params[i] - (T)a.eta * (T)tot;
      }
    }
    return;
  }
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  const int lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6), wr = w >> 1, wc = w & 1;
  const int kt_beg = STAGE == 1 ? tj : (STAGE == 2 ? ti : tj);
  const int kt_end = STAGE == 3 ? ti + 1 : nT;   // K tiles [kt_beg, kt_end)
  const int k_beg = kt_beg * kNgdTile, k_end = kt_end * kNgdTile;

  // operand elements of one K chunk, 8 per thread and operand.  "row-fast" (the tile's 64 rows are contiguous in memory): thread -> (i = tid & 63,
  // k = (tid >> 6) + 4 r); "k-fast" (K is contiguous): thread -> (k = tid & 31, i = (tid >> 5) + 8 r)
  T ra[8], rb[8];
  auto load = [&](int k0) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (STAGE == 1) {   // A_ik = H_ik (the caller's, ld d): row-fast;  B_kj = tril(C)_kj (the caller's): k-fast
        const int i = i0 + (tid & 63), k = k0 + (tid >> 6) + 4 * r;
        ra[r] = (i < d && k < d) ? a.hess[(size_t)k * d + i] : T(0);
        const int kb = k0 + (tid & 31), j = j0 + (tid >> 5) + 8 * r;
        rb[r] = (kb < d && j < d && kb >= j) ? Cg[(size_t)j * d + kb] : T(0);
      } else if (STAGE == 2) {   // A_ik = Cc_ki: k-fast;  B_kj = G_kj: k-fast
        const int k = k0 + (tid & 31), x = (tid >> 5) + 8 * r;
        ra[r] = a.Cc[(size_t)(i0 + x) * ldp + k];
        rb[r] = a.G[(size_t)(j0 + x) * ldp + k];
      } else {   // A_ik = Cc_ik: row-fast;  B_kj = T_kj: k-fast
        const int i = i0 + (tid & 63), k = k0 + (tid >> 6) + 4 * r;
        ra[r] = a.Cc[(size_t)k * ldp + i];
        const int kb = k0 + (tid & 31), j = j0 + (tid >> 5) + 8 * r;
        rb[r] = a.Tm[(size_t)j * ldp + kb];
      }
    }
  };
  auto stash = [&]() {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      if (STAGE == 2) sA[(tid & 31) * kNgdLd + (tid >> 5) + 8 * r] = ra[r];
      else sA[((tid >> 6) + 4 * r) * kNgdLd + (tid & 63)] = ra[r];
      sB[(tid & 31) * kNgdLd + (tid >> 5) + 8 * r] = rb[r];
    }
  };

  if (STAGE == 1) {   // rider: this workgroup's tile of tril(C) -> Cc (zeros in the padding and above the diagonal)
    for (int t = tid; t < kNgdTile * kNgdTile; t += 256) {
      const int i = i0 + (t & 63), j = j0 + (t >> 6);
      a.Cc[(size_t)j * ldp + i] = (i < d && j < d && i >= j) ? Cg[(size_t)j * d + i] : T(0);
    }
  }

  NgdFrag<T> acc;
  acc.zero();
  load(k_beg);
  for (int k0 = k_beg; k0 < k_end; k0 += kNgdKC) {
    stash();
    __syncthreads();
    if (k0 + kNgdKC < k_end) load(k0 + kNgdKC);
    acc.chunk(sA, sB, wr, wc, lane);
    __syncthreads();
  }

  if (STAGE == 1) {
    acc.each(wr, wc, lane, [&](int ii, int jj, T x) { a.G[(size_t)(j0 + jj) * ldp + i0 + ii] = -x; });
  } else if (STAGE == 2) {
    acc.each(wr, wc, lane, [&](int ii, int jj, T x) {
      const int i = i0 + ii, j = j0 + jj;
      const T t = i > j ? x : (i == j ? (x - T(1)) / T(2) : T(0));
      a.Tm[(size_t)j * ldp + i] = (i < d && j < d) ? t : T(0);
    });
  } else {
    const T eta = (T)a.eta;
    const bool diag = ti == tj;
    acc.each(wr, wc, lane, [&](int ii, int jj, T x) {
      const int i = i0 + ii, j = j0 + jj;
      if (i >= d || j >= d) return;
      if (i >= j) {
        const T r = a.Cc[(size_t)j * ldp + i] - eta * x;
        a.params[d + (size_t)j * d + i] = r;
        if (i == j) {
          sred[ii] = log((double)r);
          sred[kNgdTile + ii] = ngd_bad_diag((double)r) ? 1.0 : 0.0;
        }
        if (i > j) a.params[d + (size_t)i * d + j] = T(0);
      }
    });
    if (diag) {   // (uniform per workgroup)
      __syncthreads();
      if (tid == 0) {
        const int n = d - i0 < kNgdTile ? d - i0 : kNgdTile;
        double ls = 0.0, nb = 0.0;
        for (int r = 0; r < n; ++r) { ls += sred[r]; nb += sred[kNgdTile + r]; }
        __hip_atomic_store(&a.part[ti], ls, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_store(&a.part[nT + ti], nb, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __threadfence();
        const unsigned t = __hip_atomic_fetch_add(a.ticket, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
        slast = t == (unsigned)(nT - 1);
        if (slast) {
          __threadfence();
          double tot = 0.0, bad = 0.0;
          for (int b = 0; b < nT; ++b) {
            tot += __hip_atomic_load(&a.part[b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            bad += __hip_atomic_load(&a.part[nT + b], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          }
          ngd_finish(a, tot, bad > 0.0 ? 1 : 0);
        }
      }
    }
  }
}

template <typename T>
static void launch_ngd_t(mivi_ctx *c, void *params, const void *grad, const void *hess, double eta, const void *logpi, void *entropy, void *elbo) {
  NgdArgs<T> a{};
  a.d = c->cfg.d;
  a.nT = (a.d + kNgdTile - 1) / kNgdTile;
  a.ldp = a.nT * kNgdTile;
  a.params = (T *)params;
  a.grad = (const T *)grad;
  a.hess = (const T *)hess;
  a.eta = eta;
  a.logpi = (const T *)logpi;
  a.entropy_out = (T *)entropy;
  a.elbo_out = (T *)elbo;
  a.status = (int *)c->status.p;
  if (a.d <= kNgdSmallD) {
    hipLaunchKernelGGL(k_ngd_small<T>, dim3(1), dim3(256), 0, c->stream, a);
    return;
  }
  const size_t mat = (size_t)a.ldp * a.ldp;
  T *w = (T *)c->ngd_work.p;
  a.Cc = w;
  a.G = w + mat;
  a.Tm = w + 2 * mat;
  a.v = w + 3 * mat;
  a.part = (double *)c->ngd_part.p;
  a.ticket = (unsigned *)((double *)c->ngd_part.p + 2 * a.nT);
  const int n_tiles = a.nT * (a.nT + 1) / 2;
  // the ticket starts every update at zero whatever became of the update before it (a stage 3 that never ran to its end would leave it counted up)
  (void)hipMemsetAsync(a.ticket, 0, sizeof(unsigned), c->stream);
  hipLaunchKernelGGL((k_ngd_stage<T, 1>), dim3(n_tiles + a.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_ngd_stage<T, 2>), dim3(n_tiles + a.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_ngd_stage<T, 3>), dim3(n_tiles), dim3(256), 0, c->stream, a);
}

size_t ngd_work_bytes(const mivi_ctx *c) {
  if (c->cfg.d <= kNgdSmallD) return 0;
  const size_t ldp = (size_t)((c->cfg.d + kNgdTile - 1) / kNgdTile) * kNgdTile;
  return (3 * ldp * ldp + ldp) * c->esize;
}

size_t ngd_part_bytes(const mivi_ctx *c) {
  if (c->cfg.d <= kNgdSmallD) return 0;
  const size_t nT = (size_t)((c->cfg.d + kNgdTile - 1) / kNgdTile);
  return (2 * nT + 2) * sizeof(double);
}

void launch_ngd_update(mivi_ctx *c, void *params, const void *grad, const void *hess, double eta, const void *logpi, void *entropy, void *elbo) {
  if (c->cfg.dtype == MIVI_F32) launch_ngd_t<float>(c, params, grad, hess, eta, logpi, entropy, elbo);
  else launch_ngd_t<double>(c, params, grad, hess, eta, logpi, entropy, elbo);
}

}  // namespace mivi
