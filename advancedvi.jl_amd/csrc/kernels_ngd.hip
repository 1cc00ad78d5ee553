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
// The chunked tile product, the riders' column-dot and row-matvec bodies, the tile geometry and the finish (entropy / elbo / flags) are
// ngd_tile.h's, shared with kernels_natgrad.hip, as is the context's scratch pair (ms_work, ms_part).
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
  NgdOut<T> out;        // entropy / elbo / flags (ngd_tile.h)
};

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
      sbad[i] = ngd_bad((double)r) ? 1 : 0;
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
    ngd_finish(d, ls, bad, a.out);
  }
}

// ---- the tile products: NgdFrag<T>, ngd_product and ngd_tile_of (ngd_tile.h) ---------------------------------------------------------------

// STAGE 1: G = -(H C); 2: T from A = Cc' G - I; 3: C' = Cc - eta Cc T
template <typename T, int STAGE>
__global__ __launch_bounds__(256) void k_ngd_stage(NgdArgs<T> a) {
  __shared__ T sA[kNgdKC * kNgdLd], sB[kNgdKC * kNgdLd];
  __shared__ double sred[4 * kNgdTile];
  __shared__ int slast;
  const int d = a.d, nT = a.nT, ldp = a.ldp, tid = threadIdx.x;
  const int n_tiles = ngd_n_tiles(nT);
  const T *Cg = a.params + d;
  if ((int)blockIdx.x >= n_tiles) {   // riders (stages 1 and 2 only), on the 64 columns / rows of tile b
    const int b = blockIdx.x - n_tiles;
    if (STAGE == 1)   // v_j = -sum_{k >= j} C_kj g_k
      ngd_col_dots(Cg, d, a.grad, b, d, [&](int j, double s) { a.v[j] = j < d ? (T)(-s) : T(0); });
    else if (STAGE == 2)   // m'_i = m_i - eta sum_{j <= i} Cc_ij v_j
      ngd_row_matvec(
          b, d, false, sred, [&](int i, int j) { return (double)a.Cc[(size_t)j * ldp + i] * (double)a.v[j]; },
          [&](int i, double tot) { a.params[i] = a.params[i] - (T)a.eta * (T)tot; });
    return;
  }
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  NGD_WAVE;
  const int kt_beg = STAGE == 1 ? tj : (STAGE == 2 ? ti : tj);
  const int kt_end = STAGE == 3 ? ti + 1 : nT;   // K tiles [kt_beg, kt_end)
  const int k_beg = kt_beg * kNgdTile, k_end = kt_end * kNgdTile;

  NgdFrag<T> acc;
  acc.zero();
  if (STAGE == 1) {
    // rider: this workgroup's tile of tril(C) -> Cc (zeros in the padding and above the diagonal)
    for (int t = tid; t < kNgdTile * kNgdTile; t += 256) {
      const int i = i0 + (t & 63), j = j0 + (t >> 6);
      a.Cc[(size_t)j * ldp + i] = (i < d && j < d && i >= j) ? Cg[(size_t)j * d + i] : T(0);
    }
    // A_ik = H_ik, row-fast;  B_kj = tril(C)_kj, k-fast: the caller's unpadded buffers (ld d), masked
    ngd_product<T, false, true>(
        acc, [&](int x, int k) { return (i0 + x < d && k < d) ? a.hess[(size_t)k * d + i0 + x] : T(0); },
        [&](int y, int k) { return (k < d && j0 + y < d && k >= j0 + y) ? Cg[(size_t)(j0 + y) * d + k] : T(0); }, k_beg, k_end, sA, sB);
  } else if (STAGE == 2) {   // A_ik = Cc_ki, B_kj = G_kj: both k-fast
    ngd_product<T, true, true>(acc, a.Cc + (size_t)i0 * ldp, ldp, a.G + (size_t)j0 * ldp, ldp, k_beg, k_end, sA, sB);
  } else {   // A_ik = Cc_ik, row-fast;  B_kj = T_kj, k-fast
    ngd_product<T, false, true>(acc, a.Cc + i0, ldp, a.Tm + (size_t)j0 * ldp, ldp, k_beg, k_end, sA, sB);
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
          sred[kNgdTile + ii] = ngd_bad((double)r) ? 1.0 : 0.0;
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
          ngd_finish(d, tot, bad > 0.0 ? 1 : 0, a.out);
        }
      }
    }
  }
}

template <typename T>
static void launch_ngd_t(mivi_ctx *c, void *params, const void *grad, const void *hess, double eta, const void *logpi, void *entropy, void *elbo) {
  const NgdGeom g(c->cfg.d);
  NgdArgs<T> a{};
  a.d = c->cfg.d;
  a.nT = g.nT;
  a.ldp = g.ldp;
  a.params = (T *)params;
  a.grad = (const T *)grad;
  a.hess = (const T *)hess;
  a.eta = eta;
  a.out = NgdOut<T>{(const T *)logpi, (T *)entropy, (T *)elbo, (int *)c->status.p};
  if (a.d <= kNgdSmallD) {
    hipLaunchKernelGGL(k_ngd_small<T>, dim3(1), dim3(256), 0, c->stream, a);
    return;
  }
  T *w = (T *)c->ms_work.p;
  a.Cc = w;
  a.G = w + g.mat();
  a.Tm = w + 2 * g.mat();
  a.v = w + 3 * g.mat();
  a.part = (double *)c->ms_part.p;
  a.ticket = (unsigned *)(a.part + 2 * g.nT);
  // the ticket starts every update at zero whatever became of the update before it (a stage 3 that never ran to its end would leave it counted
  // up) and whatever the natural-gradient update, which shares the scratch, has left in its place
  (void)hipMemsetAsync(a.ticket, 0, sizeof(unsigned), c->stream);
  hipLaunchKernelGGL((k_ngd_stage<T, 1>), dim3(g.n_tiles + g.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_ngd_stage<T, 2>), dim3(g.n_tiles + g.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_ngd_stage<T, 3>), dim3(g.n_tiles), dim3(256), 0, c->stream, a);
}

size_t ngd_work_bytes(const mivi_ctx *c) {
  const NgdGeom g(c->cfg.d);
  return c->cfg.d <= kNgdSmallD ? 0 : (3 * g.mat() + g.ldp) * c->esize;
}

size_t ngd_part_bytes(const mivi_ctx *c) { return c->cfg.d <= kNgdSmallD ? 0 : (2 * (size_t)NgdGeom(c->cfg.d).nT + 2) * sizeof(double); }

void launch_ngd_update(mivi_ctx *c, void *params, const void *grad, const void *hess, double eta, const void *logpi, void *entropy, void *elbo) {
  by_dtype(c, [&](auto t) { launch_ngd_t<decltype(t)>(c, params, grad, hess, eta, logpi, entropy, elbo); });
}

}  // namespace mivi
