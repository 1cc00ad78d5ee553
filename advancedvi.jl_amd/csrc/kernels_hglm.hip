// The hierarchical GLM target (include/mivi.h, mivi_set_target_hglm): theta = [beta (p); u (J); s] per sample column of Z,
// eta_r = x_r . beta + u[g_r] + o_r.  api_hglm.hip sets the target and builds, on the host, the order the rows are walked in (by group id),
// the segment table gstart (J + 1) and the first and last group of every row slice; eval_generic_target reaches launch_hglm_target.
//
//   k_hglm_rows      grid (row slice, group of 16 x waves samples), 64 x waves threads (4 waves; 2 where the LDS would not hold 4).  ONE pass
//                    over X does the logits, the likelihood and both reductions.  Wave w owns samples 16 w .. 16 w + 15 of the group and
//                    stages their beta into LDS once, as a [P][17] block (P: p padded to 16 by zero rows).  The slice is walked in tiles of
//                    16 rows (through the row index vector, if one is set).  A tile of X is staged ONCE, as [P][17], and serves all waves
//                    and both products on the 16 x 16 x 4 matrix-core form of the element type (Mfma16):
//                      eta   = X_tile (A) . beta (B), K = p;
//                      dbeta += X_tile' (A: the same block read the other way) . res (B), K = the tile's 16 rows,
//                    with the ceil(p / 16) accumulator tiles of a wave in registers across the slice (NT of them: the kernel is
//                    instantiated for NT = 1, 2, 4, 8, 16); f32 accumulators are flushed into the slice's f64 partial every kHglmFlush
//                    rows.  Between the products every lane adds u[g_r] and the offset to its four (row, sample) logits and takes the
//                    log-likelihood term and the residual in f64; a row past the slice's end has res = 0.  du is a segmented sum with
//                    carry: one lane per sample column walks the tile's 16 f64 residuals in row order and, when the group id changes,
//                    stores the finished sum -- into the [J][samples] group plane if the group lies inside the slice, into the slice's
//                    edge partial if it is the slice's first or last group (it may go on in a neighbouring slice; a group that covers
//                    a whole slice is both: one edge partial).
//   k_hglm_finish_u  64 groups x 64 samples per workgroup: every group's row sum -- 0 if gstart says it has no rows, the group-plane entry
//                    if it is interior to a slice, its slices' edge partials added in slice order otherwise -- then likeadj and the prior,
//                    transposed through LDS into the u block of G.  The group plane is never cleared: entries no slice wrote are not read.
//   k_hglm_finish    one workgroup per sample: the beta partials and the log-likelihood in slice order, |beta|^2 and |u|^2, the three
//                    priors, the lgamma constant, d/ds -- all f64, rounded once into ell (M) and G (d x M).
// Every store is an ordinary one, nothing is accumulated atomically and no geometry depends on the chunking of the samples: results are
// bitwise reproducible and the same for every partial cap.
#include "flow_tile.h"

namespace mivi {

constexpr int kHglmLd = kFlowTile + 1;   // stride of a [feature][16] block (X tile, a wave's beta)
constexpr int kHglmFlush = 128;          // rows between two flushes of the f32 dbeta accumulators into the f64 partial
constexpr size_t kHglmLdsMax = 128 * 1024;   // four waves' blocks above it: the workgroup runs two waves

template <typename T>
struct HglmArgs {
  int p, P, J, d;            // P: p padded to a multiple of 16
  int M, m0;                 // samples of this chunk; the chunk's first sample column in Z / ell / G
  long long n, nr;           // X's leading dimension; rows evaluated
  const T *X, *y, *off;      // off: nullptr without an offset
  const long long *rows;     // the row order (nr entries) or nullptr: rows 0 .. nr - 1
  const int *grp;            // the group of every evaluated row (nr)
  const long long *gstart;   // J + 1
  const int *sltab;          // [n_sl][2]: first and last group of a slice
  const T *Z;                // d x M_total, ld d
  double *bpart;             // [n_sl][M][p]
  double *gplane;            // [J][M]
  double *edge;              // [n_sl][2][M]
  double *llp;               // [n_sl][M]
  int n_sl;
  long long rps;             // rows per slice, a multiple of 16
  T *G, *ell;                // d x M_total; M_total
  int likelihood, want_grad;
  double prior_std, tau_scale, likeadj, lgam;
};

// the wave's dbeta tiles -> the slice's f64 partial (added to it after the first flush); the accumulators restart at zero
template <typename T, int NT>
__device__ __forceinline__ void hglm_flush(const HglmArgs<T> &a, typename Mfma16<T>::acc_t (&acc)[NT], double *part, int ml, bool add) {
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = 16 * t + Mfma16<T>::row(kq, r);
      if (k < a.p && ml + col < a.M) {
        double *dst = part + (size_t)(ml + col) * a.p + k;
        *dst = add ? *dst + (double)acc[t][r] : (double)acc[t][r];
      }
      acc[t][r] = T(0);
    }
  }
}

template <typename T, int NT>
__global__ __launch_bounds__(256) void k_hglm_rows(HglmArgs<T> a) {
  using acc_t = typename Mfma16<T>::acc_t;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, kq = lane >> 4, nthr = blockDim.x, spw = nthr >> 2;   // spw: samples per workgroup
  const int ldr = spw + 1;
  double *Rd = flow_lds;                                                                                    // [16][spw + 1]: the tile's f64 residuals
  T *R = sizeof(T) == 8 ? reinterpret_cast<T *>(Rd) : reinterpret_cast<T *>(Rd + kFlowTile * ldr);          // the same rounded to T (f64: the same block)
  T *Xt = reinterpret_cast<T *>(Rd + kFlowTile * ldr) + (sizeof(T) == 8 ? 0 : kFlowTile * ldr);             // [P][17]
  T *Bw = Xt + (1 + w) * a.P * kHglmLd;                                                                     // this wave's beta, [P][17]
  __shared__ int gt[kFlowTile];
  __shared__ double yo[2 * kFlowTile];
  const int sl = blockIdx.x, ml0 = blockIdx.y * spw, ml = ml0 + 16 * w;   // ml: the wave's first sample of the chunk
  const bool mine = ml + col < a.M;                                        // this lane's sample column exists
  const T *z = a.Z + (size_t)(a.m0 + (mine ? ml + col : 0)) * a.d;
  for (int e = lane; e < a.P * kFlowTile; e += 64) {   // the wave's beta: [k][sample], zero rows past p and zero columns past M
    const int c = e & 15, k = e >> 4;
    Bw[k * kHglmLd + c] = (k < a.p && ml + c < a.M) ? a.Z[(size_t)(a.m0 + ml + c) * a.d + k] : T(0);
  }
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  const int gfirst = a.sltab[2 * sl], glast = a.sltab[2 * sl + 1];
  acc_t acc[NT];
#pragma unroll
  for (int t = 0; t < NT; ++t) acc[t] = acc_t{0, 0, 0, 0};
  double ll = 0.0, gsum = 0.0;
  int gcur = gfirst, since = 0;
  bool flushed = false;
  double *bpart = a.bpart + (size_t)sl * a.M * a.p;
  // a finished group sum of this lane's sample column -> the group plane, or the slice's edge partial
  auto put_group = [&](int g, double v) {
    if (g == gfirst) a.edge[((size_t)sl * 2) * a.M + ml + col] = v;
    else if (g == glast) a.edge[((size_t)sl * 2 + 1) * a.M + ml + col] = v;
    else a.gplane[(size_t)g * a.M + ml + col] = v;
  };
  for (long long rr = rbeg; rr < rend; rr += kFlowTile) {
    __syncthreads();   // the previous tile's products and walk are done with Xt, R and gt
    {
      const long long i = rr + (tid & 15);
      const long long ri = i < rend ? (a.rows ? a.rows[i] : i) : -1;   // (every thread stages the same tile row in each of its turns)
      if (tid < kFlowTile) {
        gt[tid] = ri >= 0 ? a.grp[i] : -1;
        yo[tid] = ri >= 0 ? (double)a.y[ri] : 0.0;
        yo[kFlowTile + tid] = (ri >= 0 && a.off) ? (double)a.off[ri] : 0.0;
      }
      for (int k = tid >> 4; k < a.P; k += nthr >> 4) Xt[k * kHglmLd + (tid & 15)] = (ri >= 0 && k < a.p) ? a.X[ri + (long long)k * a.n] : T(0);
    }
    __syncthreads();
    T ug[4];   // u[g_r] of this lane's four (row, sample) entries: gathered from Z ahead of the product, whose K loop covers the latency
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int g = gt[Mfma16<T>::row(kq, r)];
      ug[r] = (g >= 0 && mine) ? z[a.p + g] : T(0);
    }
    acc_t eta = acc_t{0, 0, 0, 0};
    for (int kk = 0; kk < ((a.p + 3) & ~3); kk += 4) eta = Mfma16<T>::mma(Xt[(kk + kq) * kHglmLd + col], Bw[(kk + kq) * kHglmLd + col], eta);
#pragma unroll
    for (int r = 0; r < 4; ++r) {   // (row, sample col): u[g_r], the offset, the likelihood and the residual in f64
      const int row = Mfma16<T>::row(kq, r), g = gt[row];
      double rs = 0.0;
      if (g >= 0 && mine) {
        const double y = yo[row], h = (double)eta[r] + (double)ug[r] + yo[kFlowTile + row];
        if (a.likelihood == 0) {
          const double e = exp(-fabs(h));
          ll += y * h - (fmax(h, 0.0) + log1p(e));
          rs = y - (h >= 0.0 ? 1.0 : e) / (1.0 + e);
        } else {
          const double e = exp(h);
          ll += y * h - e;
          rs = y - e;
        }
      }
      Rd[row * ldr + 16 * w + col] = rs;
      if constexpr (sizeof(T) == 4) R[row * ldr + 16 * w + col] = (T)rs;
    }
    if (a.want_grad) {
      __syncthreads();   // (R is read by its own wave only, but across lanes)
#pragma unroll
      for (int t = 0; t < NT; ++t)
        if (16 * t < a.P) {
#pragma unroll
          for (int kk = 0; kk < kFlowTile; kk += 4)
            acc[t] = Mfma16<T>::mma(Xt[(16 * t + col) * kHglmLd + kk + kq], R[(kk + kq) * ldr + 16 * w + col], acc[t]);
        }
      if (kq == 0 && mine) {   // the segmented sum with carry: the tile's residuals of this sample column in row order
        for (int r = 0; r < kFlowTile; ++r) {
          const int g = gt[r];
          if (g < 0) break;
          if (g != gcur) {
            put_group(gcur, gsum);
            gcur = g;
            gsum = 0.0;
          }
          gsum += Rd[r * ldr + 16 * w + col];
        }
      }
      if constexpr (sizeof(T) == 4) {
        since += kFlowTile;
        if (since >= kHglmFlush) {
          hglm_flush<T, NT>(a, acc, bpart, ml, flushed);
          flushed = true;
          since = 0;
        }
      }
    }
  }
  ll += __shfl_xor(ll, 16, 64);   // the four row quarters of a sample column
  ll += __shfl_xor(ll, 32, 64);
  if (kq == 0 && mine) a.llp[(size_t)sl * a.M + ml + col] = ll;
  if (!a.want_grad) return;
  hglm_flush<T, NT>(a, acc, bpart, ml, flushed);
  if (kq == 0 && mine) put_group(gcur, gsum);
}

template <typename T>
__global__ __launch_bounds__(256) void k_hglm_finish_u(HglmArgs<T> a) {
  __shared__ double tile[64][65];
  const int tid = threadIdx.x, g0 = blockIdx.x * 64, ml0 = blockIdx.y * 64;
  for (int e = tid; e < 64 * 64; e += 256) {
    const int gi = e >> 6, mi = e & 63, g = g0 + gi, ml = ml0 + mi;
    double x = 0.0;
    if (g < a.J && ml < a.M) {
      const long long r0 = a.gstart[g], r1 = a.gstart[g + 1];
      if (r1 > r0) {
        const int s0 = (int)(r0 / a.rps), s1 = (int)((r1 - 1) / a.rps);
        if (s0 == s1 && a.sltab[2 * s0] != g && a.sltab[2 * s0 + 1] != g) x = a.gplane[(size_t)g * a.M + ml];
        else
          for (int s = s0; s <= s1; ++s) x += a.edge[((size_t)s * 2 + (a.sltab[2 * s] == g ? 0 : 1)) * a.M + ml];
      }
    }
    tile[gi][mi] = x;
  }
  __syncthreads();
  for (int e = tid; e < 64 * 64; e += 256) {
    const int mi = e >> 6, gi = e & 63, g = g0 + gi, ml = ml0 + mi;
    if (g < a.J && ml < a.M) {
      const size_t zc = (size_t)(a.m0 + ml) * a.d;
      const double s = (double)a.Z[zc + a.d - 1];
      a.G[zc + a.p + g] = (T)(a.likeadj * tile[gi][mi] - (double)a.Z[zc + a.p + g] * exp(-2.0 * s));
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_hglm_finish(HglmArgs<T> a) {
  __shared__ double red[12];
  const int tid = threadIdx.x, ml = blockIdx.x;
  const size_t zc = (size_t)(a.m0 + ml) * a.d;
  const T *z = a.Z + zc;
  const double ip2 = 1.0 / (a.prior_std * a.prior_std), s = (double)z[a.d - 1];
  double v[3] = {0.0, 0.0, 0.0};   // |beta|^2, |u|^2, sum of the slices' log-likelihoods
  for (int k = tid; k < a.p; k += 256) {
    const double b = (double)z[k];
    v[0] += b * b;
    if (a.want_grad) {
      double x = 0.0;
      for (int sl = 0; sl < a.n_sl; ++sl) x += a.bpart[((size_t)sl * a.M + ml) * a.p + k];
      a.G[zc + k] = (T)(a.likeadj * x - b * ip2);
    }
  }
  for (int g = tid; g < a.J; g += 256) {
    const double u = (double)z[a.p + g];
    v[1] += u * u;
  }
  for (int sl = tid; sl < a.n_sl; sl += 256) v[2] += a.llp[(size_t)sl * a.M + ml];
  block_sum_n<double, 256, 3>(v, red);
  if (tid == 0) {
    const double e2 = exp(2.0 * s), em2 = exp(-2.0 * s), it2 = 1.0 / (a.tau_scale * a.tau_scale);
    const double lp = -0.5 * v[0] * ip2 - (double)a.p * (log(a.prior_std) + 0.5 * kLog2Pi)      // beta
                      - 0.5 * v[1] * em2 - (double)a.J * (s + 0.5 * kLog2Pi)                    // u | s
                      + log(2.0) - 0.5 * kLog2Pi - log(a.tau_scale) - 0.5 * e2 * it2 + s;       // tau, with the Jacobian of s = log tau
    a.ell[a.m0 + ml] = (T)(a.likeadj * (v[2] - a.lgam) + lp);
    if (a.want_grad) a.G[zc + a.d - 1] = (T)(-(double)a.J + v[1] * em2 - e2 * it2 + 1.0);
  }
}

// ---- the launches' geometry: a function of the evaluated rows, p, the precision and the cap alone --------------------------------------
static int hglm_chunk(const mivi_ctx *c, const RowSlices &g, int M) {   // samples per chunk under the cap
  return samples_under_cap(c->hg_rows.cap ? c->hg_rows.cap : kHglmPartCap, ((size_t)g.n_sl * (c->hg_p + 3) + (size_t)c->hg.n_groups) * sizeof(double), M);
}

bool hglm_reserve(mivi_ctx *c, int M) {
  const RowSlices g = row_slices(c->hg_rows.nr, kHglmSliceRows, kHglmMaxSlices);
  const size_t mc = (size_t)hglm_chunk(c, g, M), D = sizeof(double);
  return !ensure(c, c->hg_bpart, (size_t)g.n_sl * mc * c->hg_p * D, false) && !ensure(c, c->hg_gplane, (size_t)c->hg.n_groups * mc * D, false) &&
         !ensure(c, c->hg_edge, (size_t)g.n_sl * 2 * mc * D, false) && !ensure(c, c->hg_ll, (size_t)g.n_sl * mc * D, false);
}

// LDS bytes of k_hglm_rows with `waves` waves: the X tile and the waves' beta blocks (T), the f64 residual block and, in f32, its rounded copy
template <typename T>
static size_t hglm_lds(int P, int waves) {
  return (size_t)(1 + waves) * P * kHglmLd * sizeof(T) + (size_t)kFlowTile * (16 * waves + 1) * (sizeof(double) + (sizeof(T) == 4 ? sizeof(T) : 0));
}

template <typename T, int NT>
static bool hglm_rows_launch(mivi_ctx *c, const HglmArgs<T> &a, int n_sl) {
  const int waves = hglm_lds<T>(a.P, 4) <= kHglmLdsMax ? 4 : 2;
  const size_t lds = hglm_lds<T>(a.P, waves);
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(k_hglm_rows<T, NT>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return false;
  hipLaunchKernelGGL((k_hglm_rows<T, NT>), dim3(n_sl, (a.M + 16 * waves - 1) / (16 * waves)), dim3(64 * waves), lds, c->stream, a);
  return true;
}

template <typename T>
static bool hglm_impl(mivi_ctx *c, int M, int want_grad) {
  const RowSlices g = row_slices(c->hg_rows.nr, kHglmSliceRows, kHglmMaxSlices);
  const int Mc = hglm_chunk(c, g, M);
  HglmArgs<T> a{};
  a.p = c->hg_p;
  a.P = (a.p + 15) & ~15;
  a.J = c->hg.n_groups;
  a.d = c->cfg.d;
  a.n = c->hg_rows.n;
  a.nr = c->hg_rows.nr;
  a.X = (const T *)c->hg_X;
  a.y = (const T *)c->hg_y;
  a.off = (const T *)c->hg_off;
  a.rows = c->hg_rows.sel ? (const long long *)c->hg_rows.idx.p : nullptr;
  a.grp = (const int *)c->hg_grp.p;
  a.gstart = (const long long *)c->hg_gstart.p;
  a.sltab = (const int *)c->hg_sltab.p;
  a.Z = (const T *)c->Z.p;
  a.bpart = (double *)c->hg_bpart.p;
  a.gplane = (double *)c->hg_gplane.p;
  a.edge = (double *)c->hg_edge.p;
  a.llp = (double *)c->hg_ll.p;
  a.n_sl = g.n_sl;
  a.rps = g.rps;
  a.G = (T *)c->W.p;
  a.ell = (T *)c->ell.p;
  a.likelihood = c->hg.likelihood;
  a.want_grad = want_grad;
  a.prior_std = c->hg.prior_std;
  a.tau_scale = c->hg.tau_scale;
  a.likeadj = c->hg_rows.likeadj;
  a.lgam = c->hg_lgam;
  const int nt = a.P / 16;
  for (int m0 = 0; m0 < M; m0 += Mc) {   // chunks of samples: the f64 partials stay under their cap
    a.m0 = m0;
    a.M = M - m0 < Mc ? M - m0 : Mc;
    const bool ok = nt <= 1 ? hglm_rows_launch<T, 1>(c, a, g.n_sl) : nt <= 2 ? hglm_rows_launch<T, 2>(c, a, g.n_sl) : nt <= 4 ? hglm_rows_launch<T, 4>(c, a, g.n_sl)
                  : nt <= 8 ? hglm_rows_launch<T, 8>(c, a, g.n_sl) : hglm_rows_launch<T, 16>(c, a, g.n_sl);
    if (!ok) return false;
    if (want_grad) hipLaunchKernelGGL(k_hglm_finish_u<T>, dim3((a.J + 63) / 64, (a.M + 63) / 64), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_hglm_finish<T>, dim3(a.M), dim3(256), 0, c->stream, a);
  }
  return true;
}

// false: device allocation of the partials failed, or the runtime refused the kernel its LDS
bool launch_hglm_target(mivi_ctx *c, int M, int want_grad) {
  if (!hglm_reserve(c, M)) return false;
  return by_dtype(c, [&](auto t) { return hglm_impl<decltype(t)>(c, M, want_grad); });
}

}  // namespace mivi
