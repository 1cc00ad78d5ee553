// The logistic-regression target on ONE batch of a resident schedule of minibatches (mivi_logreg_set_batch_schedule), fused: the rows of
// the batch are read straight out of the resident data set through the schedule -- no gathered copy of X, no residual matrix in memory.
//
// The minibatch regime of docs/src/tutorials/subsampling.md (a few hundred to a few thousand rows, 1 .. 16 samples per step) is almost no
// arithmetic: the resident-data kernels spend it as a gather, the logits, X^T r and the finish -- four to six launches that hand a batch-sized
// copy of X and the residuals R through memory.  Here a workgroup owns a SLAB of RS batch rows:
//   stage    Xs[r][k] = X[rows[r0 + r]][k]  (f32: the row-major copy logreg_prepare_f32 keeps; f64: the column-major matrix), y likewise;
//            rows past the batch and columns past p are written as zeros, every call
//   per chunk of MC sample columns:  Zs[m][k] = beta of column m0 + m (zeros past M and past p)
//     logit[r][m] = sum_k Xs[r][k] Zs[m][k]      (T products and sums in k order, the arithmetic of k_lr_logits)
//     ll[m] += y logit - softplus(logit) in f64, Rs[r][m] = y - sigmoid(logit)  -- in LDS only
//     g_part[slab][m][k] = sum_r Xs[r][k] Rs[r][m]  (T; at most 64 terms: the slabs are added in f64 by k_lr_finish)
// and leaves ll_part[slab][M], g_part[slab][M][p] in the layout k_lr_finish (kernels_targets.hip) reduces: an estimate's target is this
// kernel and the finisher.
//
// LDS: row r of Xs / Zs starts at r * ldp elements, ldp = p | 1 odd: the 32 lanes of a half wave that read one column of 32 rows (the logits)
// hit 32 banks (f32; f64: 32 even bank pairs), the lanes that read consecutive columns of one row (X^T r) are contiguous.  Sized from the
// device's limit (up to 160 KB per workgroup); lr_batch_fits says whether a minimal slab (8 rows x 4 sample columns) fits -- where it does
// not (p beyond ~3000 in f32), the batch takes the device gather and the resident-data kernels (logreg_batch_route).
#include "device_common.h"

namespace mivi {

namespace {
constexpr int kLrBatchNT = 256;

struct LrBatchGeom {
  bool ok;
  int RS, MC, ldp, S;
  size_t lds;
};

size_t lr_batch_lds(int RS, int MC, int ldp, size_t es) { return es * ((size_t)RS * ldp + (size_t)MC * ldp + (size_t)RS * (MC + 1) + (size_t)RS); }

LrBatchGeom lr_batch_geom(const mivi_ctx *c, int M) {
  LrBatchGeom g{};
  const long long b = c->lr_n;
  const int p = c->cfg.d - 1;
  const size_t budget = c->lds_max < 160 * 1024 ? c->lds_max : (size_t)160 * 1024;
  g.ldp = p | 1;
  int RS = b > 2048 ? 64 : 32;   // (more, smaller slabs for the small batches: they are all latency)
  while (RS > 1 && RS / 2 >= b) RS /= 2;
  int MC = M < 32 ? M : 32;
  const int RS_min = RS < 8 ? RS : 8, MC_min = MC < 4 ? MC : 4;
  while (lr_batch_lds(RS, MC, g.ldp, c->esize) > budget) {
    if (MC > 8) MC = (MC + 1) / 2;
    else if (RS > RS_min) RS /= 2;
    else if (MC > MC_min) MC = (MC + 1) / 2;
    else return g;   // not even a minimal slab
  }
  g.ok = b >= 1 && M >= 1;
  g.RS = RS;
  g.MC = MC;
  g.S = (int)((b + RS - 1) / RS);
  g.lds = lr_batch_lds(RS, MC, g.ldp, c->esize);
  return g;
}

template <typename T>
struct LrBatchArgs {
  int d, p, M, RS, MC, ldp, want_grad;
  long long b;             // rows of the batch
  long long sr, sk;        // element (row, k) of the data set: X[row * sr + k * sk]
  const T *X;
  const uint8_t *y;
  const int32_t *rows;     // the batch: rows[0 .. b) of the data set
  const T *Z;              // d x M
  double *ll_part;         // [S][M]
  T *g_part;               // [S][M][p]
};

template <typename T>
__device__ __forceinline__ T lr_batch_softplus(T x) { return x > T(0) ? x + log1p(exp(-x)) : log1p(exp(x)); }

template <typename T>
__global__ __launch_bounds__(kLrBatchNT) void k_lr_batch(LrBatchArgs<T> a) {
  extern __shared__ __align__(16) unsigned char lr_batch_lds_raw[];
  T *Xs = reinterpret_cast<T *>(lr_batch_lds_raw);   // [RS][ldp]
  T *Zs = Xs + (size_t)a.RS * a.ldp;                  // [MC][ldp]
  T *Rs = Zs + (size_t)a.MC * a.ldp;                  // [RS][MC + 1]
  T *ys = Rs + (size_t)a.RS * (a.MC + 1);             // [RS]
  const int tid = threadIdx.x, s = blockIdx.x;
  const int RS = a.RS, MC = a.MC, ldp = a.ldp, p = a.p;
  const long long r0 = (long long)s * RS;
  const int nr = (int)(a.b - r0 < RS ? a.b - r0 : RS);   // rows of this slab (>= 1)
  // the slab's rows, once: pad rows and pad columns are zeros
  for (int e = tid; e < RS * ldp; e += kLrBatchNT) {
    const int r = e / ldp, k = e - r * ldp;
    T v = T(0);
    if (r < nr && k < p) v = a.X[(long long)a.rows[r0 + r] * a.sr + (long long)k * a.sk];
    Xs[e] = v;
  }
  for (int r = tid; r < RS; r += kLrBatchNT) ys[r] = r < nr ? (T)a.y[a.rows[r0 + r]] : T(0);
  for (int m0 = 0; m0 < a.M; m0 += MC) {
    const int mc = a.M - m0 < MC ? a.M - m0 : MC;
    for (int e = tid; e < MC * ldp; e += kLrBatchNT) {
      const int m = e / ldp, k = e - m * ldp;
      Zs[e] = (m < mc && k < p) ? a.Z[(size_t)(m0 + m) * a.d + k] : T(0);
    }
    __syncthreads();
    // logits, residuals, log-likelihood partials: item (r, m), the RS rows of a column on adjacent lanes (uniform trip count: the shuffles
    // below need whole groups of RS lanes)
    for (int e0 = 0; e0 < RS * MC; e0 += kLrBatchNT) {
      const int e = e0 + tid;
      const int r = e & (RS - 1), m = e / RS;
      double ll = 0.0;
      if (m < MC) {
        const T *xr = Xs + (size_t)r * ldp, *zm = Zs + (size_t)m * ldp;
        T lg = T(0);
        for (int k = 0; k < p; ++k) lg += xr[k] * zm[k];
        T res = T(0);
        if (r < nr && m < mc) {
          const T yv = ys[r];
          ll = (double)(yv * lg - lr_batch_softplus(lg));
          res = yv - T(1) / (T(1) + exp(-lg));
        }
        Rs[(size_t)r * (MC + 1) + m] = res;
      }
      for (int o = RS >> 1; o > 0; o >>= 1) ll += __shfl_xor(ll, o, RS);
      if (r == 0 && m < mc) a.ll_part[(size_t)s * a.M + m0 + m] = ll;
    }
    __syncthreads();
    if (a.want_grad) {
      // X^T r of the slab from the same resident rows: item (k, m), consecutive k on adjacent lanes
      for (int e = tid; e < p * mc; e += kLrBatchNT) {
        const int m = e / p, k = e - m * p;
        T acc = T(0);
        for (int r = 0; r < RS; ++r) acc += Xs[(size_t)r * ldp + k] * Rs[(size_t)r * (MC + 1) + m];
        a.g_part[((size_t)s * a.M + m0 + m) * p + k] = acc;
      }
    }
    __syncthreads();   // (the next chunk rewrites Zs and Rs)
  }
}

template <typename T>
bool lr_batch_attr(size_t lds) {
  if (lds <= 64 * 1024) return true;   // (what a kernel may take without asking)
  if (hipFuncSetAttribute(reinterpret_cast<const void *>(&k_lr_batch<T>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return true;
}
}  // namespace

bool lr_batch_fits(const mivi_ctx *c, int M) { return lr_batch_geom(c, M).ok; }
int lr_batch_slabs(const mivi_ctx *c, int M) { return lr_batch_geom(c, M).S; }

bool lr_batch_prepare(mivi_ctx *c, int M) {
  const LrBatchGeom g = lr_batch_geom(c, M);
  if (!g.ok) return false;
  return by_dtype(c, [&](auto t) { return lr_batch_attr<decltype(t)>(g.lds); });
}

void launch_lr_batch(mivi_ctx *c, int M, int want_grad, const int32_t *rows, double *ll_part, void *g_part, int *n_slabs) {
  const LrBatchGeom g = lr_batch_geom(c, M);
  *n_slabs = g.S;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    (void)lr_batch_attr<T>(g.lds);
    LrBatchArgs<T> a;
    a.d = c->cfg.d; a.p = a.d - 1; a.M = M; a.RS = g.RS; a.MC = g.MC; a.ldp = g.ldp; a.want_grad = want_grad;
    a.b = c->lr_n;
    if (std::is_same<T, float>::value) {   // whole rows of the row-major copy (its leading dimension: p up to a multiple of 32)
      a.X = (const T *)c->lr_Xrm.p;
      a.sr = (a.p + 31) / 32 * 32;
      a.sk = 1;
    } else {
      a.X = (const T *)c->lr_X_full;
      a.sr = 1;
      a.sk = c->lr_n_full;
    }
    a.y = c->lr_y_full;
    a.rows = rows;
    a.Z = (const T *)c->Z.p;
    a.ll_part = ll_part;
    a.g_part = (T *)g_part;
    hipLaunchKernelGGL(k_lr_batch<T>, dim3(g.S), dim3(kLrBatchNT), g.lds, c->stream, a);
  });
}

}  // namespace mivi
