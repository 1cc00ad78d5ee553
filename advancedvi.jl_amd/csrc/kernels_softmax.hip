// The softmax (multinomial logistic) regression target (include/mivi.h, mivi_set_target_softmax): theta = [vec B (p x C); s] per sample
// column of Z, evaluated for a chunk of samples by three launches.  api_softmax.hip sets the target; eval_generic_target reaches
// launch_sm_target below.
//
// Both data products run on the 16 x 16 x 4 matrix-core forms of the element type (Mfma16, device_common.h): products exact in T, no
// split planes.  The COLUMNS of both products are (sample, class) pairs: a sample's C logits are padded to CT = ceil(C / 16) whole
// 16-column tiles, and a workgroup's 64 columns hold SG = 4 / CT whole samples (C <= 16: four samples, C <= 32: two, else one).  Padded
// columns are fed zeros and are never read back: the softmax walks c < C only.
//   k_sm_logits  a workgroup owns 64 rows x one column group; wave w owns rows 16 w .. 16 w + 15 and all four column tiles.  X (through
//                the row index vector, if a selection is set) and B are staged through LDS over p in chunks of 16.  Epilogue: the tile of
//                Lambda goes to LDS, thread (row, sample) takes the row maximum, exp in T, the sum, lse and Lambda[r, y_r] - lse_r in f64,
//                and overwrites its logits with Y - P; wave ms sums sample ms's terms over the tile's rows (one f64 per (row tile, sample));
//                the residuals leave as R[r][sample][class], class fastest -- the B operand of the second product as it is staged.
//   k_sm_xtr     X'R: a workgroup owns 64 features x one column group x one slice of the rows, rows staged 16 at a time.  f32 accumulators
//                are flushed into f64 every 512 rows; the slice's f64 partial goes to its own plane.
//   k_sm_finish  one workgroup per sample: the slices in slice order, likeadj, the prior's -B / sigma^2, |B|^2, the s entry, ell -- all f64,
//                rounded once into ell (M) and G (d x M) where eval_generic_target leaves them for the other generic targets.
// Nothing is accumulated atomically and no geometry depends on the chunking of the samples: results are bitwise reproducible and the
// same for every plane cap.
#include "device_common.h"

namespace mivi {

constexpr int kSmKC = 16;        // the K axis staged per step (features in k_sm_logits, rows in k_sm_xtr)
constexpr int kSmFlush = 512;    // k_sm_xtr: rows between two flushes of the f32 accumulators into f64

template <typename T>
struct SmArgs {
  int d, p, C, CT, SG;
  int M, m0;                  // samples of this chunk; the chunk's first sample column in Z / ell / G
  long long n, nr;            // rows of the data set (X's leading dimension); rows evaluated
  const T *X;
  const uint8_t *y;
  const long long *rows;      // the row selection (nr entries) or nullptr: rows 0 .. nr - 1
  const T *Z;                 // d x M_total, ld d
  T *R;                       // nr x ldR: R[r ldR + ml C + c], ml the chunk-local sample
  long long ldR;
  double *ellp;               // [n_rt][M]
  double *gpart;              // [n_sl][M][p C]
  int n_sl;
  long long rps;              // rows per slice, a multiple of 16
  T *G, *ell;                 // d x M_total; M_total
  int variant, want_grad;
  double likeadj;
};

// column j of a workgroup's 64 -> (group-local sample, class); false: a padded column
__device__ __forceinline__ bool sm_col(int j, int CT, int SG, int C, int &ms, int &c) {
  const int t = j >> 4;
  ms = t / CT;
  c = (t - ms * CT) * 16 + (j & 15);
  return ms < SG && c < C;
}

template <typename T>
__global__ __launch_bounds__(256) void k_sm_logits(SmArgs<T> a) {
  using acc_t = typename Mfma16<T>::acc_t;
  constexpr int LDX = kSmKC + 1, LDB = 65;
  __shared__ T Xs[64 * LDX];
  __shared__ T Bs[kSmKC * LDB];
  __shared__ T Ls[64 * LDB];
  __shared__ long long rowi[64];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, kq = lane >> 4;
  const long long r0 = (long long)blockIdx.x * 64;
  const int g0 = blockIdx.y * a.SG, nt = a.SG * a.CT;
  if (tid < 64) {
    const long long r = r0 + tid;
    rowi[tid] = r < a.nr ? (a.rows ? a.rows[r] : r) : -1;
  }
  __syncthreads();
  acc_t acc[4];
#pragma unroll
  for (int t = 0; t < 4; ++t) acc[t] = acc_t{0, 0, 0, 0};
  for (int k0 = 0; k0 < a.p; k0 += kSmKC) {
    for (int e = tid; e < 64 * kSmKC; e += 256) {
      const int r = e & 63, k = e >> 6;
      const long long ri = rowi[r];
      Xs[r * LDX + k] = (ri >= 0 && k0 + k < a.p) ? a.X[ri + (long long)(k0 + k) * a.n] : T(0);
    }
    for (int e = tid; e < kSmKC * 64; e += 256) {
      const int k = e & (kSmKC - 1), j = e / kSmKC;
      int ms, c;
      T v = T(0);
      if (sm_col(j, a.CT, a.SG, a.C, ms, c) && g0 + ms < a.M && k0 + k < a.p)
        v = a.Z[(size_t)(a.m0 + g0 + ms) * a.d + (size_t)a.p * c + (k0 + k)];
      Bs[k * LDB + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kSmKC; kk += 4) {
      const T av = Xs[(16 * w + col) * LDX + kk + kq];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt) acc[t] = Mfma16<T>::mma(av, Bs[(kk + kq) * LDB + t * 16 + col], acc[t]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) Ls[(16 * w + Mfma16<T>::row(kq, r)) * LDB + t * 16 + col] = acc[t][r];
  __syncthreads();
  // ---- the softmax of (row, sample w): wave w is sample g0 + w of the group, its lanes the tile's 64 rows ----
  const int ms = w;
  const bool live = ms < a.SG && g0 + ms < a.M;
  double term = 0.0;
  if (live && rowi[lane] >= 0) {
    T *L = Ls + lane * LDB + ms * a.CT * 16;
    const int yr = a.y[rowi[lane]];
    T mx = L[0];
    for (int c = 1; c < a.C; ++c) mx = L[c] > mx ? L[c] : mx;
    const T ly = yr < a.C ? L[yr] : T(NAN);   // (a label outside the classes, possible with device data only: the value is NaN, not a wild read)
    double se = 0.0;
    for (int c = 0; c < a.C; ++c) {
      T e;
      if constexpr (sizeof(T) == 4) e = expf(L[c] - mx);
      else e = exp(L[c] - mx);
      L[c] = e;
      se += (double)e;
    }
    term = ((double)ly - (double)mx) - log(se);
    const T inv = (T)(1.0 / se);
    for (int c = 0; c < a.C; ++c) L[c] = (c == yr ? T(1) : T(0)) - L[c] * inv;
  }
  term = wave_sum(term);
  if (live && lane == 0) a.ellp[(size_t)blockIdx.x * a.M + g0 + ms] = term;
  if (!a.want_grad) return;
  __syncthreads();
  const int ncol = a.SG * a.C;
  for (int e = tid; e < 64 * ncol; e += 256) {
    const int row = e / ncol, j = e - row * ncol, s = j / a.C, c = j - s * a.C;
    if (rowi[row] >= 0 && g0 + s < a.M) a.R[(r0 + row) * a.ldR + (long long)g0 * a.C + j] = Ls[row * LDB + s * a.CT * 16 + c];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_sm_xtr(SmArgs<T> a) {
  using acc_t = typename Mfma16<T>::acc_t;
  constexpr int LDX = kSmKC + 1, LDB = 65;
  __shared__ T Xs[64 * LDX];      // [feature][row]
  __shared__ T Rs[kSmKC * LDB];   // [row][column]
  __shared__ long long rowi[kSmKC];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, kq = lane >> 4;
  const int f0 = blockIdx.x * 64, g0 = blockIdx.y * a.SG, sl = blockIdx.z, nt = a.SG * a.CT;
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  acc_t acc[4];
  double sum[4][4];
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    acc[t] = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[t][r] = 0.0;
  }
  int since = 0;
  for (long long rr = rbeg; rr < rend; rr += kSmKC) {
    if (tid < kSmKC) rowi[tid] = rr + tid < rend ? (a.rows ? a.rows[rr + tid] : rr + tid) : -1;
    __syncthreads();
    for (int e = tid; e < 64 * kSmKC; e += 256) {
      const int r = e & (kSmKC - 1), f = e / kSmKC;
      const long long ri = rowi[r];
      Xs[f * LDX + r] = (ri >= 0 && f0 + f < a.p) ? a.X[ri + (long long)(f0 + f) * a.n] : T(0);
    }
    for (int e = tid; e < kSmKC * 64; e += 256) {
      const int j = e & 63, r = e >> 6;
      int ms, c;
      T v = T(0);
      if (sm_col(j, a.CT, a.SG, a.C, ms, c) && g0 + ms < a.M && rowi[r] >= 0) v = a.R[(rr + r) * a.ldR + (long long)(g0 + ms) * a.C + c];
      Rs[r * LDB + j] = v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < kSmKC; kk += 4) {
      const T av = Xs[(16 * w + col) * LDX + kk + kq];
#pragma unroll
      for (int t = 0; t < 4; ++t)
        if (t < nt) acc[t] = Mfma16<T>::mma(av, Rs[(kk + kq) * LDB + t * 16 + col], acc[t]);
    }
    __syncthreads();
    if constexpr (sizeof(T) == 4) {
      since += kSmKC;
      if (since >= kSmFlush) {
        since = 0;
#pragma unroll
        for (int t = 0; t < 4; ++t)
#pragma unroll
          for (int r = 0; r < 4; ++r) { sum[t][r] += (double)acc[t][r]; acc[t][r] = T(0); }
      }
    }
  }
  const size_t pC = (size_t)a.p * a.C;
#pragma unroll
  for (int t = 0; t < 4; ++t)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int f = f0 + 16 * w + Mfma16<T>::row(kq, r);
      int ms, c;
      if (sm_col(t * 16 + col, a.CT, a.SG, a.C, ms, c) && g0 + ms < a.M && f < a.p)
        a.gpart[((size_t)sl * a.M + g0 + ms) * pC + (size_t)a.p * c + f] = sum[t][r] + (double)acc[t][r];
    }
}

template <typename T>
__global__ __launch_bounds__(256) void k_sm_finish(SmArgs<T> a, int n_rt) {
  __shared__ double red[8];
  const int tid = threadIdx.x, ml = blockIdx.x;
  const size_t pC = (size_t)a.p * a.C;
  const T *z = a.Z + (size_t)(a.m0 + ml) * a.d;
  const double s = (double)z[a.d - 1], is2 = exp(-2.0 * s);
  double v[2] = {0.0, 0.0};   // |B|^2, the log-likelihood
  for (size_t i = tid; i < pC; i += 256) v[0] += (double)z[i] * (double)z[i];
  for (int rt = tid; rt < n_rt; rt += 256) v[1] += a.ellp[(size_t)rt * a.M + ml];
  block_sum_n<double, 256, 2>(v, red);
  if (a.want_grad) {
    T *g = a.G + (size_t)(a.m0 + ml) * a.d;
    for (size_t i = tid; i < pC; i += 256) {
      double x = 0.0;
      for (int sl = 0; sl < a.n_sl; ++sl) x += a.gpart[((size_t)sl * a.M + ml) * pC + i];
      g[i] = (T)(a.likeadj * x - (double)z[i] * is2);
    }
  }
  if (tid == 0) {
    const double bb = v[0], npc = (double)pC;
    double lp = -0.5 * npc * kLog2Pi - npc * s - 0.5 * bb * is2, gs = -npc + bb * is2;
    if (a.variant == 0) {   // s = log sigma, Normal(0, 3) prior on sigma
      const double s2 = exp(2.0 * s);
      lp += -0.5 * log(2.0 * M_PI * 9.0) - s2 / 18.0;
      gs += -s2 / 9.0;
    } else {                // LogNormal(0, 3) prior on sigma, + log |det J| = s
      lp += -s - log(3.0) - 0.5 * kLog2Pi - s * s / 18.0 + s;
      gs += -1.0 - s / 9.0 + 1.0;
    }
    a.ell[a.m0 + ml] = (T)(a.likeadj * v[1] + lp);
    if (a.want_grad) a.G[(size_t)(a.m0 + ml) * a.d + a.d - 1] = (T)gs;
  }
}

// ---- the launches' geometry: a function of the rows, p, C and the caps alone ----------------------------------------------------------
struct SmGeom {
  int p, C, CT, SG, n_rt, n_sl, Mc;
  long long rps;
};
static SmGeom sm_geom(const mivi_ctx *c, int M) {
  SmGeom g;
  g.C = c->sm_C;
  g.p = (c->cfg.d - 1) / g.C;
  g.CT = (g.C + 15) / 16;
  g.SG = 4 / g.CT;
  const long long nr = c->sm_rows.nr;
  g.n_rt = (int)((nr + 63) / 64);
  long long ns = (nr + 127) / 128;
  ns = ns < 1 ? 1 : (ns > 32 ? 32 : ns);
  g.rps = ((nr + ns - 1) / ns + kSmKC - 1) / kSmKC * kSmKC;
  g.n_sl = (int)((nr + g.rps - 1) / g.rps);
  const size_t cap = c->sm_rows.cap ? c->sm_rows.cap : kSmPlaneCap;
  const size_t by_R = cap / ((size_t)nr * g.C * c->esize), by_P = kSmPartCap / ((size_t)g.n_sl * g.p * g.C * sizeof(double));
  size_t mc = by_R < by_P ? by_R : by_P;
  if (mc > (size_t)M) mc = (size_t)M;
  if (mc > (size_t)g.SG) mc -= mc % g.SG;   // (whole column groups, where a chunk holds more than one)
  g.Mc = mc < 1 ? 1 : (int)mc;
  return g;
}
int sm_chunk_samples(const mivi_ctx *c, int M) { return sm_geom(c, M).Mc; }

bool sm_reserve(mivi_ctx *c, int M) {
  const SmGeom g = sm_geom(c, M);
  const size_t pC = (size_t)g.p * g.C;
  return !ensure(c, c->sm_R, (size_t)c->sm_rows.nr * g.Mc * g.C * c->esize, false) &&
         !ensure(c, c->sm_part, (size_t)g.n_sl * g.Mc * pC * sizeof(double), false) &&
         !ensure(c, c->sm_ell, (size_t)g.n_rt * g.Mc * sizeof(double), false);
}

template <typename T>
static bool sm_impl(mivi_ctx *c, int M, int want_grad) {
  const SmGeom g = sm_geom(c, M);
  SmArgs<T> a;
  a.d = c->cfg.d;
  a.p = g.p;
  a.C = g.C;
  a.CT = g.CT;
  a.SG = g.SG;
  a.n = c->sm_rows.n;
  a.nr = c->sm_rows.nr;
  a.X = (const T *)c->sm_X;
  a.y = c->sm_y;
  a.rows = c->sm_rows.sel ? (const long long *)c->sm_rows.idx.p : nullptr;
  a.Z = (const T *)c->Z.p;
  a.R = (T *)c->sm_R.p;
  a.ldR = (long long)g.Mc * g.C;
  a.ellp = (double *)c->sm_ell.p;
  a.gpart = (double *)c->sm_part.p;
  a.n_sl = g.n_sl;
  a.rps = g.rps;
  a.G = (T *)c->W.p;
  a.ell = (T *)c->ell.p;
  a.variant = c->sm_variant;
  a.want_grad = want_grad;
  a.likeadj = c->sm_rows.likeadj;
  for (int m0 = 0; m0 < M; m0 += g.Mc) {   // chunks of samples: the residual plane and the partials stay under their caps
    a.m0 = m0;
    a.M = M - m0 < g.Mc ? M - m0 : g.Mc;
    const int groups = (a.M + g.SG - 1) / g.SG;
    hipLaunchKernelGGL(k_sm_logits<T>, dim3(g.n_rt, groups), dim3(256), 0, c->stream, a);
    if (want_grad) hipLaunchKernelGGL(k_sm_xtr<T>, dim3((g.p + 63) / 64, groups, g.n_sl), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_sm_finish<T>, dim3(a.M), dim3(256), 0, c->stream, a, g.n_rt);
  }
  return true;
}

// false: device allocation of the residual plane / the partials failed
bool launch_sm_target(mivi_ctx *c, int M, int want_grad) {
  if (!sm_reserve(c, M)) return false;
  return by_dtype(c, [&](auto t) { return sm_impl<decltype(t)>(c, M, want_grad); });
}

}  // namespace mivi
