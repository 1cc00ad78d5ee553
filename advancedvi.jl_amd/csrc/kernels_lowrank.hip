// Low-rank Gaussian family (src/families/location_scale_low_rank.jl): z = D o u1 + U u2 + m with D (d) the scale diagonal, U (d x r)
// the scale factors and (u1; u2) one Philox stream of d + r rows per column.  Parameters [m (d); D (d); vec U (d x r, column-major)].
// The kernels of one RepGradELBO estimate (api_lowrank.hip drives them; DESIGN.md "Low-rank family" has the bytes and flops per stage):
//   k_lowr_gram       (r > 4 only) A = I + U' D^-2 U on many workgroups; up to r = 4 the prep workgroup forms it itself
//   k_lowr_draw_prep  workgroup 0: the parameter-only preparation in f64 -- A, its Cholesky factor, A^-1, sum log D, 1/2 logdet A;
//                   the other workgroups: the draws (u1; u2) -> E, (d + r) x M, written once and read by the sample, the Woodbury stages and the VJP
//   k_lowr_sample     Z = D o u1 + U u2 + m (K = r) and, for the Monte-Carlo / STL estimators, t = u1 + D^-1 U u2
//   k_lowr_s          s = U' D^-1 t (r x M, K = d, f64) and |t|^2 per column
//   k_lowr_xv         x = A^-1 s (f64), log q per column, V = Sigma^-1 (z - m) = D^-1 (t - D^-1 U x) in place over t
//   k_lowr_vjp        the three cotangent products (sum C, sum C o a1, C a2'; K = M) as f64 partials per slice of the sample axis
//   k_lowr_finish     the gradient entries from the slices' partials in a fixed order, with the entropy gradients dH/dU = D^-2 U A^-1 and
//                   dH/dD = 1/D - D^-3 diag(U A^-1 U') formed per entry; its last workgroup: the objective value, the status bit, the elbo record
// All products are plain fused multiply-adds (the f32-input MFMA runs at the vector rate on gfx950): the sample's K = r product in the
// element type, everything of size r (A, its factor, s, x) and every sum over d or M in f64 for either element type.  At the sizes measured
// (d = 1024, M = 256) no stage is bandwidth- or issue-bound: each is a 5-10 us launch, and the prep workgroup's serial factorisation is the
// longest link (DESIGN.md has the per-kernel table).  No floating-point atomics, one summation order: results are bitwise repeatable.
#include "device_common.h"

namespace mivi {

constexpr int kLowrScal = 16;   // doubles in front of the prep block: [0] sum log D, [1] 1/2 logdet A
// layout of the prep block (f64): [scalars (16) | A^-1 (r x r) | A (r x r, lower triangle: k_lowr_gram's)]
__host__ __device__ inline size_t lowr_off_ainv() { return kLowrScal; }
__host__ __device__ inline size_t lowr_off_a(int r) { return kLowrScal + (size_t)r * r; }
size_t lowr_prep_doubles(int d, int r) { (void)d; return kLowrScal + 2 * (size_t)r * r; }
#define LT(i, k) ((i) * ((i) + 1) / 2 + (k))

// N per-thread f64 values summed over a 256-thread workgroup through LDS, a fixed order (32 consecutive threads, then the 8 groups): a
// butterfly per value costs 12 cross-lane moves, and the K = d reductions below carry 16 to 20 values.  Results in out[0 .. N) (LDS), valid
// after the call's last barrier.  red: N x 256, out: N x 9 doubles (the results, then the 8 group sums of every value).
template <int N>
__device__ __forceinline__ void lowr_block_sums(const double (&v)[N], double *red, double *out) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int q = 0; q < N; ++q) red[q * 256 + tid] = v[q];
  __syncthreads();
  for (int t = tid; t < N * 8; t += 256) {
    const double *src = red + (t >> 3) * 256 + (t & 7) * 32;
    double a = 0.0;
    for (int l = 0; l < 32; ++l) a += src[l];
    out[N + t] = a;
  }
  __syncthreads();
  if (tid < N) {
    double a = 0.0;
    for (int g = 0; g < 8; ++g) a += out[N + tid * 8 + g];
    out[tid] = a;
  }
  __syncthreads();
}
constexpr int kLowrMaxSlices = 8;   // slices of the sample axis the VJP leaves partials for
int lowr_vjp_slices(int M) { const int s = (M + 31) / 32; return s < 1 ? 1 : (s > kLowrMaxSlices ? kLowrMaxSlices : s); }

// ---- A = I + U' D^-2 U for r > 4: one workgroup per 4 x 4 tile of the lower triangle, its threads over the K = d axis ---------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_lowr_gram(int d, int r, const T *__restrict__ params, double *__restrict__ prep) {
  __shared__ double red[16 * 256], out[16 * 9];
  const int a0 = blockIdx.x * 4, b0 = blockIdx.y * 4, tid = threadIdx.x;
  if (b0 > a0) return;
  const T *D = params + d, *U = params + 2 * (size_t)d;
  double acc[16] = {};
  for (int i = tid; i < d; i += 256) {
    const double id = 1.0 / (double)D[i];
    double ua[4], ub[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      ua[k] = (a0 + k < r) ? (double)U[i + (size_t)(a0 + k) * d] * id : 0.0;
      ub[k] = (b0 + k < r) ? (double)U[i + (size_t)(b0 + k) * d] * id : 0.0;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[k * 4 + j] += ua[k] * ub[j];
  }
  lowr_block_sums<16>(acc, red, out);
  double *A = prep + lowr_off_a(r);
  if (tid < 16) {
    const int a = a0 + tid / 4, b = b0 + tid % 4;
    if (a < r && b <= a) A[(size_t)a * r + b] = out[tid] + (a == b ? 1.0 : 0.0);
  }
}

// ---- draws + parameter-only preparation ----------------------------------------------------------------------------------------------
// workgroup 0 (with_prep): A (its own K = d reduction unless gram_done), Cholesky, A^-1, the two log sums, the non-positive-scale flag.
// the others: thread = one Philox block, rows 4 q .. 4 q + 3 of column m of the (d + r)-row stream
template <typename T>
__global__ __launch_bounds__(256) void k_lowr_draw_prep(int d, int r, int M, RngArgs rng, T *__restrict__ E, int with_prep, int gram_done,
                                                      const T *__restrict__ params, double *__restrict__ prep, int *status) {
  __shared__ double L[64 * 65 / 2];   // the factor's lower triangle, packed by rows: (i, k) at i (i + 1) / 2 + k
  __shared__ double W[64 * 65];       // A^-1 in the making: W[i][j], thread j owns column j
  __shared__ double red[2 * 4];
  __shared__ int bad_piv;
  const int tid = threadIdx.x;
  if ((int)blockIdx.x >= with_prep) {
    const int n = d + r, n4 = (n + 3) / 4;
    const long long t = (long long)(blockIdx.x - with_prep) * 256 + tid;
    if (t >= (long long)n4 * M) return;
    const int m = (int)(t / n4), q = (int)(t - (long long)m * n4);
    T e[4];
    eps_block<T>(rng.seed, rng_index(rng), (uint64_t)(rng.m_offset + m) * (uint64_t)n4 + (uint64_t)q, e);
    T *col = E + (size_t)m * n;
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (4 * q + j < n) col[4 * q + j] = e[j];
    return;
  }
  const int lane = tid & 63, wv = tid >> 6;
  const T *D = params + d, *U = params + 2 * (size_t)d;
  if (tid == 0) bad_piv = 0;
  // sum log D and the non-positive / non-finite count
  double sl = 0.0, bad = 0.0;
  for (int i = tid; i < d; i += 256) {
    const double di = (double)D[i];
    if (!(di > 0.0) || !isfinite(di)) bad = 1.0;
    sl += log(di);
  }
  double v2[2] = {sl, bad};
  block_sum_n<double, 256, 2>(v2, red);
  if (gram_done) {
    const double *A = prep + lowr_off_a(r);
    for (int t = tid; t < r * r; t += 256) {
      const int a = t / r, b = t % r;
      if (b <= a) L[LT(a, b)] = A[(size_t)a * r + b];
    }
  } else {   // lower triangle: one wave per entry, lanes over the K = d axis
    const int n_ent = r * (r + 1) / 2;
    for (int e = wv; e < n_ent; e += 4) {
      int a = (int)((sqrt(8.0 * e + 1.0) - 1.0) * 0.5);
      while (a * (a + 1) / 2 > e) --a;
      while ((a + 1) * (a + 2) / 2 <= e) ++a;
      const int b = e - a * (a + 1) / 2;
      double s = 0.0;
      for (int i = lane; i < d; i += 64) {
        const double id = 1.0 / (double)D[i];
        s += ((double)U[i + (size_t)a * d] * id) * ((double)U[i + (size_t)b * d] * id);
      }
      s = wave_sum(s);
      if (lane == 0) L[LT(a, b)] = s + (a == b ? 1.0 : 0.0);
    }
  }
  __syncthreads();
  // Cholesky factor in place (right-looking), r <= 64
  double hl = 0.0;   // (thread 0) sum log L_jj = 1/2 logdet A
  for (int j = 0; j < r; ++j) {
    if (tid == 0) {
      const double p = L[LT(j, j)];
      if (!(p > 0.0) || !isfinite(p)) bad_piv = 1;
      const double l = sqrt(p);
      L[LT(j, j)] = l;
      hl += log(l);
    }
    __syncthreads();
    const double ljj = L[LT(j, j)];
    for (int i = j + 1 + tid; i < r; i += 256) L[LT(i, j)] /= ljj;
    __syncthreads();
    for (int i = j + 1 + (tid >> 4); i < r; i += 16)   // 16 x 16 threads over the trailing block's lower triangle
      for (int k = j + 1 + (tid & 15); k <= i; k += 16) L[LT(i, k)] -= L[LT(i, j)] * L[LT(k, j)];
    __syncthreads();
  }
  // A^-1 column by column: L y = e_j, L' x = y (thread j owns column j of W), then out to the global block
  if (tid < r) {
    const int j = tid;
    for (int i = 0; i < j; ++i) W[i * 65 + j] = 0.0;
    for (int i = j; i < r; ++i) {
      double s = (i == j) ? 1.0 : 0.0;
      for (int k = j; k < i; ++k) s -= L[LT(i, k)] * W[k * 65 + j];
      W[i * 65 + j] = s / L[LT(i, i)];
    }
    for (int i = r - 1; i >= 0; --i) {
      double s = W[i * 65 + j];
      for (int k = i + 1; k < r; ++k) s -= L[LT(k, i)] * W[k * 65 + j];
      W[i * 65 + j] = s / L[LT(i, i)];
    }
  }
  __syncthreads();
  double *Ainv = prep + lowr_off_ainv();
  for (int t = tid; t < r * r; t += 256) Ainv[t] = W[(t % r) * 65 + t / r];   // column-major: entry (i, j) at j r + i
  if (tid == 0) {
    prep[0] = v2[0];
    prep[1] = hl;
    if ((v2[1] > 0.0 || bad_piv) && status) atomicOr(status, 2);
  }
}

// ---- sample: thread = row i, workgroup = 256 rows x MT columns --------------------------------------------------------------------
template <typename T, int MT>
__global__ __launch_bounds__(256) void k_lowr_sample(int d, int r, int M, const T *__restrict__ params, const T *__restrict__ E,
                                                   T *__restrict__ Z, T *__restrict__ tbuf) {
  __shared__ T B[64 * MT];   // u2 of the column tile: B[k][j]
  const int n = d + r, m0 = blockIdx.y * MT, i = blockIdx.x * 256 + threadIdx.x;
  for (int t = threadIdx.x; t < r * MT; t += 256) {
    const int k = t / MT, j = t % MT;
    B[t] = (m0 + j < M) ? E[(size_t)(m0 + j) * n + d + k] : T(0);
  }
  __syncthreads();
  if (i >= d) return;
  const T *U = params + 2 * (size_t)d;
  T acc[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) acc[j] = T(0);
  for (int k = 0; k < r; ++k) {
    const T u = U[i + (size_t)k * d];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] = fma(u, B[k * MT + j], acc[j]);
  }
  const T mu = params[i], Dv = params[d + i];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = m0 + j;
    if (m < M) {
      const T u1 = E[(size_t)m * n + i];
      Z[(size_t)m * d + i] = fma(Dv, u1, acc[j]) + mu;
      if (tbuf) tbuf[(size_t)m * d + i] = u1 + acc[j] / Dv;
    }
  }
}

// ---- s = U' D^-1 t and |t|^2: one workgroup per 4 x 4 tile of (k, m), its threads over the K = d axis ---------------------------------
template <typename T>
__global__ __launch_bounds__(256) void k_lowr_s(int d, int r, int M, const T *__restrict__ params, const T *__restrict__ tbuf,
                                                double *__restrict__ sbuf, double *__restrict__ ttbuf) {
  __shared__ double red[20 * 256], out[20 * 9];
  const int k0 = blockIdx.x * 4, m0 = blockIdx.y * 4, tid = threadIdx.x;
  const T *D = params + d, *U = params + 2 * (size_t)d;
  double acc[20] = {};   // [a * 4 + j]: s of (k0 + a, m0 + j); [16 + j]: |t|^2 of column m0 + j
  for (int i = tid; i < d; i += 256) {
    const double id = 1.0 / (double)D[i];
    double u[4], tv[4];
#pragma unroll
    for (int a = 0; a < 4; ++a) u[a] = (k0 + a < r) ? (double)U[i + (size_t)(k0 + a) * d] * id : 0.0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      tv[j] = (m0 + j < M) ? (double)tbuf[(size_t)(m0 + j) * d + i] : 0.0;
      acc[16 + j] += tv[j] * tv[j];
    }
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
      for (int j = 0; j < 4; ++j) acc[a * 4 + j] += u[a] * tv[j];
  }
  lowr_block_sums<20>(acc, red, out);
  if (tid < 16) {
    const int k = k0 + tid / 4, m = m0 + tid % 4;
    if (k < r && m < M) sbuf[(size_t)m * r + k] = out[tid];
  } else if (tid < 20 && blockIdx.x == 0 && m0 + tid - 16 < M) {
    ttbuf[m0 + tid - 16] = out[tid];
  }
}

// ---- x = A^-1 s, log q, V = D^-1 (t - D^-1 U x) in place over t: the sample kernel's shape, s and x in f64 ----------------------------------
// every workgroup forms x of its MT columns (r^2 MT flops: cheaper than a launch); the workgroups of row block 0 leave x and log q
template <typename T, int MT>
__global__ __launch_bounds__(256) void k_lowr_xv(int d, int r, int M, const T *__restrict__ params, const double *__restrict__ prep,
                                               const double *__restrict__ sbuf, const double *__restrict__ ttbuf, double *__restrict__ xbuf,
                                               double *__restrict__ lq, T *__restrict__ V) {
  __shared__ double S[64 * MT], B[64 * MT];
  const int m0 = blockIdx.y * MT, i = blockIdx.x * 256 + threadIdx.x;
  const double *Ainv = prep + lowr_off_ainv();
  for (int t = threadIdx.x; t < r * MT; t += 256) {
    const int k = t / MT, j = t % MT;
    S[t] = (m0 + j < M) ? sbuf[(size_t)(m0 + j) * r + k] : 0.0;
  }
  __syncthreads();
  for (int t = threadIdx.x; t < r * MT; t += 256) {
    const int k = t / MT, j = t % MT;
    double x = 0.0;
    for (int a = 0; a < r; ++a) x += Ainv[(size_t)a * r + k] * S[a * MT + j];   // (A^-1 is symmetric: column a read along k)
    B[t] = x;
    if (blockIdx.x == 0 && m0 + j < M) xbuf[(size_t)(m0 + j) * r + k] = x;
  }
  __syncthreads();
  if (blockIdx.x == 0 && threadIdx.x < MT && m0 + (int)threadIdx.x < M) {
    const int j = threadIdx.x;
    double sx = 0.0;
    for (int k = 0; k < r; ++k) sx += S[k * MT + j] * B[k * MT + j];
    lq[m0 + j] = -0.5 * d * kLog2Pi - prep[0] - prep[1] - 0.5 * (ttbuf[m0 + j] - sx);
  }
  if (!V || i >= d) return;
  const T *U = params + 2 * (size_t)d;
  double acc[MT];
#pragma unroll
  for (int j = 0; j < MT; ++j) acc[j] = 0.0;
  for (int k = 0; k < r; ++k) {
    const double u = (double)U[i + (size_t)k * d];
#pragma unroll
    for (int j = 0; j < MT; ++j) acc[j] += u * B[k * MT + j];
  }
  const double id = 1.0 / (double)params[d + i];
#pragma unroll
  for (int j = 0; j < MT; ++j) {
    const int m = m0 + j;
    if (m < M) V[(size_t)m * d + i] = (T)(((double)V[(size_t)m * d + i] - id * acc[j]) * id);
  }
}

// ---- VJP: workgroup = 64 rows x RB columns of U x one slice of the sample axis; its four waves deal the slice's columns, lane = row ---------
// mode 0: cotangent G, (a1, a2) = (u1, u2)                                  closed-form estimators
// mode 1: cotangent G + V                                                    sticking the landing
// mode 2: mode 0 plus cotangent V with (a1, a2) = (u1 - D o V, u2 - x)       Monte-Carlo entropy (U' V = x exactly: A x = s)
// part[slice][entry]: the un-normalised f64 sums of the slice, laid out like the gradient
template <typename T, int RB>
__global__ __launch_bounds__(256) void k_lowr_vjp(int d, int r, int M, int mode, const T *__restrict__ params, const T *__restrict__ E,
                                                const T *__restrict__ G, const T *__restrict__ V, const double *__restrict__ xbuf,
                                                double *__restrict__ part) {
  __shared__ double red[4][RB + 2][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int i = blockIdx.x * 64 + lane, k0 = blockIdx.y * RB, n = d + r;
  const int Mb = (M + (int)gridDim.z - 1) / (int)gridDim.z, m_lo = blockIdx.z * Mb, m_hi = m_lo + Mb < M ? m_lo + Mb : M;
  const bool row = i < d;
  const int ic = row ? i : d - 1;
  const double Dv = (double)params[d + ic];
  double gm = 0.0, gD = 0.0, gU[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) gU[j] = 0.0;
  int kk[RB];
#pragma unroll
  for (int j = 0; j < RB; ++j) kk[j] = (k0 + j < r) ? k0 + j : r - 1;
  for (int m = m_lo + wv; m < m_hi; m += 4) {
    const T *e = E + (size_t)m * n;
    const double u1 = (double)e[ic];
    double c1 = (double)G[(size_t)m * d + ic];
    double v = 0.0;
    if (mode != 0) v = (double)V[(size_t)m * d + ic];
    if (mode == 1) c1 += v;
    gm += c1;
    gD += c1 * u1;
    if (mode == 2) {
      gD += v * (u1 - Dv * v);
      const double *x = xbuf + (size_t)m * r;
#pragma unroll
      for (int j = 0; j < RB; ++j) {
        const double u2 = (double)e[d + kk[j]];
        gU[j] += c1 * u2 + v * (u2 - x[kk[j]]);
      }
    } else {
#pragma unroll
      for (int j = 0; j < RB; ++j) gU[j] += c1 * (double)e[d + kk[j]];
    }
  }
  red[wv][0][lane] = gm;
  red[wv][1][lane] = gD;
#pragma unroll
  for (int j = 0; j < RB; ++j) red[wv][2 + j][lane] = gU[j];
  __syncthreads();
  const size_t plen = 2 * (size_t)d + (size_t)d * r;
  double *dst = part + (size_t)blockIdx.z * plen;
  for (int t = threadIdx.x; t < (RB + 2) * 64; t += 256) {
    const int q = t >> 6, l = t & 63, ii = blockIdx.x * 64 + l;
    if (ii >= d) continue;
    const double s = ((red[0][q][l] + red[1][q][l]) + red[2][q][l]) + red[3][q][l];
    if (q < 2) {
      if (blockIdx.y == 0) dst[(size_t)q * d + ii] = s;
    } else if (k0 + q - 2 < r) {
      dst[2 * (size_t)d + ii + (size_t)(k0 + q - 2) * d] = s;
    }
  }
}

// ---- finish: the gradient entries and (last workgroup) the objective value -------------------------------------------------------------
// grad = -(sum of the slices' partials) / M - cH dH, dH formed per entry from A^-1: dH/dU_ib = D_i^-2 (U A^-1)_ib,
// dH/dD_i = 1/D_i - D_i^-3 (U A^-1 U')_ii.  value = -(sum ell / M + H) for the closed-form estimators, -(sum ell / M) + mean log q for the
// others; H = d/2 (1 + log 2 pi) + sum log D + 1/2 logdet A
template <typename T>
__global__ __launch_bounds__(256) void k_lowr_finish(int d, int r, int n_slices, int n_grad_blocks, const T *__restrict__ params,
                                                   const double *__restrict__ part, const double *__restrict__ prep,
                                                   const double *__restrict__ lq, ValueIn vin, OutArgs out) {
  __shared__ double red[2 * 4];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n_grad_blocks) {
    const size_t plen = 2 * (size_t)d + (size_t)d * r;
    const double cH = direct_entropy_coeff(out.ent_kind);
    const double *Ainv = prep + lowr_off_ainv();
    const T *U = params + 2 * (size_t)d;
    const int n_d_blocks = (d + 3) / 4;
    if ((int)blockIdx.x < n_d_blocks) {   // the scale diagonal's entries: one wave per row i, lane b forms (U A^-1)_ib
      const int i = blockIdx.x * 4 + (tid >> 6), b = tid & 63;
      if (i >= d) return;
      double g = 0.0;
      for (int s = 0; s < n_slices; ++s) g += part[(size_t)s * plen + d + i];
      double dH = 0.0;
      if (cH != 0.0) {
        double ua = 0.0;
        if (b < r) {
          for (int a = 0; a < r; ++a) ua += (double)U[i + (size_t)a * d] * Ainv[(size_t)a * r + b];   // (A^-1 is symmetric: row a read along b)
          ua *= (double)U[i + (size_t)b * d];
        }
        const double diag = wave_sum(ua), id = 1.0 / (double)params[d + i];
        dH = id - id * id * id * diag;
      }
      if (b == 0) ((T *)out.grad)[d + i] = (T)(-g / (double)out.M_total - cH * dH);
      return;
    }
    const size_t t = (size_t)(blockIdx.x - n_d_blocks) * 256 + tid;
    if (t >= plen || (t >= (size_t)d && t < 2 * (size_t)d)) return;
    double g = 0.0;
    for (int s = 0; s < n_slices; ++s) g += part[(size_t)s * plen + t];
    double dH = 0.0;
    if (cH != 0.0 && t >= (size_t)d) {   // a factor entry (i, b)
      const size_t o = t - 2 * (size_t)d;
      const int b = (int)(o / d), i = (int)(o - (size_t)b * d);
      const double id = 1.0 / (double)params[d + i];
      double ua = 0.0;
      for (int a = 0; a < r; ++a) ua += (double)U[i + (size_t)a * d] * Ainv[(size_t)b * r + a];
      dH = id * id * ua;
    }
    ((T *)out.grad)[t] = (T)(-g / (double)out.M_total - cH * dH);
    return;
  }
  double s_ell = 0.0, s_lq = 0.0;
  for (int i = tid; i < vin.n_ell_part; i += 256) s_ell += vin.ell_part[i];
  for (int i = tid; i < vin.n_ell; i += 256) s_ell += (double)((const T *)vin.ell)[i];
  const bool closed = ent_is_closed(out.ent_kind);
  if (!closed)
    for (int i = tid; i < out.M_local; i += 256) s_lq += lq[i];
  double v[2] = {s_ell, s_lq};
  block_sum_n<double, 256, 2>(v, red);
  if (tid == 0) {
    const double Mt = (double)out.M_total;
    const double energy = (v[0] + (double)out.M_local * vin.ell_const) / Mt;
    const double value = closed ? -(energy + 0.5 * d * (1.0 + kLog2Pi) + prep[0] + prep[1]) : -energy + v[1] / Mt;
    *(T *)out.value = (T)value;
    if (!isfinite(value) && out.status) atomicOr(out.status, 1);
    if (out.elbo_rec) out.elbo_rec[out.rec_slot] = -value;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
// the draws of M columns -> lowr_E; params != nullptr: also the parameter-only preparation -> lowr_prep
void launch_lowr_draw_prep(mivi_ctx *c, const RngArgs &rng, int M, const void *params, double *prep) {
  if (!prep) prep = (double *)c->lowr_prep.p;
  const int d = c->cfg.d, r = c->cfg.rank;
  const long long nt = (long long)((d + r + 3) / 4) * M;
  const int with_prep = params ? 1 : 0, gram = (params && r > 4) ? 1 : 0;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    if (gram) hipLaunchKernelGGL(k_lowr_gram<T>, dim3((r + 3) / 4, (r + 3) / 4), dim3(256), 0, c->stream, d, r, (const T *)params, prep);
    hipLaunchKernelGGL(k_lowr_draw_prep<T>, dim3((unsigned)((nt + 255) / 256) + with_prep), dim3(256), 0, c->stream, d, r, M, rng, (T *)c->lowr_E.p, with_prep,
                       gram, (const T *)params, prep, (int *)c->status.p);
  });
}

void launch_lowr_sample(mivi_ctx *c, const void *params, int M, void *Z, bool with_t) {
  const int d = c->cfg.d, r = c->cfg.rank;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_lowr_sample<T, 8>), dim3((d + 255) / 256, (M + 7) / 8), dim3(256), 0, c->stream, d, r, M, (const T *)params, (const T *)c->lowr_E.p,
                       (T *)Z, with_t ? (T *)c->lowr_V.p : (T *)nullptr);
  });
}

static double *lowr_sx_part(double *sx, size_t r, size_t cap, int which) {   // f64 [s (r x cap) | x (r x cap) | |t|^2 (cap) | log q (cap)]
  const size_t off[4] = {0, r * cap, 2 * r * cap, (2 * r + 1) * cap};
  return sx + off[which];
}
static double *lowr_sx_part(const mivi_ctx *c, int which) { return lowr_sx_part((double *)c->lowr_sx.p, c->cfg.rank, c->cap_M, which); }
double *lowr_logq_of(const mivi_ctx *c, const LowrPoints &pts) { return lowr_sx_part(pts.sx, c->cfg.rank, pts.cap, 3); }

// t (in lowr_V, or pts->t) -> s, x, log q and V = Sigma^-1 (z - m) (over t)
void launch_lowr_woodbury(mivi_ctx *c, const void *params, int M, bool want_v, const LowrPoints *pts) {
  const int d = c->cfg.d, r = c->cfg.rank;
  const LowrPoints own{c->lowr_V.p, (double *)c->lowr_prep.p, (double *)c->lowr_sx.p, (size_t)c->cap_M};
  const LowrPoints &P = pts ? *pts : own;
  double *s = lowr_sx_part(P.sx, r, P.cap, 0), *x = lowr_sx_part(P.sx, r, P.cap, 1), *tt = lowr_sx_part(P.sx, r, P.cap, 2), *lq = lowr_sx_part(P.sx, r, P.cap, 3);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_lowr_s<T>, dim3((r + 3) / 4, (M + 3) / 4), dim3(256), 0, c->stream, d, r, M, (const T *)params, (const T *)P.t, s, tt);
    hipLaunchKernelGGL((k_lowr_xv<T, 8>), dim3(want_v ? (d + 255) / 256 : 1, (M + 7) / 8), dim3(256), 0, c->stream, d, r, M, (const T *)params,
                       (const double *)P.prep, (const double *)s, (const double *)tt, x, lq, want_v ? (T *)P.t : (T *)nullptr);
  });
}

// the VJP's partials, then (or alone: want_grad == 0) the finish: out.grad, out.value, the non-finite flag, the elbo record
void launch_lowr_vjp_finish(mivi_ctx *c, const void *params, int M, int want_grad, const ValueIn &vin, const OutArgs &out) {
  const int d = c->cfg.d, r = c->cfg.rank;
  const int mode = out.ent_kind == MIVI_ENT_MONTE_CARLO ? 2 : ((out.ent_kind == MIVI_ENT_STL || out.ent_kind == MIVI_ENT_STL_ZERO_GRAD) ? 1 : 0);
  const int ns = lowr_vjp_slices(M);
  const size_t plen = 2 * (size_t)d + (size_t)d * r;
  const int ngb = want_grad ? (int)((plen + 255) / 256) + (d + 3) / 4 : 0;   // the scale diagonal's waves, then one thread per entry
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    if (want_grad)
      hipLaunchKernelGGL((k_lowr_vjp<T, 16>), dim3((d + 63) / 64, (r + 15) / 16, ns), dim3(256), 0, c->stream, d, r, M, mode, (const T *)params,
                         (const T *)c->lowr_E.p, (const T *)c->W.p, (const T *)c->lowr_V.p, (const double *)lowr_sx_part(c, 1), (double *)c->lowr_part.p);
    hipLaunchKernelGGL(k_lowr_finish<T>, dim3(ngb + 1), dim3(256), 0, c->stream, d, r, ns, ngb, (const T *)params, (const double *)c->lowr_part.p,
                       (const double *)c->lowr_prep.p, (const double *)lowr_sx_part(c, 3), vin, out);
  });
}

}  // namespace mivi
