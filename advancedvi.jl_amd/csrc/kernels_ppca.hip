// The probabilistic PCA / Bayesian factor model target (include/mivi.h, mivi_set_target_ppca): theta = [vec W (D x k, column c contiguous);
// Z (k x N, z_r contiguous); mu (D); a (k, with ARD); s] per sample column of the context's Z plane, pred_rj = mu_j + W_j. . z_r.
// api_ppca.hip sets the target and the row selection; eval_generic_target reaches launch_ppca_target.
//
//   k_ppca_rows      grid (row slice, sample), 64 x waves threads (waves = min(4, ceil(D / 16))).  ONE pass over Y does the likelihood and
//                    every gradient.  The workgroup stages its sample's W into LDS once, as [KP][ldw] (the layout of theta: row c is column
//                    c of W; KP = k padded to 16 and the columns past D are zero), and walks its rows in tiles of 16 (through the row index
//                    vector, if one is set).  The waves split the FEATURE axis: wave w owns the NB blocks of 16 columns from 16 NB w on.
//                    A tile of Z is staged once, as [16][KP + 1]; every wave takes its fragments of it into registers ahead of its blocks
//                    (the A operand of the forward product, the B operand of dW), so per block on the 16 x 16 x 4 matrix cores (Mfma16):
//                      pred = Z_tile (A, registers) . W_blk' (B, LDS), K = k;
//                      res  = m (y - mu - pred) in f64 straight from Y and the mask: squared error, count and dmu in f64 per lane;
//                      dW_blk += res' (A: the lane's OWN four accumulator rows -- the K order of a tile's 16 rows is permuted the same way
//                                in both operands) . Z_tile (B, registers), accumulated in registers across the whole slice;
//                      dZ_tile += res (A: transposed through a wave-private [16][17] LDS block) . W_blk (B, LDS), over the wave's blocks.
//                    dW and dmu are private to the wave: no reduction across waves.  f32 dW accumulators are flushed into the slice's f64
//                    partial every kPpcaFlush rows.  dZ_tile sums over D and so over waves: every wave leaves its 16 x k partial in LDS,
//                    they are added in wave order and the finished rows go straight into G at the ORIGINAL row id (a row belongs to one
//                    slice: no partial planes for dZ).  e^{-2s} and likeadj multiply the sums once, in f64, where they are stored.
//   k_ppca_clear_z   with a row selection in force: zeros in the Z block of G ahead of the rows kernel (ordinary stores, no memset).
//   k_ppca_finish_w  one thread per entry of W and mu: the slices' partials in slice order, e^{-2s}, likeadj and the prior.
//   k_ppca_finish    one workgroup per sample: the scalar partials in slice order, |W_c|^2 per column, |mu|^2, the priors, d/da, d/ds and
//                    the value -- all f64, rounded once into ell (M) and G (d x M).
// Every store is an ordinary one, nothing is accumulated atomically and no geometry depends on the chunking of the samples: results are
// bitwise reproducible and the same for every partial cap.
#include "flow_tile.h"

namespace mivi {

constexpr int kPpcaEld = kFlowTile + 1;   // stride of the wave-private [16][16] residual block
constexpr int kPpcaFlush = 128;           // rows between two flushes of the f32 dW accumulators into the f64 partial
constexpr size_t kPpcaLdsMax = 160 * 1024;   // gfx950's LDS per workgroup

template <typename T>
struct PpcaArgs {
  int D, k, d, ldw;          // ldw: stride of a row of W in LDS
  int M, m0;                 // samples of this chunk; the chunk's first sample column in Z / ell / G
  long long n, nr;           // rows of the data set (Y's leading dimension); rows evaluated
  const T *Y;                // n x D column-major
  const unsigned char *mask; // the same layout, or nullptr: all observed
  const long long *rows;     // the selection (nr entries) or nullptr: rows 0 .. nr - 1
  const T *Z;                // d x M_total, ld d
  double *part;              // [n_sl][M][plen]: dW (D k), dmu (D), squared error, observed count, |z|^2 of the slice's rows
  long long plen;
  int n_sl;
  long long rps;             // rows per slice, a multiple of 16
  T *G, *ell;                // d x M_total; M_total
  int ard, want_grad;
  double prior_std, mean_std, noise_scale, likeadj;
};

__device__ __forceinline__ void ppca_wave_sync() {   // LDS written by some lanes of a wave, read by others of the same wave
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// the wave's dW tiles -> the slice's f64 partial (added to it after the first flush); the accumulators restart at zero
template <typename T, int NB, int NC>
__device__ __forceinline__ void ppca_flush(const PpcaArgs<T> &a, typename Mfma16<T>::acc_t (&dW)[NB][NC], double *part, int w, bool add) {
  const int lane = threadIdx.x & 63, col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int b = 0; b < NB; ++b) {
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int j = 16 * (w * NB + b) + Mfma16<T>::row(kq, r), c = 16 * cb + col;
        if (j < a.D && c < a.k) {
          double *dst = part + (size_t)c * a.D + j;
          *dst = add ? *dst + (double)dW[b][cb][r] : (double)dW[b][cb][r];
        }
        dW[b][cb][r] = T(0);
      }
    }
  }
}

template <typename T, int NB, int NC>
__global__ __launch_bounds__(256) void k_ppca_rows(PpcaArgs<T> a) {
  using acc_t = typename Mfma16<T>::acc_t;
  constexpr int KP = 16 * NC, ldz = KP + 1;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, kq = lane >> 4, nthr = blockDim.x, waves = nthr >> 6;
  T *Wl = reinterpret_cast<T *>(flow_lds);   // [KP][ldw]
  T *Zt = Wl + (size_t)KP * a.ldw;           // [16][ldz]: the tile of Z
  T *Pall = Zt + kFlowTile * ldz;            // [waves][16][ldz]: the waves' dZ partials of a tile ...
  T *Pw = Pall + w * kFlowTile * ldz;        // ... whose head is this wave's residual block Et [16][17] while it walks its column blocks
  __shared__ long long rid[kFlowTile];
  __shared__ double red[12];
  const int sl = blockIdx.x, ml = blockIdx.y;
  const size_t zc = (size_t)(a.m0 + ml) * a.d, oZ = (size_t)a.D * a.k, oMu = oZ + (size_t)a.n * a.k;
  const T *th = a.Z + zc;
  for (int c = 0; c < KP; ++c)   // this sample's W: zero rows past k, zero columns past D
    for (int j = tid; j < a.ldw; j += nthr) Wl[c * a.ldw + j] = (c < a.k && j < a.D) ? th[(size_t)c * a.D + j] : T(0);
  double mu[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    const int j = 16 * (w * NB + b) + col;
    mu[b] = j < a.D ? (double)th[oMu + j] : 0.0;
  }
  const double em2 = exp(-2.0 * (double)th[a.d - 1]);
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  acc_t dW[NB][NC];
  double dmu[NB];
#pragma unroll
  for (int b = 0; b < NB; ++b) {
    dmu[b] = 0.0;
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) dW[b][cb] = acc_t{0, 0, 0, 0};
  }
  double v[3] = {0.0, 0.0, 0.0};   // this thread's share of the squared error, the observed count and |z|^2
  int since = 0;
  bool flushed = false;
  double *part = a.part + ((size_t)sl * a.M + ml) * a.plen;
  for (long long rr = rbeg; rr < rend; rr += kFlowTile) {
    __syncthreads();   // the previous tile is done with Zt, rid and the partials (and, the first time, W is staged)
    for (int e = tid; e < kFlowTile * KP; e += nthr) {
      const int row = e / KP, c = e - row * KP;
      const long long i = rr + row, ri = i < rend ? (a.rows ? a.rows[i] : i) : -1;
      const T z = (ri >= 0 && c < a.k) ? th[oZ + (size_t)ri * a.k + c] : T(0);
      Zt[row * ldz + c] = z;
      v[2] += (double)z * (double)z;
      if (c == 0) rid[row] = ri;
    }
    __syncthreads();
    long long ri4[4];
    T za[KP / 4], zb[NC][4];
#pragma unroll
    for (int r = 0; r < 4; ++r) ri4[r] = rid[Mfma16<T>::row(kq, r)];
#pragma unroll
    for (int q = 0; q < KP / 4; ++q) za[q] = Zt[col * ldz + 4 * q + kq];
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) {
#pragma unroll
      for (int t = 0; t < 4; ++t) zb[cb][t] = Zt[Mfma16<T>::row(kq, t) * ldz + 16 * cb + col];
    }
    acc_t dz[NC];
#pragma unroll
    for (int cb = 0; cb < NC; ++cb) dz[cb] = acc_t{0, 0, 0, 0};
#pragma unroll
    for (int b = 0; b < NB; ++b) {
      const int j0 = 16 * (w * NB + b), j = j0 + col;
      if (j0 < a.D) {   // (wave-uniform)
        acc_t pr = acc_t{0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < KP / 4; ++q)
          if (4 * q < a.k) pr = Mfma16<T>::mma(za[q], Wl[(4 * q + kq) * a.ldw + j], pr);
        acc_t e;
        double sm = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {   // (row, column j): the masked residual in f64, read straight from Y
          double res = 0.0;
          if (j < a.D && ri4[r] >= 0) {
            const size_t at = (size_t)j * a.n + ri4[r];
            if (!a.mask || a.mask[at]) {
              res = (double)a.Y[at] - (mu[b] + (double)pr[r]);
              v[0] += res * res;
              v[1] += 1.0;
            }
          }
          sm += res;
          e[r] = (T)res;
        }
        dmu[b] += sm;
        if (a.want_grad) {
#pragma unroll
          for (int cb = 0; cb < NC; ++cb) {
#pragma unroll
            for (int t = 0; t < 4; ++t) dW[b][cb] = Mfma16<T>::mma(e[t], zb[cb][t], dW[b][cb]);
          }
          ppca_wave_sync();   // (the previous block's reads of Et are done)
#pragma unroll
          for (int r = 0; r < 4; ++r) Pw[Mfma16<T>::row(kq, r) * kPpcaEld + col] = e[r];
          ppca_wave_sync();
#pragma unroll
          for (int q = 0; q < 4; ++q) {
            const T ea = Pw[col * kPpcaEld + 4 * q + kq];
#pragma unroll
            for (int cb = 0; cb < NC; ++cb) dz[cb] = Mfma16<T>::mma(ea, Wl[(16 * cb + col) * a.ldw + j0 + 4 * q + kq], dz[cb]);
          }
        }
      }
    }
    if (a.want_grad) {
      ppca_wave_sync();
#pragma unroll
      for (int cb = 0; cb < NC; ++cb) {
#pragma unroll
        for (int r = 0; r < 4; ++r) Pw[Mfma16<T>::row(kq, r) * ldz + 16 * cb + col] = dz[cb][r];
      }
      __syncthreads();
      for (int e = tid; e < kFlowTile * a.k; e += nthr) {   // dz_r = likeadj (e^{-2s} sum_j res_rj W_j. - z_r), the waves in order
        const int row = e / a.k, c = e - row * a.k;
        const long long ri = rid[row];
        if (ri >= 0) {
          double x = 0.0;
          for (int u = 0; u < waves; ++u) x += (double)Pall[(u * kFlowTile + row) * ldz + c];
          a.G[zc + oZ + (size_t)ri * a.k + c] = (T)(a.likeadj * (em2 * x - (double)Zt[row * ldz + c]));
        }
      }
      if constexpr (sizeof(T) == 4) {
        since += kFlowTile;
        if (since >= kPpcaFlush) {
          ppca_flush<T, NB, NC>(a, dW, part, w, flushed);
          flushed = true;
          since = 0;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) v[i] = wave_sum(v[i]);
  __syncthreads();
  if (lane == 0)
    for (int i = 0; i < 3; ++i) red[3 * w + i] = v[i];
  __syncthreads();
  if (tid < 3) {
    double x = 0.0;
    for (int u = 0; u < waves; ++u) x += red[3 * u + tid];
    part[(size_t)a.D * a.k + a.D + tid] = x;
  }
  if (!a.want_grad) return;
  ppca_flush<T, NB, NC>(a, dW, part, w, flushed);
#pragma unroll
  for (int b = 0; b < NB; ++b) {   // the four row quarters of a column
    double x = dmu[b];
    x += __shfl_xor(x, 16, 64);
    x += __shfl_xor(x, 32, 64);
    const int j = 16 * (w * NB + b) + col;
    if (kq == 0 && j < a.D) part[(size_t)a.D * a.k + j] = x;
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ppca_clear_z(PpcaArgs<T> a) {
  const size_t nz = (size_t)a.n * a.k;
  T *g = a.G + (size_t)(a.m0 + blockIdx.y) * a.d + (size_t)a.D * a.k;
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nz; i += (size_t)gridDim.x * 256) g[i] = T(0);
}

template <typename T>
__global__ __launch_bounds__(256) void k_ppca_finish_w(PpcaArgs<T> a) {
  const int e = blockIdx.x * 256 + threadIdx.x, ml = blockIdx.y, dk = a.D * a.k;
  if (e >= dk + a.D) return;
  const size_t zc = (size_t)(a.m0 + ml) * a.d;
  const T *th = a.Z + zc;
  double x = 0.0;
  for (int sl = 0; sl < a.n_sl; ++sl) x += a.part[((size_t)sl * a.M + ml) * a.plen + e];
  x *= a.likeadj * exp(-2.0 * (double)th[a.d - 1]);
  if (e < dk) {
    const double wv = (double)th[e];
    const double ip = a.ard ? exp(-2.0 * (double)th[a.d - 1 - a.k + e / a.D]) : 1.0 / (a.prior_std * a.prior_std);
    a.G[zc + e] = (T)(x - wv * ip);
  } else {
    const size_t at = (size_t)dk + (size_t)a.n * a.k + (e - dk);
    a.G[zc + at] = (T)(x - (double)th[at] / (a.mean_std * a.mean_std));
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_ppca_finish(PpcaArgs<T> a) {
  __shared__ double red[16], colsq[32];
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, ml = blockIdx.x;
  const size_t zc = (size_t)(a.m0 + ml) * a.d, oMu = (size_t)a.D * a.k + (size_t)a.n * a.k;
  const T *th = a.Z + zc;
  for (int c = w; c < a.k; c += 4) {   // |W_c|^2: one wave per column
    double x = 0.0;
    for (int j = lane; j < a.D; j += 64) {
      const double wv = (double)th[(size_t)c * a.D + j];
      x += wv * wv;
    }
    x = wave_sum(x);
    if (lane == 0) colsq[c] = x;
  }
  double v[4] = {0.0, 0.0, 0.0, 0.0};   // squared error, observed count, |z|^2 over the slices; |mu|^2
  for (int sl = tid; sl < a.n_sl; sl += 256) {
    const double *p = a.part + ((size_t)sl * a.M + ml) * a.plen + (size_t)a.D * a.k + a.D;
    v[0] += p[0];
    v[1] += p[1];
    v[2] += p[2];
  }
  for (int j = tid; j < a.D; j += 256) {
    const double m = (double)th[oMu + j];
    v[3] += m * m;
  }
  block_sum_n<double, 256, 4>(v, red);   // (its barriers publish colsq too)
  const double s = (double)th[a.d - 1], ip2 = 1.0 / (a.prior_std * a.prior_std);
  const T *av = th + a.d - 1 - a.k;   // (with ARD)
  if (a.ard && a.want_grad && tid < a.k) {
    const double ac = (double)av[tid];
    a.G[zc + a.d - 1 - a.k + tid] = (T)(-(double)a.D + colsq[tid] * exp(-2.0 * ac) - exp(2.0 * ac) * ip2 + 1.0);
  }
  if (tid == 0) {
    const double e2 = exp(2.0 * s), em2 = exp(-2.0 * s), in2 = 1.0 / (a.noise_scale * a.noise_scale), hn = log(2.0) - 0.5 * kLog2Pi;
    double lp = -0.5 * v[3] / (a.mean_std * a.mean_std) - (double)a.D * (log(a.mean_std) + 0.5 * kLog2Pi)   // mu
                + hn - log(a.noise_scale) - 0.5 * e2 * in2 + s;                                              // sigma, with the Jacobian of s = log sigma
    for (int c = 0; c < a.k; ++c) {
      if (a.ard) {
        const double ac = (double)av[c];
        lp += -0.5 * colsq[c] * exp(-2.0 * ac) - (double)a.D * (ac + 0.5 * kLog2Pi) + hn - log(a.prior_std) - 0.5 * exp(2.0 * ac) * ip2 + ac;
      } else {
        lp += -0.5 * colsq[c] * ip2 - (double)a.D * (log(a.prior_std) + 0.5 * kLog2Pi);
      }
    }
    const double rows = -0.5 * em2 * v[0] - v[1] * (s + 0.5 * kLog2Pi) - 0.5 * v[2] - (double)a.nr * (0.5 * (double)a.k * kLog2Pi);
    a.ell[a.m0 + ml] = (T)(a.likeadj * rows + lp);
    if (a.want_grad) a.G[zc + a.d - 1] = (T)(a.likeadj * (em2 * v[0] - v[1]) - e2 * in2 + 1.0);
  }
}

// ---- the launches' geometry: a function of the evaluated rows, D, k and the precision alone ---------------------------------------------
static long long ppca_plen(const mivi_ctx *c) { return (long long)c->pp_D * c->pp.k + c->pp_D + 3; }

static RowSlices ppca_slices(const mivi_ctx *c) {   // (the row slices of the hierarchical GLM target: 256 rows, at most 1024 slices)
  return row_slices(c->pp_rows.nr, kHglmSliceRows, kHglmMaxSlices);
}
static int ppca_chunk(const mivi_ctx *c, const RowSlices &g, int M) {   // samples per chunk under the cap
  return samples_under_cap(c->pp_rows.cap ? c->pp_rows.cap : kPpcaPartCap, (size_t)g.n_sl * ppca_plen(c) * sizeof(double), M);
}

bool ppca_reserve(mivi_ctx *c, int M) {
  const RowSlices g = ppca_slices(c);
  return !ensure(c, c->pp_part, (size_t)g.n_sl * ppca_chunk(c, g, M) * ppca_plen(c) * sizeof(double), false);
}

template <typename T, int NB, int NC>
static bool ppca_rows_launch(mivi_ctx *c, const PpcaArgs<T> &a, int waves) {
  const size_t lds = ((size_t)16 * NC * a.ldw + (size_t)(1 + waves) * kFlowTile * (16 * NC + 1)) * sizeof(T);
  if (lds > kPpcaLdsMax) return false;
  if (lds > 48 * 1024 &&
      hipFuncSetAttribute(reinterpret_cast<const void *>(k_ppca_rows<T, NB, NC>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess)
    return false;
  hipLaunchKernelGGL((k_ppca_rows<T, NB, NC>), dim3(a.n_sl, a.M), dim3(64 * waves), lds, c->stream, a);
  return true;
}

template <typename T, int NB>
static bool ppca_rows_nc(mivi_ctx *c, const PpcaArgs<T> &a, int waves) {
  return a.k <= 16 ? ppca_rows_launch<T, NB, 1>(c, a, waves) : ppca_rows_launch<T, NB, 2>(c, a, waves);
}

template <typename T>
static bool ppca_impl(mivi_ctx *c, int M, int want_grad) {
  const RowSlices g = ppca_slices(c);
  const int Mc = ppca_chunk(c, g, M);
  PpcaArgs<T> a{};
  a.D = c->pp_D;
  a.k = c->pp.k;
  a.d = c->cfg.d;
  a.ldw = ((a.D + 63) & ~63) + 17;   // (the forward product reads 16 consecutive columns of 4 rows, dZ's 4 consecutive columns of 16 rows)
  a.n = c->pp_rows.n;
  a.nr = c->pp_rows.nr;
  a.Y = (const T *)c->pp_Y;
  a.mask = (const unsigned char *)c->pp_mask;
  a.rows = c->pp_rows.sel ? (const long long *)c->pp_rows.idx.p : nullptr;
  a.Z = (const T *)c->Z.p;
  a.part = (double *)c->pp_part.p;
  a.plen = ppca_plen(c);
  a.n_sl = g.n_sl;
  a.rps = g.rps;
  a.G = (T *)c->W.p;
  a.ell = (T *)c->ell.p;
  a.ard = c->pp.ard;
  a.want_grad = want_grad;
  a.prior_std = c->pp.prior_std;
  a.mean_std = c->pp.mean_std;
  a.noise_scale = c->pp.noise_scale;
  a.likeadj = c->pp_rows.likeadj;
  const int nblk = (a.D + 15) / 16, waves = nblk < 4 ? nblk : 4, nb = (nblk + waves - 1) / waves;   // nb <= 8 at D <= 512
  const size_t nz = (size_t)a.n * a.k;
  for (int m0 = 0; m0 < M; m0 += Mc) {   // chunks of samples: the f64 partials stay under their cap
    a.m0 = m0;
    a.M = M - m0 < Mc ? M - m0 : Mc;
    if (want_grad && a.rows)   // rows outside the selection: dz_r = 0, written here
      hipLaunchKernelGGL(k_ppca_clear_z<T>, dim3((unsigned)((nz + 255) / 256 < 4096 ? (nz + 255) / 256 : 4096), a.M), dim3(256), 0, c->stream, a);
    const bool ok = nb <= 1 ? ppca_rows_nc<T, 1>(c, a, waves) : nb <= 2 ? ppca_rows_nc<T, 2>(c, a, waves)
                  : nb <= 4 ? ppca_rows_nc<T, 4>(c, a, waves) : ppca_rows_nc<T, 8>(c, a, waves);
    if (!ok) return false;
    if (want_grad) hipLaunchKernelGGL(k_ppca_finish_w<T>, dim3((a.D * a.k + a.D + 255) / 256, a.M), dim3(256), 0, c->stream, a);
    hipLaunchKernelGGL(k_ppca_finish<T>, dim3(a.M), dim3(256), 0, c->stream, a);
  }
  return true;
}

// false: device allocation of the partials failed, or the runtime refused the kernel its LDS
bool launch_ppca_target(mivi_ctx *c, int M, int want_grad) {
  if (!ppca_reserve(c, M)) return false;
  return by_dtype(c, [&](auto t) { return ppca_impl<decltype(t)>(c, M, want_grad); });
}

}  // namespace mivi
