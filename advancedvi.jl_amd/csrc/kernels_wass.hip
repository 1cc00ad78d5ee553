// KLMinWassFwdBwd (stochastic proximal gradient descent in Wasserstein space, src/algorithms/klminwassfwdbwd.jl): the update of `step`
// (:105-114) on the device-resident [m; vec C] and Sigma (d x d column-major, both triangles bitwise mirrored; `init`'s Sigma = C C' is
// kernels_bam.hip's launch).  With (g, H) from the estimator and eta the step size:
//     m' = m + eta g        M = I + eta H'        Sh = Hermitian(M Sigma M')                       (H as it comes; Hermitian: the UPPER triangle mirrored)
//     Sigma' = (Sh + 2 eta I + sqrt(Hermitian(Sh (Sh + 4 eta I)))) / 2        C' = cholesky(Sigma').L
// The reference's sqrt is a d x d eigendecomposition.  Here it is built from products alone, by the coupled Newton-Schulz iteration:
//     A = Hermitian(Sh (Sh + 4 eta I))    c = |A|_F    Y_0 = A (1/c)    Z_0 = I
//     E_k = I - Z_k Y_k    r_k = |E_k|_F    Y_k+1 = Y_k + Y_k E_k / 2    Z_k+1 = Z_k + E_k Z_k / 2        sqrt(A) = sqrt(c) (Y + Y')/2
// The products Z Y, Y E and E Z are formed in FULL (mirroring a triangle inside the iteration destroys the coupling Z Y -> I and costs four to
// ten digits); Y is symmetrised once, at the end.  The iteration stops at the first round k with
//     r_k <= 64 d eps,   or from k >= 4:   r_k >= r_k-1,   or   r_k >= r_k-1 / 2 and r_k < 1e-6        (stagnated: iterating on lets Y and Z run away)
// and Y_k is the result; a non-finite r_k also stops it.  Nothing goes to the host for that: the workgroups of round k's second launch each
// add the round's tile partials in one fixed order, decide alike, and the first of them records the decision for the launches behind it
// (ctl), which return at once.  kWassMaxRounds rounds are launched; none stopping, or a non-finite r_k (a NaN in g or H), sets the sticky
// non-finite flag.  All of it FLOAT64 on the matrix cores for either context type (an f32 context's parameters, state, g and H are converted
// where they are loaded and stored: the square root and the factorisation of Sigma' rounded to float32 lose kappa(Sigma') x 6e-8).
// Launches, nT = ceil(d / 64), any d >= 1 (a small d only makes the grids one workgroup each):
//     prep    N = M' = I + eta H, Sigma, Z_0 = I_d -- zero-padded to ldp = 64 nT; the identity on the padding of the work matrix W; m'
//     mt, sh  T = M Sigma over all tiles; the upper tiles of T M', mirrored: Sh
//     a       the upper tiles of Sh (Sh + 4 eta I), mirrored: A; one partial of |A|_F^2 per tile
//     e(k)    E_k, one partial of r_k^2 per tile                                                           (nT^2 workgroups)
//     yz(k)   the stop rule on r_k; Y_k+1 | Z_k+1                                                          (2 nT^2 workgroups)
//     sigma   the lower tiles of Sigma', mirrored bitwise into the state and, with rows and columns REVERSED, into W
//     factor  kernels_natgrad.hip's blocked factorisation of W and its finish: C' (exact zeros above the diagonal), entropy(q'), elbo, flags
// 2 nT + 2 kWassMaxRounds + 5 launches.  No floating-point atomics, one summation order: bitwise repeatable.  g and H are read-only.
#include "mivi_internal.h"
#include "ngd_tile.h"

#include <cmath>

namespace mivi {

constexpr int kWassMaxRounds = MIVI_WASS_MAX_ROUNDS;   // 11 to 34 rounds on non-singular inputs, at most 57 with a singular M

template <typename TI>
struct WassArgs {
  int d, nT, ldp, k;           // k: the round of this launch (e, yz)
  TI *params;                  // [m (d); vec C (d x d, column-major)] in / out
  TI *state;                   // Sigma (d x d) in / out
  const TI *grad, *hess;       // g (d), H (d x d, column-major)
  double *N, *P, *T, *Sh, *A;  // ldp x ldp each, zero beyond d.  After `a`: N and P hold Y_k (k odd / even, k >= 1), T holds E_k
  double *Z0, *Z1;             // Z_k, k even / odd
  double *W;                   // Sigma' reversed (the identity on its padding), then its factor
  double *part_a, *part_e;     // the tile partials of |A|_F^2 (n_tiles) and of r_k^2 (nT^2)
  double *ctl;                 // [kWassMaxRounds + 1][2]: entering round k, {the round the iteration stopped at or -1, r_k-1}
  double eta;
  int *status;

  __device__ const double *Y(int k) const { return k == 0 ? A : (k & 1) ? N : P; }
  __device__ const double *Z(int k) const { return (k & 1) ? Z1 : Z0; }
};

// the sum of the workgroup's 256 values in one fixed order, the same in every thread; all threads call it
__device__ __forceinline__ double wass_reduce(double s, double *sred) {
  const int tid = threadIdx.x;
  sred[tid] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if (tid < o) sred[tid] += sred[tid + o];
    __syncthreads();
  }
  const double r = sred[0];
  __syncthreads();
  return r;
}

__device__ __forceinline__ double wass_sum(const double *p, int n, double *sred) {
  double s = 0.0;
  for (int t = threadIdx.x; t < n; t += 256) s += p[t];
  return wass_reduce(s, sred);
}

// ---- prep ---------------------------------------------------------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_wass_prep(WassArgs<TI> a) {
  const int d = a.d, nT = a.nT, ldp = a.ldp, tid = threadIdx.x;
  const int i0 = ((int)blockIdx.x % nT) * kNgdTile, j0 = ((int)blockIdx.x / nT) * kNgdTile;
  for (int t = tid; t < kNgdTile * kNgdTile; t += 256) {
    const int i = i0 + (t & 63), j = j0 + (t >> 6);
    const bool in = i < d && j < d;
    const size_t o = (size_t)j * ldp + i;
    const double eye = i == j ? 1.0 : 0.0;
    a.N[o] = in ? eye + a.eta * (double)a.hess[(size_t)j * d + i] : 0.0;
    a.P[o] = in ? (double)a.state[(size_t)j * d + i] : 0.0;
    a.Z0[o] = in ? eye : 0.0;
    if (!in) a.W[o] = eye;
  }
  if (j0 == 0 && tid < kNgdTile && i0 + tid < d) a.params[i0 + tid] = (TI)((double)a.params[i0 + tid] + a.eta * (double)a.grad[i0 + tid]);
  if (blockIdx.x == 0 && tid == 0) {
    a.ctl[0] = -1.0;
    a.ctl[1] = INFINITY;
  }
}

// ---- mt: T = M Sigma, every tile ---------------------------------------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_wass_mt(WassArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  const int nT = a.nT, ldp = a.ldp;
  const int i0 = ((int)blockIdx.x % nT) * kNgdTile, j0 = ((int)blockIdx.x / nT) * kNgdTile;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, true, true>(acc, a.N + (size_t)i0 * ldp, ldp, a.P + (size_t)j0 * ldp, ldp, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) { a.T[(size_t)(j0 + jj) * ldp + i0 + ii] = x; });
}

// ---- sh, a: the upper tiles of T M' (Sh) | of Sh (Sh + 4 eta I) (A, with the tile's share of |A|_F^2), mirrored ------------------------------------------
template <typename TI, bool NORM>
__global__ __launch_bounds__(256) void k_wass_upper(WassArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  __shared__ double sred[256];
  const int d = a.d, ldp = a.ldp;
  int tc, tr;
  ngd_tile_of((int)blockIdx.x, tc, tr);   // tr <= tc: an upper tile
  const int i0 = tr * kNgdTile, j0 = tc * kNgdTile;
  const double *L = NORM ? a.Sh : a.T, *R = NORM ? a.Sh : a.N;
  double *out = NORM ? a.A : a.Sh;
  const double shift = NORM ? 4.0 * a.eta : 0.0;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, false, true>(
      acc, [=](int x, int k) { return L[(size_t)k * ldp + i0 + x]; },
      [=](int y, int k) { const int j = j0 + y; return R[(size_t)j * ldp + k] + ((NORM && k == j && j < d) ? shift : 0.0); }, 0, ldp, sAB,
      sAB + kNgdKC * kNgdLd);
  double s = 0.0;
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
    const int i = i0 + ii, j = j0 + jj;
    if (i > j) return;
    out[(size_t)j * ldp + i] = x;
    out[(size_t)i * ldp + j] = x;
    s += (i == j ? 1.0 : 2.0) * x * x;
  });
  if (NORM) {
    s = wass_reduce(s, sred);
    if (threadIdx.x == 0) a.part_a[blockIdx.x] = s;
  }
}

// 1 / c in round 0, where Y_0 = A (1/c) is read through its scale; 1 afterwards
template <typename TI>
__device__ __forceinline__ double wass_yscale(const WassArgs<TI> &a, double *sred) {
  return a.k == 0 ? 1.0 / sqrt(wass_sum(a.part_a, ngd_n_tiles(a.nT), sred)) : 1.0;
}

// ---- e(k): E_k = I - Z_k Y_k, every tile, and the tile's share of r_k^2 ------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_wass_e(WassArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  __shared__ double sred[256];
  if (a.ctl[2 * a.k] >= 0.0) return;   // stopped in an earlier round
  const int d = a.d, nT = a.nT, ldp = a.ldp;
  const int i0 = ((int)blockIdx.x % nT) * kNgdTile, j0 = ((int)blockIdx.x / nT) * kNgdTile;
  const double ys = wass_yscale(a, sred);
  const double *Y = a.Y(a.k), *Z = a.Z(a.k);
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, false, true>(
      acc, [=](int x, int k) { return Z[(size_t)k * ldp + i0 + x]; }, [=](int y, int k) { return Y[(size_t)(j0 + y) * ldp + k] * ys; }, 0, ldp, sAB,
      sAB + kNgdKC * kNgdLd);
  double s = 0.0;
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
    const int i = i0 + ii, j = j0 + jj;
    const double e = ((i == j && i < d) ? 1.0 : 0.0) - x;
    a.T[(size_t)j * ldp + i] = e;
    s += e * e;
  });
  s = wass_reduce(s, sred);
  if (threadIdx.x == 0) a.part_e[blockIdx.x] = s;
}

// ---- yz(k): the stop rule; Y_k+1 = Y_k + Y_k E_k / 2 (blocks < nT^2) | Z_k+1 = Z_k + E_k Z_k / 2 (the others) ---------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_wass_yz(WassArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  __shared__ double sred[256];
  const int nT = a.nT, ldp = a.ldp, k = a.k, n2 = nT * nT;
  const bool first = blockIdx.x == 0 && threadIdx.x == 0;
  double *next = a.ctl + 2 * (k + 1);
  const double stopped = a.ctl[2 * k], r_prev = a.ctl[2 * k + 1];
  if (stopped >= 0.0) {
    if (first) {
      next[0] = stopped;
      next[1] = r_prev;
    }
    return;
  }
  const double r = sqrt(wass_sum(a.part_e, n2, sred));
  const bool stop = !isfinite(r) || r <= 64.0 * (double)a.d * 2.220446049250313e-16 || (k >= 4 && (r >= r_prev || (r >= 0.5 * r_prev && r < 1e-6)));
  if (first) {
    next[0] = stop ? (double)k : -1.0;
    next[1] = r;
    if (!isfinite(r)) atomicOr(a.status, 1);
  }
  if (stop) return;
  const double ys = wass_yscale(a, sred);
  const bool isy = (int)blockIdx.x < n2;
  const int b = isy ? (int)blockIdx.x : (int)blockIdx.x - n2, i0 = (b % nT) * kNgdTile, j0 = (b / nT) * kNgdTile;
  const double *Y = a.Y(k), *Z = a.Z(k), *E = a.T;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  if (isy) {
    double *Yn = const_cast<double *>(a.Y(k + 1));
    ngd_product<double, false, true>(
        acc, [=](int x, int kk) { return Y[(size_t)kk * ldp + i0 + x] * ys; }, [=](int y, int kk) { return E[(size_t)(j0 + y) * ldp + kk]; }, 0, ldp, sAB,
        sAB + kNgdKC * kNgdLd);
    acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
      const size_t o = (size_t)(j0 + jj) * ldp + i0 + ii;
      Yn[o] = Y[o] * ys + 0.5 * x;
    });
  } else {
    double *Zn = const_cast<double *>(a.Z(k + 1));
    ngd_product<double, false, true>(acc, E + i0, ldp, Z + (size_t)j0 * ldp, ldp, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
    acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
      const size_t o = (size_t)(j0 + jj) * ldp + i0 + ii;
      Zn[o] = Z[o] + 0.5 * x;
    });
  }
}

// ---- sigma: the lower tiles of Sigma' = (Sh + 2 eta I + sqrt(c) (Y + Y')/2) / 2 --------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_wass_sigma(WassArgs<TI> a) {
  __shared__ double sred[256];
  const int d = a.d, ldp = a.ldp;
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  const double stopped = a.ctl[2 * kWassMaxRounds];
  if (stopped < 0.0 && blockIdx.x == 0 && threadIdx.x == 0) atomicOr(a.status, 1);   // the bound was reached without a stop
  const int kf = stopped >= 0.0 ? (int)stopped : kWassMaxRounds;
  const double c = sqrt(wass_sum(a.part_a, ngd_n_tiles(a.nT), sred));
  const double scale = sqrt(c) * (kf == 0 ? 1.0 / c : 1.0);
  const double *Y = a.Y(kf);
  for (int t = threadIdx.x; t < kNgdTile * kNgdTile; t += 256) {
    const int i = i0 + (t & 63), j = j0 + (t >> 6);
    if (i >= d || j >= d || i < j) continue;
    const double root = scale * (0.5 * (Y[(size_t)j * ldp + i] + Y[(size_t)i * ldp + j]));
    const double v = 0.5 * ((a.Sh[(size_t)j * ldp + i] + (i == j ? 2.0 * a.eta : 0.0)) + root);
    const TI vt = (TI)v;
    a.state[(size_t)j * d + i] = vt;
    a.state[(size_t)i * d + j] = vt;
    const int ri = d - 1 - i, rj = d - 1 - j;
    a.W[(size_t)rj * ldp + ri] = v;
    a.W[(size_t)ri * ldp + rj] = v;
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------
size_t wass_work_bytes(const mivi_ctx *c) {
  const NgdGeom g(c->cfg.d);
  return (8 * g.mat() + (size_t)g.nT * kNgdTile * kNgdTile) * sizeof(double);
}

size_t wass_part_bytes(const mivi_ctx *c) {
  const NgdGeom g(c->cfg.d);
  return (2 * (size_t)g.nT + (size_t)g.n_tiles + (size_t)g.nT * g.nT + 2 * (size_t)(kWassMaxRounds + 1)) * sizeof(double);
}

template <typename TI>
static void wass_update_t(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double eta, const void *logpi, void *entropy,
                          void *elbo) {
  const NgdGeom g(c->cfg.d);
  WassArgs<TI> a{};
  a.d = c->cfg.d;
  a.nT = g.nT;
  a.ldp = g.ldp;
  a.params = (TI *)params;
  a.state = (TI *)state;
  a.grad = (const TI *)grad;
  a.hess = (const TI *)hess;
  double *w = (double *)c->ms_work.p;
  a.N = w;
  a.P = w + g.mat();
  a.T = w + 2 * g.mat();
  a.Sh = w + 3 * g.mat();
  a.A = w + 4 * g.mat();
  a.Z0 = w + 5 * g.mat();
  a.Z1 = w + 6 * g.mat();
  a.W = w + 7 * g.mat();
  double *Dinv = w + 8 * g.mat();
  double *part = (double *)c->ms_part.p;   // [2][nT] of the factorisation first
  a.part_a = part + 2 * g.nT;
  a.part_e = a.part_a + g.n_tiles;
  a.ctl = a.part_e + (size_t)g.nT * g.nT;
  a.eta = (double)(TI)eta;   // convert(eltype(m), stepsize) (:88)
  a.status = (int *)c->status.p;
  const dim3 all(g.nT * g.nT), upper(g.n_tiles), wg(256);
  hipLaunchKernelGGL((k_wass_prep<TI>), all, wg, 0, c->stream, a);
  hipLaunchKernelGGL((k_wass_mt<TI>), all, wg, 0, c->stream, a);
  hipLaunchKernelGGL((k_wass_upper<TI, false>), upper, wg, 0, c->stream, a);
  hipLaunchKernelGGL((k_wass_upper<TI, true>), upper, wg, 0, c->stream, a);
  for (a.k = 0; a.k < kWassMaxRounds; ++a.k) {
    hipLaunchKernelGGL((k_wass_e<TI>), all, wg, 0, c->stream, a);
    hipLaunchKernelGGL((k_wass_yz<TI>), dim3(2 * g.nT * g.nT), wg, 0, c->stream, a);
  }
  hipLaunchKernelGGL((k_wass_sigma<TI>), upper, wg, 0, c->stream, a);
  launch_natgrad_factor(c, a.d, a.W, Dinv, part);
  launch_natgrad_factor_fin(c, a.W, part, params, logpi, entropy, elbo);
}

void launch_wass_update(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double eta, const void *logpi, void *entropy,
                        void *elbo) {
  by_dtype(c, [&](auto t) { wass_update_t<decltype(t)>(c, params, state, grad, hess, eta, logpi, entropy, elbo); });
}

}  // namespace mivi
