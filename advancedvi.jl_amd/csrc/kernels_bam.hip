// FisherMinBatchMatch ("batch and match", src/algorithms/fisherminbatchmatch.jl): the objective of rand_batch_match_samples_with_objective!
// (:81-111), the state of `init` (:76) and the update of `step` (:143-155) on the device-resident [m; vec C] and Sigma (d x d column-major,
// both triangles bitwise mirrored).  With u (d x B) the draws, z = C u + m, G the per-sample gradients, lambda = d B / iteration:
//     fisher = sum |u + C' G|^2 / B          elbo = mean logpi + entropy(q)                                                         (:108, :157)
//     U = lambda Gamma + lambda/(1+lambda) gbar gbar'      V = Sigma + lambda Cz + lambda/(1+lambda) (m - zbar)(m - zbar)'          (:150-151)
//     Sigma' = 2 V (I + sqrt(I + 4 U V))^-1      m' = m/(1+lambda) + lambda/(1+lambda) (Sigma' gbar + zbar)      C' = cholesky(Sigma').L
// The update is built in the low-rank form (rank exactly B), all of it in FLOAT64 for either context type (the subtraction below cancels
// about log10(lambda) digits):
//     alpha = sqrt(lambda/(B-1))   beta = sqrt(lambda/((1+lambda) B))   Q_b = alpha (g_b - gbar) + beta gbar   (U = Q Q')
//     Ut_b = alpha (u_b - ubar) + beta ubar      Zt = C Ut   (V = Sigma + Zt Zt';  z_b - zbar = C (u_b - ubar), zbar - m = C ubar)
//     M = Zt' Q     K = Q' Sigma Q + M' M = E diag(w) E' (w clamped at 0)     a = 1/2 + sqrt(w + 1/4)
//     Y = (Sigma Q + Zt M) E diag(1/a)           Sigma' = Sigma + Zt Zt' - Y Y'
// Launches of one update, nT = ceil(d / 64), any d >= 1 and 2 <= B <= MIVI_BAM_MAX_SAMPLES (there is no one-workgroup path: the eigenproblem
// is one workgroup's work at every size, and a small d only makes the tile grids one workgroup each):
//     prep    gbar, ubar, Q, Ut (padded to ldp x 64); the identity on the padding of the work matrix A
//     thin    Zt = C Ut and zbar = m + C ubar | SQ = Sigma Q                                    (2 nT workgroups, the tile product of ngd_tile.h)
//     eig     ONE workgroup: M, K in LDS, cyclic Jacobi (round-robin pairs, at most kBamMaxSweeps sweeps -- a compile-time bound; a matrix
//             that has not converged by then, or a non-finite eigenvalue, sets the sticky non-finite flag), E1 = E diag(1/a) and M E1
//     y       Y = SQ E1 + Zt (M E1)                                                                              (nT workgroups, K = 128)
//     sigma   the lower tiles of Sigma' = Sigma + [Zt Y][Zt -Y]', mirrored bitwise into the state and, with its rows and columns REVERSED, into A
//     mean    m' (ngd_row_matvec on A: Sigma' gbar is a product, not a solve, so there is nothing to refine)
//     factor  kernels_natgrad.hip's blocked factorisation A = Lr' Lr (2 nT - 1 launches).  It runs from the bottom-right corner, so on the
//             reversed matrix it IS the lower Cholesky factorisation: C'_pq = Lr_(d-1-q)(d-1-p).  A pivot that is not a positive finite number
//             sets MIVI_ERR_NONPOSITIVE_SCALE's flag and is replaced by 1 there.
//     fin     kernels_natgrad.hip's finish of a reversed factor: C' into the parameter vector (exact zeros above the diagonal); entropy(q')
//             and the flags (ngd_finish)
// 2 nT + 6 launches: 8 for d <= 64, 38 at d = 1024.  No floating-point atomics, one summation order: bitwise repeatable.  u and G are read-only.
// The moments: one launch of 64 x 64 tiles of C' G (float64, ngd_tile.h) whose epilogue adds u, squares and leaves one partial per tile, and
// a one-workgroup finish (fisher, logpi_avg, elbo = logpi_avg + entropy(q), the flags); init: the lower tiles of C C', mirrored.
#include "mivi_internal.h"
#include "ngd_tile.h"

namespace mivi {

constexpr int kBamB = MIVI_BAM_MAX_SAMPLES;   // the padded sample count: one tile
static_assert(kBamB == kNgdTile, "the thin matrices are one 64-column tile wide");
constexpr int kBamMaxSweeps = 30;             // cyclic Jacobi converges quadratically: 8 to 12 sweeps at n = 64
constexpr int kBamLdsDoubles = 3 * kNgdTile * kNgdLd;   // the staging pair (later E), M, K

template <typename TI>
struct BamArgs {
  int d, nT, ldp, B, n_eig;    // n_eig: B rounded up to an even number, the order of the Jacobi problem
  size_t ldu;                  // the leading dimension of u: d (the caller's buffer) or dP (the context's eps plane)
  TI *params;                  // [m (d); vec C (d x d, column-major)] in / out
  TI *state;                   // Sigma (d x d) in / out
  const TI *u, *G;             // d x B, column-major
  double *Q, *Ut, *Zt, *SQ, *Y;   // ldp x 64 each (element (i, b) at [b ldp + i]), zero beyond d and B
  double *A, *Dinv;            // ldp x ldp: Sigma' reversed, then its factor; nT tiles of 64 x 64
  double *M, *E1, *ME;         // 64 x 64 each: M (b1, b2) at [b2 64 + b1]; E1 and M E1 (b, c) at [c 64 + b]
  double *gbar, *ubar, *zbar;  // ldp each
  double *part;                // [2][nT] of the factorisation
  double lambda, alpha, beta;
  NgdOut<TI> out;
};

// ---- prep ---------------------------------------------------------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_prep(BamArgs<TI> a) {
  __shared__ double sg[kNgdTile], su[kNgdTile];
  const int d = a.d, ldp = a.ldp, B = a.B, tid = threadIdx.x, r = tid & 63, q = tid >> 6, i = (int)blockIdx.x * kNgdTile + r;
  if (q == 0) {
    double gs = 0.0, us = 0.0;
    if (i < d)
      for (int b = 0; b < B; ++b) {
        gs += (double)a.G[(size_t)b * d + i];
        us += (double)a.u[(size_t)b * a.ldu + i];
      }
    gs /= (double)B;
    us /= (double)B;
    sg[r] = gs;
    su[r] = us;
    a.gbar[i] = gs;
    a.ubar[i] = us;
  }
  __syncthreads();
  const double gb = sg[r], ub = su[r];
  for (int b = q; b < kBamB; b += 4) {
    const bool in = i < d && b < B;
    a.Q[(size_t)b * ldp + i] = in ? a.alpha * ((double)a.G[(size_t)b * d + i] - gb) + a.beta * gb : 0.0;
    a.Ut[(size_t)b * ldp + i] = in ? a.alpha * ((double)a.u[(size_t)b * a.ldu + i] - ub) + a.beta * ub : 0.0;
  }
  // the padding of A, tile column blockIdx.x: the identity (the factorisation then leaves diag(Lr, I))
  const int j0 = (int)blockIdx.x * kNgdTile;
  if (ldp > d)
    for (int t = tid; t < kNgdTile * ldp; t += 256) {
      const int j = j0 + t / ldp, ii = t % ldp;
      if (ii >= d || j >= d) a.A[(size_t)j * ldp + ii] = ii == j ? 1.0 : 0.0;
    }
}

// ---- thin: Zt = C Ut, zbar = m + C ubar (blocks < nT) | SQ = Sigma Q (the others) -----------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_thin(BamArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  __shared__ double sred[4 * kNgdTile];
  const int d = a.d, nT = a.nT, ldp = a.ldp;
  const bool zt = (int)blockIdx.x < nT;
  const int bi = zt ? (int)blockIdx.x : (int)blockIdx.x - nT, i0 = bi * kNgdTile;
  const TI *C = a.params + d, *S = a.state;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  if (zt) {
    const double *Ut = a.Ut;
    ngd_product<double, false, true>(
        acc, [=](int x, int k) { const int i = i0 + x; return (i < d && k <= i) ? (double)C[(size_t)k * d + i] : 0.0; },
        [=](int y, int k) { return Ut[(size_t)y * ldp + k]; }, 0, i0 + kNgdTile, sAB, sAB + kNgdKC * kNgdLd);
    acc.each(wr, wc, lane, [&](int ii, int jj, double x) { a.Zt[(size_t)jj * ldp + i0 + ii] = x; });
    const double *ubar = a.ubar;
    ngd_row_matvec(
        bi, d, false, sred, [=](int i, int j) { return (double)C[(size_t)j * d + i] * ubar[j]; },
        [&](int i, double tot) { a.zbar[i] = (double)a.params[i] + tot; });
  } else {
    const double *Q = a.Q;
    ngd_product<double, false, true>(
        acc, [=](int x, int k) { const int i = i0 + x; return (i < d && k < d) ? (double)S[(size_t)k * d + i] : 0.0; },
        [=](int y, int k) { return Q[(size_t)y * ldp + k]; }, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
    acc.each(wr, wc, lane, [&](int ii, int jj, double x) { a.SQ[(size_t)jj * ldp + i0 + ii] = x; });
  }
}

// ---- eig: the B x B symmetric eigenproblem, one workgroup --------------------------------------------------------------------------------------------
// Cyclic Jacobi on the n x n matrix K in LDS (row-major, kNgdLd; n even), E <- the rotations' product.  A round rotates n / 2 disjoint pairs
// (the round-robin tournament), n - 1 rounds a sweep, rotations applied by Rutishauser's formulas; a pair is skipped when |K_pq| <= 2^-53 sqrt|K_pp K_qq| or <= 1e-25 |K|_F.  Returns 1
// when a whole sweep rotated nothing, 0 after kBamMaxSweeps sweeps (NaNs rotate for ever: they end here).  256 threads, all call it.
__device__ __forceinline__ int bam_jacobi(double *K, double *E, int n, double floor_abs, double *sc, double *ss, int *sp, int *sq, int *srot) {
  const int tid = threadIdx.x, half = n >> 1, m1 = n - 1;
  double *sdp = sc + kBamB / 2, *sdq = ss + kBamB / 2;   // (the second halves of sc / ss: the rotated pair's new diagonal entries)
  for (int sweep = 0; sweep < kBamMaxSweeps; ++sweep) {
    if (tid == 0) *srot = 0;
    __syncthreads();
    for (int r = 0; r < m1; ++r) {
      if (tid < half) {
        int p = tid == 0 ? m1 : (r + tid) % m1, q = tid == 0 ? r : (r - tid + m1) % m1;
        if (p > q) { const int t = p; p = q; q = t; }
        const double app = K[p * kNgdLd + p], aqq = K[q * kNgdLd + q], apq = K[p * kNgdLd + q];
        double s = 0.0, tau = 0.0, dp = app, dq = aqq;
        if (!(fabs(apq) <= 1.1102230246251565e-16 * sqrt(fabs(app * aqq)) || fabs(apq) <= floor_abs)) {
          const double th = (aqq - app) / (2.0 * apq);
          const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(1.0 + th * th));
          const double c = 1.0 / sqrt(1.0 + t * t);
          s = t * c;
          tau = s / (1.0 + c);
          dp = app - t * apq;   // (Rutishauser's update formulas: a small rotation changes an entry by a small correction, not by a
          dq = aqq + t * apq;   //  rounded product with c close to 1)
          *srot = 1;            // (an int in LDS, the same value from every writer)
        }
        sc[tid] = tau;
        ss[tid] = s;
        sdp[tid] = dp;
        sdq[tid] = dq;
        sp[tid] = p;
        sq[tid] = q;
      }
      __syncthreads();
      for (int t = tid; t < half * n; t += 256) {   // columns p, q of K and of E
        const int pr = t / n, row = t % n, p = sp[pr], q = sq[pr];
        const double tau = sc[pr], s = ss[pr];
        if (s != 0.0) {
          const double kp = K[row * kNgdLd + p], kq = K[row * kNgdLd + q], ep = E[row * kNgdLd + p], eq = E[row * kNgdLd + q];
          K[row * kNgdLd + p] = kp - s * (kq + tau * kp);
          K[row * kNgdLd + q] = kq + s * (kp - tau * kq);
          E[row * kNgdLd + p] = ep - s * (eq + tau * ep);
          E[row * kNgdLd + q] = eq + s * (ep - tau * eq);
        }
      }
      __syncthreads();
      for (int t = tid; t < half * n; t += 256) {   // rows p, q of K
        const int pr = t / n, col = t % n, p = sp[pr], q = sq[pr];
        const double tau = sc[pr], s = ss[pr];
        if (s != 0.0) {
          const double kp = K[p * kNgdLd + col], kq = K[q * kNgdLd + col];
          K[p * kNgdLd + col] = kp - s * (kq + tau * kp);
          K[q * kNgdLd + col] = kq + s * (kp - tau * kq);
        }
      }
      __syncthreads();
      if (tid < half && ss[tid] != 0.0) {   // the rotated pair: its off-diagonal element is zero by construction, its diagonal by the formulas
        const int p = sp[tid], q = sq[tid];
        K[p * kNgdLd + q] = 0.0;
        K[q * kNgdLd + p] = 0.0;
        K[p * kNgdLd + p] = sdp[tid];
        K[q * kNgdLd + q] = sdq[tid];
      }
      __syncthreads();
    }
    const int rot = *srot;
    __syncthreads();
    if (!rot) return 1;
  }
  return 0;
}

template <typename TI>
__global__ __launch_bounds__(256) void k_bam_eig(BamArgs<TI> a) {
  extern __shared__ double bam_lds[];
  double *sAB = bam_lds, *sM = bam_lds + kNgdTile * kNgdLd, *sK = bam_lds + 2 * kNgdTile * kNgdLd;   // (2 kNgdKC = kNgdTile: the staging pair is one matrix)
  __shared__ double sc[kBamB], ss[kBamB], sw[kBamB], sred[256];   // (sc / ss: tau, s | the new diagonal entries)
  __shared__ int sp[kBamB / 2], sq[kBamB / 2], srot;
  const int ldp = a.ldp, n = a.n_eig, tid = threadIdx.x;
  NGD_WAVE;
  {   // M = Zt' Q
    NgdFrag<double> acc;
    acc.zero();
    ngd_product<double, true, true>(acc, a.Zt, ldp, a.Q, ldp, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
    acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
      sM[ii * kNgdLd + jj] = x;
      a.M[jj * kBamB + ii] = x;
    });
  }
  __syncthreads();
  {   // K = Q' (Sigma Q) + M' M
    NgdFrag<double> acc;
    acc.zero();
    ngd_product<double, true, true>(acc, a.Q, ldp, a.SQ, ldp, 0, ldp, sAB, sAB + kNgdKC * kNgdLd);
    acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
      double s = 0.0;
      for (int k = 0; k < kBamB; ++k) s += sM[k * kNgdLd + ii] * sM[k * kNgdLd + jj];
      sK[ii * kNgdLd + jj] = x + s;
    });
  }
  __syncthreads();
  double *sE = sAB;
  double fro = 0.0;
  for (int t = tid; t < kBamB * kBamB; t += 256) {   // the lower triangle, mirrored; E = I
    const int i = t >> 6, j = t & 63;
    if (i > j) continue;
    const double v = sK[j * kNgdLd + i];   // (j >= i: the lower triangle's element)
    fro += (i == j ? 1.0 : 2.0) * v * v;
  }
  sred[tid] = fro;
  __syncthreads();
  for (int t = tid; t < kBamB * kBamB; t += 256) {
    const int i = t >> 6, j = t & 63;
    if (i < j) sK[i * kNgdLd + j] = sK[j * kNgdLd + i];
    sE[i * kNgdLd + j] = i == j ? 1.0 : 0.0;
  }
  if (tid == 0) {
    double s = 0.0;
    for (int t = 0; t < 256; ++t) s += sred[t];
    sred[0] = sqrt(s);
  }
  __syncthreads();
  const double floor_abs = 1e-25 * sred[0];
  __syncthreads();
  const int conv = bam_jacobi(sK, sE, n, floor_abs, sc, ss, sp, sq, &srot);
  if (tid < kBamB) {
    const double w = sK[tid * kNgdLd + tid];
    sw[tid] = 1.0 / (0.5 + sqrt((w > 0.0 ? w : 0.0) + 0.25));   // 1 / a
    if (!isfinite(w) || (tid == 0 && !conv)) atomicOr(a.out.status, 1);
  }
  __syncthreads();
  for (int t = tid; t < kBamB * kBamB; t += 256) {   // E1 = E diag(1/a); M E1
    const int b = t & 63, c = t >> 6;
    a.E1[t] = sE[b * kNgdLd + c] * sw[c];
    double s = 0.0;
    for (int k = 0; k < kBamB; ++k) s += sM[b * kNgdLd + k] * sE[k * kNgdLd + c];
    a.ME[t] = s * sw[c];
  }
}

// ---- y: Y = SQ E1 + Zt (M E1) ------------------------------------------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_y(BamArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  const int ldp = a.ldp, i0 = (int)blockIdx.x * kNgdTile;
  const double *SQ = a.SQ, *Zt = a.Zt, *E1 = a.E1, *ME = a.ME;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, false, true>(
      acc, [=](int x, int k) { return k < kBamB ? SQ[(size_t)k * ldp + i0 + x] : Zt[(size_t)(k - kBamB) * ldp + i0 + x]; },
      [=](int y, int k) { return k < kBamB ? E1[y * kBamB + k] : ME[y * kBamB + k - kBamB]; }, 0, 2 * kBamB, sAB, sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) { a.Y[(size_t)jj * ldp + i0 + ii] = x; });
}

// ---- sigma: the lower tiles of Sigma' = Sigma + Zt Zt' - Y Y' ---------------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_sigma(BamArgs<TI> a) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  const int d = a.d, ldp = a.ldp;
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  const double *Zt = a.Zt, *Y = a.Y;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, false, false>(
      acc, [=](int x, int k) { return k < kBamB ? Zt[(size_t)k * ldp + i0 + x] : Y[(size_t)(k - kBamB) * ldp + i0 + x]; },
      [=](int y, int k) { return k < kBamB ? Zt[(size_t)k * ldp + j0 + y] : -Y[(size_t)(k - kBamB) * ldp + j0 + y]; }, 0, 2 * kBamB, sAB,
      sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
    const int i = i0 + ii, j = j0 + jj;
    if (i >= d || j >= d || i < j) return;
    const double v = (double)a.state[(size_t)j * d + i] + x;   // (the lower triangle's element: nobody else reads or writes it)
    const TI vt = (TI)v;
    a.state[(size_t)j * d + i] = vt;
    a.state[(size_t)i * d + j] = vt;
    const int ri = d - 1 - i, rj = d - 1 - j;
    a.A[(size_t)rj * ldp + ri] = v;
    a.A[(size_t)ri * ldp + rj] = v;
  });
}

// ---- mean: m' = m/(1+lambda) + lambda/(1+lambda) (Sigma' gbar + zbar) ----------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_mean(BamArgs<TI> a) {
  __shared__ double sred[4 * kNgdTile];
  const int d = a.d, ldp = a.ldp;
  const double *A = a.A, *gbar = a.gbar;
  const double w = a.lambda / (1.0 + a.lambda);
  ngd_row_matvec(
      (int)blockIdx.x, d, true, sred, [=](int i, int j) { return A[(size_t)(d - 1 - j) * ldp + (d - 1 - i)] * gbar[j]; },
      [&](int i, double tot) { a.params[i] = (TI)((double)a.params[i] / (1.0 + a.lambda) + w * (tot + a.zbar[i])); });
}

// ---- init: Sigma = C C', the lower tiles, mirrored -------------------------------------------------------------------------------------------------------------
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_init(int d, const TI *C, TI *Sigma) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  int ti, tj;
  ngd_tile_of((int)blockIdx.x, ti, tj);
  const int i0 = ti * kNgdTile, j0 = tj * kNgdTile;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, false, false>(
      acc, [=](int x, int k) { const int i = i0 + x; return (i < d && k <= i) ? (double)C[(size_t)k * d + i] : 0.0; },
      [=](int y, int k) { const int j = j0 + y; return (j < d && k <= j) ? (double)C[(size_t)k * d + j] : 0.0; }, 0, j0 + kNgdTile, sAB,
      sAB + kNgdKC * kNgdLd);
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
    const int i = i0 + ii, j = j0 + jj;
    if (i >= d || j >= d || i < j) return;
    Sigma[(size_t)j * d + i] = (TI)x;
    Sigma[(size_t)i * d + j] = (TI)x;
  });
}

// ---- the objective -----------------------------------------------------------------------------------------------------------------------------------------------
// tile (rows j0 of C' G, samples b0): part[blockIdx] = sum over the tile of (u_jb + sum_{k >= j} C_kj G_kb)^2, one order
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_fisher(int d, int nT, int M, const TI *C, const TI *u, size_t ldu, const TI *G, double *part) {
  __shared__ double sAB[2 * kNgdKC * kNgdLd];
  __shared__ double sred[256];
  const int j0 = ((int)blockIdx.x % nT) * kNgdTile, b0 = ((int)blockIdx.x / nT) * kNgdTile;
  NGD_WAVE;
  NgdFrag<double> acc;
  acc.zero();
  ngd_product<double, true, true>(
      acc, [=](int x, int k) { const int j = j0 + x; return (j < d && k < d && k >= j) ? (double)C[(size_t)j * d + k] : 0.0; },
      [=](int y, int k) { const int b = b0 + y; return (b < M && k < d) ? (double)G[(size_t)b * d + k] : 0.0; }, j0, nT * kNgdTile, sAB,
      sAB + kNgdKC * kNgdLd);
  double s = 0.0;
  acc.each(wr, wc, lane, [&](int ii, int jj, double x) {
    const int j = j0 + ii, b = b0 + jj;
    if (j < d && b < M) {
      const double v = (double)u[(size_t)b * ldu + j] + x;
      s += v * v;
    }
  });
  sred[threadIdx.x] = s;
  __syncthreads();
  for (int o = 128; o > 0; o >>= 1) {
    if ((int)threadIdx.x < o) sred[threadIdx.x] += sred[threadIdx.x + o];
    __syncthreads();
  }
  if (threadIdx.x == 0) part[blockIdx.x] = sred[0];
}

// fisher = (sum of the n_part tile partials, in order) / n; logpi_avg = ell_sum / n; elbo = logpi_avg + entropy(q).  One workgroup.
template <typename TI>
__global__ __launch_bounds__(256) void k_bam_objective(int d, const TI *params, const double *part, int n_part, double n, const TI *ell_sum, TI *fisher,
                                                       TI *logpi_avg, TI *elbo, int *status) {
  __shared__ double sf[256], sl[256];
  __shared__ int sbad[256];
  const int tid = threadIdx.x;
  double f = 0.0, l = 0.0;
  int bad = 0;
  for (int t = tid; t < n_part; t += 256) f += part[t];
  if (elbo)
    for (int i = tid; i < d; i += 256) {
      const double cii = (double)params[d + (size_t)i * d + i];
      bad |= ngd_bad(cii) ? 1 : 0;
      l += log(cii);
    }
  sf[tid] = f;
  sl[tid] = l;
  sbad[tid] = bad;
  __syncthreads();
  if (tid == 0) {
    f = 0.0;
    l = 0.0;
    bad = 0;
    for (int t = 0; t < 256; ++t) {
      f += sf[t];
      l += sl[t];
      bad |= sbad[t];
    }
    const TI fv = (TI)(f / n);
    if (fisher) *fisher = fv;
    if (!isfinite((double)fv)) atomicOr(status, 1);
    if (logpi_avg) *logpi_avg = (TI)((double)ell_sum[0] / n);
    if (elbo) ngd_finish(d, l, bad, NgdOut<TI>{logpi_avg, nullptr, elbo, status});
  }
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------------------------------
size_t bam_work_bytes(const mivi_ctx *c) {
  const NgdGeom g(c->cfg.d);
  return (g.mat() + (size_t)g.nT * kNgdTile * kNgdTile + 5 * (size_t)g.ldp * kBamB + 3 * (size_t)kBamB * kBamB + 3 * (size_t)g.ldp) * sizeof(double);
}

size_t bam_part_bytes(const mivi_ctx *c) { return 2 * (size_t)NgdGeom(c->cfg.d).nT * sizeof(double); }

int bam_fisher_tiles(const mivi_ctx *c, int M) { return NgdGeom(c->cfg.d).nT * ((M + kNgdTile - 1) / kNgdTile); }

template <typename TI>
static void bam_update_t(mivi_ctx *c, void *params, void *state, const void *u, size_t ldu, const void *G, int B, double lambda, void *entropy) {
  const NgdGeom g(c->cfg.d);
  BamArgs<TI> a{};
  a.d = c->cfg.d;
  a.nT = g.nT;
  a.ldp = g.ldp;
  a.B = B;
  a.n_eig = (B + 1) & ~1;
  a.ldu = ldu;
  a.params = (TI *)params;
  a.state = (TI *)state;
  a.u = (const TI *)u;
  a.G = (const TI *)G;
  double *w = (double *)c->ms_work.p;
  const size_t thin = (size_t)g.ldp * kBamB, sq = (size_t)kBamB * kBamB;
  a.A = w;
  a.Dinv = a.A + g.mat();
  a.Q = a.Dinv + (size_t)g.nT * kNgdTile * kNgdTile;
  a.Ut = a.Q + thin;
  a.Zt = a.Ut + thin;
  a.SQ = a.Zt + thin;
  a.Y = a.SQ + thin;
  a.M = a.Y + thin;
  a.E1 = a.M + sq;
  a.ME = a.E1 + sq;
  a.gbar = a.ME + sq;
  a.ubar = a.gbar + g.ldp;
  a.zbar = a.ubar + g.ldp;
  a.part = (double *)c->ms_part.p;
  a.lambda = lambda;
  a.alpha = sqrt(lambda / (double)(B - 1));
  a.beta = sqrt(lambda / ((1.0 + lambda) * (double)B));
  a.out = NgdOut<TI>{nullptr, (TI *)entropy, nullptr, (int *)c->status.p};
  const size_t lds = (size_t)kBamLdsDoubles * sizeof(double);
  static bool lds_set[64] = {};   // (per instantiation and device: once, not a host call in every step of mivi_bam_steps)
  const int dev = c->cfg.device;
  if (dev < 0 || dev >= 64 || !lds_set[dev]) {
    (void)hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bam_eig<TI>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (dev >= 0 && dev < 64) lds_set[dev] = true;
  }
  hipLaunchKernelGGL((k_bam_prep<TI>), dim3(g.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_bam_thin<TI>), dim3(2 * g.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_bam_eig<TI>), dim3(1), dim3(256), lds, c->stream, a);
  hipLaunchKernelGGL((k_bam_y<TI>), dim3(g.nT), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_bam_sigma<TI>), dim3(g.n_tiles), dim3(256), 0, c->stream, a);
  hipLaunchKernelGGL((k_bam_mean<TI>), dim3(g.nT), dim3(256), 0, c->stream, a);
  launch_natgrad_factor(c, a.d, a.A, a.Dinv, a.part);
  launch_natgrad_factor_fin(c, a.A, a.part, params, nullptr, entropy, nullptr);
}

void launch_bam_update(mivi_ctx *c, void *params, void *state, const void *u, size_t ldu, const void *G, int B, double lambda, void *entropy) {
  by_dtype(c, [&](auto t) { bam_update_t<decltype(t)>(c, params, state, u, ldu, G, B, lambda, entropy); });
}

void launch_bam_init(mivi_ctx *c, const void *params, void *state) {
  const int d = c->cfg.d;
  const NgdGeom g(d);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_bam_init<T>), dim3(g.n_tiles), dim3(256), 0, c->stream, d, (const T *)params + d, (T *)state);
  });
}

void launch_bam_fisher(mivi_ctx *c, const void *params, int M, const void *u, size_t ldu, const void *G, double *part) {
  const int d = c->cfg.d;
  const NgdGeom g(d);
  const dim3 grid(bam_fisher_tiles(c, M));
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_bam_fisher<T>), grid, dim3(256), 0, c->stream, d, g.nT, M, (const T *)params + d, (const T *)u, ldu, (const T *)G, part);
  });
}

void launch_bam_objective(mivi_ctx *c, const void *params, const double *part, int n_part, double n, const void *ell_sum, void *fisher, void *logpi_avg,
                          void *elbo) {
  int *st = (int *)c->status.p;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL((k_bam_objective<T>), dim3(1), dim3(256), 0, c->stream, c->cfg.d, (const T *)params, part, n_part, n, (const T *)ell_sum, (T *)fisher,
                       (T *)logpi_avg, (T *)elbo, st);
  });
}

}  // namespace mivi
