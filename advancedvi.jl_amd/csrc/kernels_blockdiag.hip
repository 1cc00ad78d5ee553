// The block-diagonal Gaussian family (MIVI_BLOCKDIAG; include/mivi.h holds the definition): the kernels of one RepGradELBO estimate, of
// rand and of logpdf (k_bd_logpdf, below the estimate).  api_blockdiag.hip and api_logpdf.hip drive them.
//
// The scale is nb = ceil(d / b) independent lower-triangular blocks, so there is no d x d operand and nothing crosses a block but the
// per-sample scalars of the value.  The work is cut into UNITS: one block for b > 8, a run of g = 16 / b consecutive blocks for b <= 8 (their
// rows fill one 16-row matrix-core tile; the unit's scale is itself block-diagonal inside it).  One workgroup is ONE wave and owns one unit x
// one slice of the 16-sample tiles (tile s, s + n_slices, ...):
//   * the unit's scale is staged once in LDS as [R16][R16] (R16 = the unit's rows rounded up to 16) with zeros above the diagonal and
//     between the blocks of a run, so every product below is whole 16 x 16 x 4 steps (Mfma16, device_common.h) without per-element masks;
//   * the eps tile is drawn in the kernel (the mean-field Philox stream: counter = global coordinate quad, sample column, estimate) into LDS;
//   * Z = mu + C E skips the k-groups that lie wholly above the diagonal;
//   * sticking the landing: U = C^-T E by back substitution in LDS (lane = sample column x a quarter of the row sum, the scale's column
//     read as a broadcast).  It is RECOMPUTED from the redrawn tile where the gradient is formed: no U plane is stored;
//   * dC = -(1/M) tril(W E') with the samples as the K axis, the accumulators held in registers across the workgroup's tiles; dmu = -(1/M) W 1
//     and every per-sample scalar in f64, in a fixed order.
// k_bd<T, NT, MODE>: NT = R16 / 16;  MODE 0 forward (Z, the draws, the value's partials), 1 VJP (W = grad log pi from the target's output,
// the tile redrawn), 2 fused: forward, the diagonal-Gaussian target and the VJP in one pass (W is elementwise in z: only the gradient and the
// value's partials leave the workgroup).  With more than one slice the gradients are f64 partials per slice, summed slice after slice by
// k_bd_finish: no atomics, bitwise reproducible.
#include "device_common.h"

namespace mivi {

BdShape bd_shape(int d, int b) {
  BdShape s;
  s.d = d;
  s.b = b;
  s.g = b <= 8 ? 16 / b : 1;
  s.R = s.g * b;
  s.n_units = (d + s.R - 1) / s.R;
  s.ns_max = s.n_units >= 1024 ? 1 : (1024 / s.n_units < 64 ? 1024 / s.n_units : 64);
  const long long nb = (d + b - 1) / b, bl = d - (nb - 1) * b;
  s.plen = d + (nb - 1) * (long long)b * b + bl * bl;
  return s;
}
int bd_slices(const BdShape &s, int M) {
  const long long tiles = (M + 15) / 16, by_mem = (1ll << 25) / s.plen;   // the partials stay under 256 MB
  long long ns = tiles < s.ns_max ? tiles : s.ns_max;
  if (ns > by_mem) ns = by_mem;
  return ns < 1 ? 1 : (int)ns;
}

template <typename T>
struct BdArgs {
  BdShape s;
  int M, n_slices;
  const T *params;
  RngArgs rng;
  T *Z, *eps;                 // d x M outputs, ld = d (or nullptr)
  const T *W;                 // MODE 1: grad log pi, d x M (ld = d)
  const T *t_mean, *t_istd;   // MODE 2: the diagonal-Gaussian target
  double *he_part, *ell_part; // [n_units][n_slices]: sum 0.5 eps^2, sum ell (MODE 2)
  double *ld_part;            // [2][n_units]: sum log C_ii, count of non-positive C_ii (slice 0 writes them); nullptr: rand
  double *part;               // [n_slices][plen] f64 gradient partials, or nullptr: one slice, the gradient goes to `grad`
  T *grad;
  int stl;                    // W += C^-T eps
  double direct, invM;        // the coefficient of -1 / C_ii (direct_entropy_coeff), 1 / M_total
};

extern __shared__ double bd_lds[];

template <int NT>
constexpr int bd_lds_elems() { return NT * 16 * (NT * 16 + 1) + 3 * NT * 16 * 16 + NT * 16; }

template <typename T, int NT, int MODE>
__global__ __launch_bounds__(64) void k_bd(BdArgs<T> a) {
  constexpr int R16 = NT * 16, LDC = R16 + 1;
  using acc_t = typename Mfma16<T>::acc_t;
  T *Cs = (T *)bd_lds, *Et = Cs + R16 * LDC, *Wt = Et + R16 * 16, *Ut = Wt + R16 * 16, *Mu = Ut + R16 * 16;
  const int d = a.s.d, b = a.s.b, g = a.s.g;
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  const int u = blockIdx.x, sl = blockIdx.y;
  const int r0 = u * a.s.R, Ru = d - r0 < a.s.R ? d - r0 : a.s.R;
  const T *Cp = a.params + d;
  // ---- the unit's scale, once: zeros above the diagonal, between the blocks of a run and past the unit's rows ----
  for (int e = lane; e < R16 * R16; e += 64) {
    const int j = e / R16, i = e - j * R16;
    T v = T(0);
    if (i < Ru && j <= i && i / b == j / b) {
      const int q = i / b, kb = u * g + q, bk = d - kb * b < b ? d - kb * b : b;
      v = Cp[(size_t)kb * b * b + (size_t)(j - q * b) * bk + (i - q * b)];
    }
    Cs[i * LDC + j] = v;
  }
  for (int e = lane; e < R16 * 16; e += 64) Et[e] = Wt[e] = Ut[e] = T(0);
  if (lane < R16) Mu[lane] = lane < Ru ? a.params[r0 + lane] : T(0);
  __syncthreads();
  if (MODE != 1 && a.ld_part && sl == 0) {
    double lg = 0.0, bad = 0.0;
    if (lane < Ru) {
      const double c = (double)Cs[lane * LDC + lane];
      lg = log(c);
      bad = c > 0.0 ? 0.0 : 1.0;
    }
    lg = wave_sum(lg);
    bad = wave_sum(bad);
    if (lane == 0) {
      a.ld_part[u] = lg;
      a.ld_part[gridDim.x + u] = bad;
    }
  }
  acc_t accC[NT * (NT + 1) / 2];
#pragma unroll
  for (int t = 0; t < NT * (NT + 1) / 2; ++t) accC[t] = acc_t{0, 0, 0, 0};
  double accMu = 0.0, he = 0.0, ell = 0.0;
  const int tiles = (a.M + 15) / 16, d4 = (d + 3) >> 2;
  const int q0 = r0 >> 2, nq = ((r0 + Ru - 1) >> 2) - q0 + 1;
  const uint64_t idx = rng_index(a.rng);
  for (int tile = sl; tile < tiles; tile += a.n_slices) {
    const int m0 = tile * 16, n_ok = a.M - m0 < 16 ? a.M - m0 : 16;
    // ---- the draws of the unit's rows: the coordinate quads that cover them ----
    for (int e = lane; e < 16 * nq; e += 64) {
      const int m = e / nq, rq = q0 + (e - m * nq);
      T ev[4] = {T(0), T(0), T(0), T(0)};
      if (m < n_ok) eps_block<T>(a.rng.seed, idx, (uint64_t)(a.rng.m_offset + m0 + m) * (uint64_t)d4 + (uint64_t)rq, ev);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 4 * rq + r - r0;
        if (row >= 0 && row < Ru) Et[row * 16 + m] = ev[r];
      }
    }
    __syncthreads();
    if (MODE == 0 && a.eps)
      for (int e = lane; e < 16 * Ru; e += 64) {
        const int m = e / Ru, row = e - m * Ru;
        if (m < n_ok) a.eps[(size_t)(m0 + m) * d + r0 + row] = Et[row * 16 + m];
      }
    if (MODE != 1 && lane < 16) {
      double h = 0.0;
      for (int i = 0; i < Ru; ++i) h += (double)Et[i * 16 + lane] * (double)Et[i * 16 + lane];
      he += 0.5 * h;
    }
    if (MODE != 1) {   // Z = mu + C E: row group ti needs the k-groups up to its own
      static_for<0, NT>([&](auto ti_) {
        constexpr int ti = decltype(ti_)::value;
        acc_t acc = {0, 0, 0, 0};
        for (int k0 = 0; k0 < (ti + 1) * 16; k0 += 4) acc = Mfma16<T>::mma(Cs[(ti * 16 + col) * LDC + k0 + kq], Et[(k0 + kq) * 16 + col], acc);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = ti * 16 + Mfma16<T>::row(kq, r);
          Wt[row * 16 + col] = acc[r] + Mu[row];
        }
      });
      __syncthreads();
    }
    if (MODE == 0) {
      if (a.Z)
        for (int e = lane; e < 16 * Ru; e += 64) {
          const int m = e / Ru, row = e - m * Ru;
          if (m < n_ok) a.Z[(size_t)(m0 + m) * d + r0 + row] = Wt[row * 16 + m];
        }
      __syncthreads();
      continue;
    }
    if (MODE == 2) {   // the diagonal-Gaussian target in place: t = (z - mean) / std, ell -= t^2 / 2, w = -t / std
      for (int e = lane; e < 16 * Ru; e += 64) {
        const int m = e / Ru, row = e - m * Ru;
        Wt[row * 16 + m] = (Wt[row * 16 + m] - a.t_mean[r0 + row]) * a.t_istd[r0 + row];
      }
      __syncthreads();
      if (lane < n_ok) {
        double s = 0.0;
        for (int i = 0; i < Ru; ++i) s += (double)Wt[i * 16 + lane] * (double)Wt[i * 16 + lane];
        ell -= 0.5 * s;
      }
      __syncthreads();
      for (int e = lane; e < 16 * Ru; e += 64) {
        const int m = e / Ru, row = e - m * Ru;
        Wt[row * 16 + m] = m < n_ok ? -Wt[row * 16 + m] * a.t_istd[r0 + row] : T(0);
      }
    } else {
      for (int e = lane; e < 16 * Ru; e += 64) {
        const int m = e / Ru, row = e - m * Ru;
        Wt[row * 16 + m] = m < n_ok ? a.W[(size_t)(m0 + m) * d + r0 + row] : T(0);
      }
    }
    __syncthreads();
    if (a.stl) {   // C' U = E from the last row up; rows of another block of the run contribute zeros and are skipped
      for (int i = Ru - 1; i >= 0; --i) {
        const int jend = (i / b + 1) * b < Ru ? (i / b + 1) * b : Ru;
        T s = T(0);
        for (int j = i + 1 + kq; j < jend; j += 4) s += Cs[j * LDC + i] * Ut[j * 16 + col];
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (kq == 0) Ut[i * 16 + col] = (Et[i * 16 + col] - s) / Cs[i * LDC + i];
        __syncthreads();
      }
      for (int e = lane; e < 16 * Ru; e += 64) Wt[e] += Ut[e];   // (columns past n_ok: E = 0, so U = 0)
      __syncthreads();
    }
    // ---- dC += W E' over the tile's 16 samples, the lower tile pairs only; dmu += W 1 ----
    static_for<0, NT>([&](auto ti_) {
      constexpr int ti = decltype(ti_)::value;
      static_for<0, ti + 1>([&](auto tj_) {
        constexpr int tj = decltype(tj_)::value;
        acc_t &acc = accC[ti * (ti + 1) / 2 + tj];
#pragma unroll
        for (int k0 = 0; k0 < 16; k0 += 4) acc = Mfma16<T>::mma(Wt[(ti * 16 + col) * 16 + k0 + kq], Et[(tj * 16 + col) * 16 + k0 + kq], acc);
      });
    });
    if (lane < Ru) {
      double s = 0.0;
      for (int m = 0; m < 16; ++m) s += (double)Wt[lane * 16 + m];
      accMu += s;
    }
    __syncthreads();
  }
  if (MODE != 1 && a.he_part) {
    he = wave_sum(he);
    if (lane == 0) a.he_part[(size_t)u * a.n_slices + sl] = he;
  }
  if (MODE == 0) return;
  if (MODE == 2) {
    ell = wave_sum(ell);
    if (lane == 0) a.ell_part[(size_t)u * a.n_slices + sl] = ell;
  }
  // ---- the unit's gradient entries: every entry of its blocks is written (exact zeros above a block's diagonal) ----
  double *part = a.part ? a.part + (size_t)sl * a.s.plen : nullptr;
  auto put = [&](size_t off, double v) {
    if (part) part[off] = v;
    else a.grad[off] = (T)v;
  };
  if (lane < Ru) put((size_t)r0 + lane, -accMu * a.invM);
  static_for<0, NT>([&](auto ti_) {
    constexpr int ti = decltype(ti_)::value;
    static_for<0, NT>([&](auto tj_) {
      constexpr int tj = decltype(tj_)::value;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = ti * 16 + Mfma16<T>::row(kq, r), cj = tj * 16 + col;
        if (row >= Ru || cj >= Ru || row / b != cj / b) continue;
        const int q = row / b, kb = u * g + q, bk = d - kb * b < b ? d - kb * b : b, li = row - q * b, lj = cj - q * b;
        double v = 0.0;
        if constexpr (ti >= tj) {
          if (li >= lj) v = -(double)accC[ti * (ti + 1) / 2 + tj][r] * a.invM;
        }
        if (li == lj && sl == 0) v -= a.direct / (double)Cs[row * LDC + row];
        put((size_t)d + (size_t)kb * b * b + (size_t)lj * bk + li, v);
      }
    });
  });
}

// the gradient from the slices' partials, slice after slice
template <typename T>
__global__ __launch_bounds__(256) void k_bd_finish(long long plen, int n_slices, const double *__restrict__ part, T *__restrict__ grad) {
  const long long t = (long long)blockIdx.x * 256 + threadIdx.x;
  if (t >= plen) return;
  double s = 0.0;
  for (int k = 0; k < n_slices; ++k) s += part[(size_t)k * plen + t];
  grad[t] = (T)s;
}

// logpdf(q, z) at the caller's points: the forward substitution C_k X_k = Z_k - mu_k per unit in LDS -- the back substitution above on the
// other triangle (lane = point column x a quarter of the row sum).  X and every sum are f64.  Workgroup (tile, ch) owns 16 points and the
// units ch, ch + n_chunks, ...; it leaves part[ch][point] = sum over its units of (-1/2 |x|^2 - sum log C_ii); std: X itself, d x n.
// LDS: Cs [R16][R16 + 1] (T) | X [R16][16] (f64)
template <typename T>
__global__ __launch_bounds__(64) void k_bd_logpdf(BdShape s, const T *__restrict__ params, const T *__restrict__ Z, int n, T *__restrict__ std,
                                                 double *__restrict__ part, int *status) {
  const int R16 = (s.R + 15) & ~15, LDC = R16 + 1;
  double *X = bd_lds;
  T *Cs = (T *)(X + R16 * 16);
  const int d = s.d, b = s.b, lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  const int m0 = blockIdx.x * 16, n_ok = n - m0 < 16 ? n - m0 : 16;
  double acc = 0.0;   // lanes < 16: the column's sum over this workgroup's units
  for (int u = blockIdx.y; u < s.n_units; u += gridDim.y) {
    const int r0 = u * s.R, Ru = d - r0 < s.R ? d - r0 : s.R;
    __syncthreads();
    for (int e = lane; e < Ru * Ru; e += 64) {   // the lower triangles of the unit's blocks; nothing else is read below
      const int j = e / Ru, i = e - j * Ru;
      if (j > i || i / b != j / b) continue;
      const int q = i / b, kb = u * s.g + q, bk = d - kb * b < b ? d - kb * b : b;
      Cs[i * LDC + j] = params[(size_t)d + (size_t)kb * b * b + (size_t)(j - q * b) * bk + (i - q * b)];
    }
    for (int e = lane; e < 16 * Ru; e += 64) {
      const int m = e / Ru, row = e - m * Ru;
      X[row * 16 + m] = m < n_ok ? (double)Z[(size_t)(m0 + m) * d + r0 + row] - (double)params[r0 + row] : 0.0;
    }
    __syncthreads();
    double ld = 0.0;
    if (lane < Ru) {
      const double c = (double)Cs[lane * LDC + lane];
      if (!(c > 0.0) && blockIdx.x == 0 && status) atomicOr(status, 2);
      ld = log(c);
    }
    ld = wave_sum(ld);
    for (int i = 0; i < Ru; ++i) {   // rows of another block of the run contribute nothing and are skipped
      double t = 0.0;
      for (int j = (i / b) * b + kq; j < i; j += 4) t += (double)Cs[i * LDC + j] * X[j * 16 + col];
      t += __shfl_xor(t, 16, 64);
      t += __shfl_xor(t, 32, 64);
      if (kq == 0) X[i * 16 + col] = (X[i * 16 + col] - t) / (double)Cs[i * LDC + i];
      __syncthreads();
    }
    if (lane < 16) {
      double q = 0.0;
      for (int i = 0; i < Ru; ++i) q += X[i * 16 + lane] * X[i * 16 + lane];
      acc += -0.5 * q - ld;
    }
    if (std)
      for (int e = lane; e < 16 * Ru; e += 64) {
        const int m = e / Ru, row = e - m * Ru;
        if (m < n_ok) std[(size_t)(m0 + m) * d + r0 + row] = (T)X[row * 16 + m];
      }
  }
  if (lane < n_ok) part[(size_t)blockIdx.y * n + m0 + lane] = acc;
}
// logq[k] = the chunks' partials in chunk order - d/2 log 2 pi
template <typename T>
__global__ __launch_bounds__(256) void k_bd_logpdf_fin(int d, int n, int n_chunks, const double *__restrict__ part, T *__restrict__ logq) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  double s = -0.5 * d * kLog2Pi;
  for (int c = 0; c < n_chunks; ++c) s += part[(size_t)c * n + k];
  logq[k] = (T)s;
}

int bd_logpdf_chunks(const BdShape &s) { return s.n_units < 64 ? s.n_units : 64; }
void launch_bd_logpdf(mivi_ctx *c, const void *params, const void *Z, int n, void *logq, void *std, double *part) {
  const int nc = bd_logpdf_chunks(c->bd), R16 = (c->bd.R + 15) & ~15;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    const size_t lds = (size_t)R16 * 16 * sizeof(double) + (size_t)R16 * (R16 + 1) * sizeof(T);   // at most 41 KB
    hipLaunchKernelGGL(k_bd_logpdf<T>, dim3((n + 15) / 16, nc), dim3(64), lds, c->stream, c->bd, (const T *)params, (const T *)Z, n, (T *)std, part,
                       (int *)c->status.p);
    hipLaunchKernelGGL(k_bd_logpdf_fin<T>, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->cfg.d, n, nc, (const double *)part, (T *)logq);
  });
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
template <typename T, int NT, int MODE>
static bool bd_attr() {
  const size_t bytes = (size_t)bd_lds_elems<NT>() * sizeof(T);
  if (bytes <= 48 * 1024) return true;   // above 48 KB the runtime has to be told
  return hipFuncSetAttribute(reinterpret_cast<const void *>(&k_bd<T, NT, MODE>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes) == hipSuccess;
}
template <typename T, int NT>
static bool bd_attr_modes() { return bd_attr<T, NT, 0>() && bd_attr<T, NT, 1>() && bd_attr<T, NT, 2>(); }

bool bd_prepare(mivi_ctx *c) {
  const int nt = (c->bd.R + 15) / 16;
  return by_dtype(c, [&](auto t) {
    using T = decltype(t);
    return nt == 1 ? bd_attr_modes<T, 1>() : nt == 2 ? bd_attr_modes<T, 2>() : nt == 3 ? bd_attr_modes<T, 3>() : bd_attr_modes<T, 4>();
  });
}

template <typename T, int MODE>
static void bd_launch(mivi_ctx *c, const BdArgs<T> &a) {
  const dim3 grid(a.s.n_units, a.n_slices), block(64);
  switch ((a.s.R + 15) / 16) {
    case 1: hipLaunchKernelGGL((k_bd<T, 1, MODE>), grid, block, bd_lds_elems<1>() * sizeof(T), c->stream, a); break;
    case 2: hipLaunchKernelGGL((k_bd<T, 2, MODE>), grid, block, bd_lds_elems<2>() * sizeof(T), c->stream, a); break;
    case 3: hipLaunchKernelGGL((k_bd<T, 3, MODE>), grid, block, bd_lds_elems<3>() * sizeof(T), c->stream, a); break;
    default: hipLaunchKernelGGL((k_bd<T, 4, MODE>), grid, block, bd_lds_elems<4>() * sizeof(T), c->stream, a); break;
  }
}

template <typename T>
static BdArgs<T> bd_args(mivi_ctx *c, const void *params, const RngArgs &rng, int M) {
  BdArgs<T> a{};
  a.s = c->bd;
  a.M = M;
  a.n_slices = bd_slices(c->bd, M);
  a.params = (const T *)params;
  a.rng = rng;
  return a;
}

// [he (n_units x n_slices) | ell (the same) | ld (2 x n_units)] of c->bd_sc
static double *bd_he(const mivi_ctx *c) { return (double *)c->bd_sc.p; }
static double *bd_ell(const mivi_ctx *c) { return bd_he(c) + (size_t)c->bd.n_units * c->bd.ns_max; }
static double *bd_ld(const mivi_ctx *c) { return bd_ell(c) + (size_t)c->bd.n_units * c->bd.ns_max; }

void launch_bd_forward(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *Z, void *eps, bool stats) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    BdArgs<T> a = bd_args<T>(c, params, rng, M);
    a.Z = (T *)Z;
    a.eps = (T *)eps;
    a.he_part = stats ? bd_he(c) : nullptr;
    a.ld_part = stats ? bd_ld(c) : nullptr;
    bd_launch<T, 0>(c, a);
  });
}

// the VJP (fused: the whole estimate) and, with more than one slice, the finish; wires the value's partials into vin
void launch_bd_grad(mivi_ctx *c, const void *params, const RngArgs &rng, int M, bool fused, ValueIn &vin, const OutArgs &out) {
  const int ek = out.ent_kind;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    BdArgs<T> a = bd_args<T>(c, params, rng, M);
    a.W = (const T *)c->W.p;
    a.t_mean = (const T *)c->t_mean.p;
    a.t_istd = (const T *)c->t_istd.p;
    a.he_part = bd_he(c);
    a.ell_part = bd_ell(c);
    a.ld_part = bd_ld(c);
    a.part = a.n_slices > 1 ? (double *)c->bd_part.p : nullptr;
    a.grad = (T *)out.grad;
    a.stl = ek == MIVI_ENT_STL || ek == MIVI_ENT_STL_ZERO_GRAD;
    a.direct = ek == MIVI_ENT_CLOSED_FORM || ek == MIVI_ENT_MONTE_CARLO ? 1.0 : ek == MIVI_ENT_STL_ZERO_GRAD ? -1.0 : 0.0;   // direct_entropy_coeff
    a.invM = 1.0 / (double)out.M_total;
    if (fused) bd_launch<T, 2>(c, a);
    else bd_launch<T, 1>(c, a);
    if (a.n_slices > 1)
      hipLaunchKernelGGL(k_bd_finish<T>, dim3((unsigned)((a.s.plen + 255) / 256)), dim3(256), 0, c->stream, a.s.plen, a.n_slices, (const double *)c->bd_part.p, (T *)out.grad);
  });
  bd_wire_value(c, M, fused, vin);
}

void bd_wire_value(const mivi_ctx *c, int M, bool fused, ValueIn &vin) {
  const int n = c->bd.n_units * bd_slices(c->bd, M);
  vin.he_part = bd_he(c);
  vin.n_he_part = n;
  if (fused) {
    vin.ell_part = bd_ell(c);
    vin.n_ell_part = n;
  }
  vin.ld_part = bd_ld(c);
  vin.n_ld_part = c->bd.n_units;
}

size_t bd_sc_bytes(const BdShape &s) { return ((size_t)s.n_units * s.ns_max * 2 + (size_t)s.n_units * 2) * sizeof(double); }

}  // namespace mivi
