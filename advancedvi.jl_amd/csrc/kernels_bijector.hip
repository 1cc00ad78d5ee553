// The extended Stacked bijector (mivi_set_bijector_stacked_ex): bounded / half-bounded (`truncated(lb, ub)`) and ordered blocks next to the
// identity / exp blocks of kernels_targets.hip -- the maps Bijectors.jl attaches to Uniform / Beta / truncated supports and to ordered
// vectors (docs/src/tutorials/constrained.md:154-231).  eta is the unconstrained coordinate the family draws, x = binv(eta) what the target sees.
//
//   BIJ_LOWER     x = lb + e^eta                  ladj += eta                                     d/d eta =  e^eta g + 1
//   BIJ_UPPER     x = ub - e^eta                  ladj += eta                                     d/d eta = -e^eta g + 1
//   BIJ_BOTH      x = lb + (ub - lb) sigma(eta)   ladj += log(ub - lb) - |eta| - 2 log1p(e^-|eta|)  d/d eta = (ub - lb) s (1 - s) g + (1 - 2 s)
//   BIJ_ORD_HEAD  x_b = eta_b                                                                     d/d eta = S_b
//   BIJ_ORD       x_k = x_{k-1} + e^eta_k         ladj += eta_k                                   d/d eta = e^eta_k S_k + 1,  S_k = sum_{j >= k in block} g_j
//
// One workgroup per sample column, as k_bij_fwd / k_bij_bwd: ld[m] is one fixed-order f64 block sum, so two calls agree bit for bit.  The
// ordered kind is a segmented scan along the column (forward: inclusive prefix sums with heads at block starts; backward: the mirrored suffix
// sums with heads at block ends), carried in f64 across the 256-row chunks of a long column and rounded once to T.
// The backward pass takes every Jacobian factor from eta -- the forward pass saves it (`save`, d x cap_M, mivi_ctx::bij_eta) -- never from
// differences of the stored x: in f32 x - lb and x_k - x_{k-1} cancel as soon as |lb| or x_b is large against the increment.
// The exp kind is BIJ_LOWER with lb = 0: e^eta in T as k_bij_fwd forms it, 0 + e exact, fma(e, g, 1) as k_bij_bwd -- bitwise the legacy kind.
#include "device_common.h"

namespace mivi {

// Inclusive segmented scan of (v, head) over the 256 threads of the workgroup, continuing the segment `carry` belongs to; returns this
// thread's running sum and leaves the sum at thread 255 in `carry`.  (f, v) o (f', v') = (f | f', f' ? v' : v + v'): Hillis-Steele in LDS,
// a fixed order.  Every thread of the workgroup must call it.
__device__ __forceinline__ double seg_scan256(double v, int f, double &carry, double *sv, int *sf) {
  const int tid = threadIdx.x;
  __syncthreads();   // (the previous chunk's reads of sv / sf)
  sv[tid] = v;
  sf[tid] = f;
  __syncthreads();
#pragma unroll
  for (int off = 1; off < 256; off <<= 1) {
    double pv = 0.0;
    int pf = 0;
    if (tid >= off) { pv = sv[tid - off]; pf = sf[tid - off]; }
    __syncthreads();
    if (tid >= off) {
      if (!f) v = pv + v;
      f |= pf;
      sv[tid] = v;
      sf[tid] = f;
    }
    __syncthreads();
  }
  if (!f) v = carry + v;   // no head between the chunk's first row and this one
  if (tid == 255) sv[0] = v;
  __syncthreads();
  carry = sv[0];
  return v;
}

// the smaller of sigma(eta), 1 - sigma(eta): p = e^-|eta| / (1 + e^-|eta|), never a saturated difference
__device__ __forceinline__ double sigmoid_small_side(double eta, double &t) {
  t = exp(-fabs(eta));
  return t / (1.0 + t);
}

template <typename T>
__global__ __launch_bounds__(256) void k_bijx_fwd(int d, const uint8_t *code, const double *bnd, int has_ord, T *Z, T *save, T *ld) {
  __shared__ double red[4];
  __shared__ double sv[256];
  __shared__ int sf[256];
  const int m = blockIdx.x, tid = threadIdx.x;
  T *z = Z + (size_t)m * d;
  T *sc = save ? save + (size_t)m * d : nullptr;
  double acc = 0.0, carry = 0.0;
  for (int base = 0; base < d; base += 256) {
    const int i = base + tid;
    const bool in = i < d;
    const int k = in ? code[i] : BIJ_ID;
    const T eta = in ? z[i] : T(0);
    if (in && sc) sc[i] = eta;
    double v = 0.0;
    int head = 1;   // rows of no ordered block are segments of their own
    if (k == BIJ_LOWER) {
      acc += (double)eta;
      z[i] = (T)(bnd[2 * i] + (double)exp(eta));
    } else if (k == BIJ_UPPER) {
      acc += (double)eta;
      z[i] = (T)(bnd[2 * i + 1] - (double)exp(eta));
    } else if (k == BIJ_BOTH) {
      const double lo = bnd[2 * i], hi = bnd[2 * i + 1], w = hi - lo, h = (double)eta;
      double t;
      const double p = sigmoid_small_side(h, t);
      acc += log(w) - fabs(h) - 2.0 * log1p(t);
      z[i] = (T)(h >= 0.0 ? hi - w * p : lo + w * p);
    } else if (k == BIJ_ORD_HEAD) {
      v = (double)eta;
    } else if (k == BIJ_ORD) {
      acc += (double)eta;
      v = exp((double)eta);
      head = 0;
    }
    if (has_ord) {
      const double x = seg_scan256(v, head, carry, sv, sf);
      if (k == BIJ_ORD) z[i] = (T)x;
    }
  }
  const double s = block_sum<double, 256>(acc, red);
  if (ld && tid == 0) ld[m] = (T)s;
}

template <typename T>
__global__ __launch_bounds__(256) void k_bijx_bwd(int d, const uint8_t *code, const double *bnd, int has_ord, const T *save, T *G, T *ell,
                                                  const T *ld, int want_grad) {
  __shared__ double sv[256];
  __shared__ int sf[256];
  const int m = blockIdx.x, tid = threadIdx.x;
  if (want_grad) {
    const T *e = save + (size_t)m * d;
    T *g = G + (size_t)m * d;
    double carry = 0.0;
    for (int base = 0; base < d; base += 256) {   // rows from the last to the first: the suffix sums are prefix sums of the mirrored column
      const int i = d - 1 - (base + tid);
      const bool in = i >= 0;
      const int k = in ? code[i] : BIJ_ID;
      const T eta = in ? e[i] : T(0);
      const T gi = in ? g[i] : T(0);
      double v = 0.0;
      int head = 1;
      if (k == BIJ_LOWER) {
        g[i] = fma(exp(eta), gi, T(1));
      } else if (k == BIJ_UPPER) {
        g[i] = fma(-exp(eta), gi, T(1));
      } else if (k == BIJ_BOTH) {
        const double w = bnd[2 * i + 1] - bnd[2 * i], h = (double)eta;
        double t;
        const double p = sigmoid_small_side(h, t);
        g[i] = (T)(w * p * (1.0 - p) * (double)gi + (h >= 0.0 ? 2.0 * p - 1.0 : 1.0 - 2.0 * p));
      } else if (k == BIJ_ORD_HEAD || k == BIJ_ORD) {
        v = (double)gi;
        head = (i + 1 >= d || code[i + 1] != BIJ_ORD) ? 1 : 0;   // the block's last row heads the mirrored segment
      }
      if (has_ord) {
        const double S = seg_scan256(v, head, carry, sv, sf);
        if (k == BIJ_ORD_HEAD) g[i] = (T)S;
        else if (k == BIJ_ORD) g[i] = (T)(exp((double)eta) * S + 1.0);
      }
    }
  }
  if (ell && tid == 0) ell[m] += ld[m];
}

// The inverse direction, for logpdf of the transformed distribution at the caller's constrained points: eta = b(x) per column,
// ladj[m] = logabsdetjac(binv, eta) in f64, flag[m] bit 0: a finite point outside the support, bit 1: a NaN coordinate (eta is 0 there,
// so that the density kernels behind this one see finite data; k_bijx_fin writes the column's -inf / NaN).
template <typename T>
__global__ __launch_bounds__(256) void k_bijx_inv(int d, const uint8_t *code, const double *bnd, const T *X, T *E, double *ladj, int *flag) {
  __shared__ double red[4];
  const int m = blockIdx.x, tid = threadIdx.x;
  const T *x = X + (size_t)m * d;
  T *e = E + (size_t)m * d;
  double acc = 0.0, n_out = 0.0, n_nan = 0.0;
  for (int i = tid; i < d; i += 256) {
    const int k = code[i];
    const double xi = (double)x[i];
    double h = xi, t = 1.0;
    bool nan = isnan(xi), out = false;
    if (k == BIJ_LOWER) t = xi - bnd[2 * i];
    else if (k == BIJ_UPPER) t = bnd[2 * i + 1] - xi;
    else if (k == BIJ_ORD) {
      t = xi - (double)x[i - 1];
      nan = nan || isnan(t);   // (the previous row's NaN, or inf - inf)
    }
    if (k == BIJ_LOWER || k == BIJ_UPPER || k == BIJ_ORD) {
      if (t > 0.0 && !isinf(t)) { h = log(t); acc += h; }
      else out = true;
    } else if (k == BIJ_BOTH) {
      const double lo = bnd[2 * i], w = bnd[2 * i + 1] - lo, u = (xi - lo) / w;
      if (u > 0.0 && u < 1.0) {
        const double lu = log(u), l1 = log1p(-u);
        h = lu - l1;
        acc += log(w) + lu + l1;
      } else out = true;
    }
    if (nan) n_nan += 1.0;
    else if (out) n_out += 1.0;
    e[i] = (nan || out) ? T(0) : (T)h;
  }
  const double s = block_sum<double, 256>(acc, red);
  const double so = block_sum<double, 256>(n_out, red);
  const double sn = block_sum<double, 256>(n_nan, red);
  if (tid == 0) {
    ladj[m] = s;
    flag[m] = (so > 0.0 ? 1 : 0) | (sn > 0.0 ? 2 : 0);
  }
}

// logq[k] = log q(b(x_k)) - ladj[k]; exactly -inf outside the support, NaN for a NaN point
template <typename T>
__global__ __launch_bounds__(256) void k_bijx_fin(int n, T *logq, const double *ladj, const int *flag) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= n) return;
  const int f = flag[k];
  const double v = (double)logq[k] - ladj[k];
  logq[k] = (f & 2) ? (T)NAN : (f & 1) ? (T)(-INFINITY) : (T)v;
}

void launch_bijx_forward(mivi_ctx *c, int M, void *Z, void *save, void *ld) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bijx_fwd<T>, dim3(M), dim3(256), 0, c->stream, c->cfg.d, (const uint8_t *)c->bij_code.p, (const double *)c->bij_bnd.p,
                       (int)c->bij_ord, (T *)Z, (T *)save, (T *)ld);
  });
}
void launch_bijx_backward(mivi_ctx *c, int M, int want_grad, bool add_to_ell) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bijx_bwd<T>, dim3(M), dim3(256), 0, c->stream, c->cfg.d, (const uint8_t *)c->bij_code.p, (const double *)c->bij_bnd.p,
                       (int)c->bij_ord, (const T *)c->bij_eta.p, (T *)c->W.p, add_to_ell ? (T *)c->ell.p : nullptr, (const T *)c->bij_ld.p, want_grad);
  });
}
void launch_bijx_inverse(mivi_ctx *c, int n, const void *X, void *eta, double *ladj, int *flag) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bijx_inv<T>, dim3(n), dim3(256), 0, c->stream, c->cfg.d, (const uint8_t *)c->bij_code.p, (const double *)c->bij_bnd.p,
                       (const T *)X, (T *)eta, ladj, flag);
  });
}
void launch_bijx_finish(mivi_ctx *c, int n, void *logq, const double *ladj, const int *flag) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    hipLaunchKernelGGL(k_bijx_fin<T>, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, (T *)logq, ladj, flag);
  });
}

}  // namespace mivi
