// The neural spline flow family (MIVI_NSF; include/mivi.h holds the definition): the kernels of one RepGradELBO estimate, of rand and of
// logpdf.  The launchers of kernels_flow.hip branch here on a context with bins; api_flow.hip drives them, and the finish kernel is RealNVP's.
//
// The shape is RealNVP's (kernels_flow.hip): one workgroup is ONE wave on tiles of 16 samples, a tile's quantities are [row][16] blocks in
// LDS, every product of a net's layer is whole 16 x 16 x 4 matrix-core steps (Mfma16), every x^l is saved by the forward pass and the nets
// are recomputed in the backward sweeps from the saved x^{l-1} with the forward pass's own code.  What differs:
//   * ONE net per layer, and its output layer has |A_l| (3K - 1) rows -- up to 64 x 47.  It is never held whole: a layer is walked in
//     CHUNKS of whole coordinates, floor(64 / (3K - 1)) of them, one [64][16] block (S) at a time: chunk forward -> the spline of the
//     chunk's coordinates, lane = (coordinate, sample) -> [backward: the cotangents of the raw outputs replace them in S; the chunk's
//     weight and bias gradients go straight to the slice's partial vector; its input VJP W_chunk' delta is added into matrix-core
//     accumulators that live across the chunks (4 x acc_t: the last hidden layer has at most 64 units)].  LDS does not grow with K.
//   * the coupling is the monotone rational-quadratic spline: nsf_widths (softmax -> w, h in place), nsf_bin (the search, knots as running
//     sums of w / h), nsf_spline_eval (forward, or the analytic inverse), nsf_spline_vjp (the cotangents of a, u^w, u^h, u^d from those of
//     y and of log y'; w, h, delta always from the recomputed raw outputs).  Values are T, a sample's sum of log y' is f64.
//   k_nsf_forward   draws -> x^0 ... x^L = z; saves every x^l (flow_X) and the f64 log q per sample.  INVERSE: z -> eps, log q (mivi_logpdf)
//   k_nsf_vjp       workgroup s owns the tiles s, s + n_slices, ...: [sticking the landing: u = grad_z log q by a sweep l = 1 .. L through
//                   the inverse layers, input VJPs only] then the sweep l = L .. 1; f64 partials per slice, tile after tile -- no atomics
#include "flow_tile.h"

namespace mivi {

__device__ __forceinline__ float nsf_exp(float x) { return expf(x); }
__device__ __forceinline__ double nsf_exp(double x) { return exp(x); }
__device__ __forceinline__ float nsf_log(float x) { return logf(x); }
__device__ __forceinline__ double nsf_log(double x) { return log(x); }
__device__ __forceinline__ float nsf_log1p(float x) { return log1pf(x); }
__device__ __forceinline__ double nsf_log1p(double x) { return log1p(x); }
__device__ __forceinline__ float nsf_sqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ double nsf_sqrt(double x) { return sqrt(x); }

// where layer l's parameters start: the layers before it are l / 2 odd ones and (l - 1) / 2 even ones
__device__ __forceinline__ long long nsf_layer_off(const FlowArch &a, int l) {
  const int nA1 = flow_nA(a.d, 1), nA2 = flow_nA(a.d, 2), P = nsf_rows(a);
  return (long long)(l / 2) * flow_net_len(a, a.d - nA1, nA1 * P) + (long long)((l - 1) / 2) * flow_net_len(a, a.d - nA2, nA2 * P);
}

// ---- a net's layer, rows [r0, r0 + nr) of it (nr <= 64): W is out x prev, column-major ---------------------------------------------------
// dst[row - r0][16] = W in + b (leakyrelu of it: leaky), zero rows up to a multiple of 16; `in` has zero rows up to a multiple of 16
template <typename T>
__device__ void nsf_layer_forward(const T *Wm, const T *bv, int out, int prev, int r0, int nr, bool leaky, const T *in, T *dst) {
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  for (int o0 = 0; o0 < nr; o0 += 16) {
    typename Mfma16<T>::acc_t acc = {0, 0, 0, 0};
    const int o = o0 + col;
    for (int k0 = 0; k0 < prev; k0 += 4) {
      const int k = k0 + kq;
      const T av = (o < nr && k < prev) ? Wm[r0 + o + (size_t)k * out] : T(0);
      acc = Mfma16<T>::mma(av, in[k * 16 + col], acc);
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = o0 + Mfma16<T>::row(kq, r);
      T v = T(0);
      if (row < nr) {
        v = acc[r] + bv[r0 + row];
        if (leaky) v = v > T(0) ? v : T(0.01) * v;
      }
      dst[row * 16 + col] = v;
    }
  }
  __syncthreads();
}
// the hidden layers: Hb[0] holds the input, Hb[1 .. H] receive the activations.  Returns the output layer's parameters.
template <typename T>
__device__ const T *nsf_hidden_forward(const FlowArch &a, const T *np, int nin, T *Hb) {
  int prev = nin;
  for (int j = 0; j < a.H; ++j) {
    const int out = a.h[j];
    nsf_layer_forward(np, np + (size_t)out * prev, out, prev, 0, out, true, Hb + j * kFlowBlk, Hb + (j + 1) * kFlowBlk);
    np += (size_t)out * prev + out;
    prev = out;
  }
  return np;
}
// dW[r0 + row][ci] = sum over the tile's samples of delta[row] h[ci], db likewise: stored into the partial if `first`, added otherwise
template <typename T>
__device__ void nsf_weight_vjp(const T *dl, const T *hin, int out, int in_, int r0, int nr, double *pW, double *pb, bool first) {
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  for (int o0 = 0; o0 < nr; o0 += 16)
    for (int i0 = 0; i0 < in_; i0 += 16) {
      typename Mfma16<T>::acc_t acc = {0, 0, 0, 0};
#pragma unroll
      for (int k0 = 0; k0 < 16; k0 += 4) acc = Mfma16<T>::mma(dl[(o0 + col) * 16 + k0 + kq], hin[(i0 + col) * 16 + k0 + kq], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = o0 + Mfma16<T>::row(kq, r), ci = i0 + col;
        if (row < nr && ci < in_) {
          const size_t e = r0 + row + (size_t)ci * out;
          pW[e] = first ? (double)acc[r] : pW[e] + (double)acc[r];
        }
      }
    }
  for (int o = lane; o < nr; o += 64) {
    double s = 0.0;
    for (int m = 0; m < 16; ++m) s += (double)dl[o * 16 + m];
    pb[r0 + o] = first ? s : pb[r0 + o] + s;
  }
}
// acc[ib] += W[r0 .. r0 + nr, 16 ib .. 16 ib + 16]' delta: the input VJP of the rows, block ib of the inputs (in_ <= 64)
template <typename T>
__device__ __forceinline__ void nsf_input_vjp(const T *Wm, int out, int in_, int r0, int nr, const T *dl, typename Mfma16<T>::acc_t (&acc)[4]) {
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ib = 0; ib < 4; ++ib) {
    const int i = 16 * ib + col;
    if (16 * ib < in_)
      for (int k0 = 0; k0 < nr; k0 += 4) {
        const int k = k0 + kq;
        const T av = (i < in_ && k < nr) ? Wm[r0 + k + (size_t)i * out] : T(0);
        acc[ib] = Mfma16<T>::mma(av, dl[k * 16 + col], acc[ib]);
      }
  }
}
// the accumulators -> dst[in_][16] (zero rows up to a multiple of 16), times the leakyrelu slope at hin where hin is given
template <typename T>
__device__ __forceinline__ void nsf_store_vjp(const typename Mfma16<T>::acc_t (&acc)[4], int in_, const T *hin, T *dst) {
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int ib = 0; ib < 4; ++ib)
    if (16 * ib < in_) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ib + Mfma16<T>::row(kq, r);
        T v = T(0);
        if (row < in_) {
          v = acc[ib][r];
          if (hin) v *= hin[row * 16 + col] > T(0) ? T(1) : T(0.01);
        }
        dst[row * 16 + col] = v;
      }
    }
  __syncthreads();
}

// ---- the spline of one coordinate at one sample: u points at its 3K - 1 raw outputs in S, stride 16 -------------------------------------
template <typename T>
__device__ __forceinline__ T nsf_softplus(T u) { return (u > T(0) ? u : T(0)) + nsf_log1p(nsf_exp(u > T(0) ? -u : u)); }
template <typename T>
__device__ __forceinline__ T nsf_sigmoid(T u) {
  const T e = nsf_exp(u > T(0) ? -u : u);
  return (u > T(0) ? T(1) : e) / (T(1) + e);
}
// u_1 .. u_K -> 2B softmax(u), in place
template <typename T>
__device__ __forceinline__ void nsf_widths(T *u, int K, T B2) {
  T mx = u[0];
  for (int k = 1; k < K; ++k) mx = u[k * 16] > mx ? u[k * 16] : mx;
  T sum = T(0);
  for (int k = 0; k < K; ++k) {
    const T e = nsf_exp(u[k * 16] - mx);
    u[k * 16] = e;
    sum += e;
  }
  for (int k = 0; k < K; ++k) u[k * 16] = B2 * u[k * 16] / sum;
}
template <typename T>
struct NsfBin {
  int k;             // 0-based: the knots k and k + 1 bound it
  T w, h, d0, d1;    // its width, height and the slopes at its two knots
  T X0, Y0;          // its left knot
};
// the bin of v among the knots X (onY: Y): v >= knot j moves past it, j = 1 .. K - 1; the knots are the running sums -B + w_1 + ... in T
template <typename T>
__device__ __forceinline__ NsfBin<T> nsf_bin(const T *u, int K, T B, T v, bool onY) {
  NsfBin<T> b;
  b.k = 0;
  b.X0 = -B;
  b.Y0 = -B;
  for (int j = 0; j < K - 1; ++j) {
    const T Xn = b.X0 + u[j * 16], Yn = b.Y0 + u[(K + j) * 16];
    if (!(v >= (onY ? Yn : Xn))) break;
    b.X0 = Xn;
    b.Y0 = Yn;
    b.k = j + 1;
  }
  b.w = u[b.k * 16];
  b.h = u[(K + b.k) * 16];
  b.d0 = b.k == 0 ? T(1) : nsf_softplus(u[(2 * K + b.k - 1) * 16]);
  b.d1 = b.k == K - 1 ? T(1) : nsf_softplus(u[(2 * K + b.k) * 16]);
  return b;
}
// forward: v = a -> y; INVERSE: v = y -> a.  ld = log y'(a) for both.  Outside (-B, B): the identity, ld = 0.  Overwrites u^w, u^h.
template <typename T, bool INVERSE>
__device__ __forceinline__ T nsf_spline_eval(T *u, int K, T B, T v, T &ld) {
  ld = T(0);
  if (!(v > -B && v < B)) return v;
  nsf_widths(u, K, T(2) * B);
  nsf_widths(u + K * 16, K, T(2) * B);
  const NsfBin<T> b = nsf_bin(u, K, B, v, INVERSE);
  const T s = b.h / b.w, t = b.d1 + b.d0 - T(2) * s;
  T xi, res;
  if (INVERSE) {   // the root of the quadratic in xi, in the form without cancellation
    const T dy = v - b.Y0;
    const T qa = b.h * (s - b.d0) + dy * t, qb = b.h * b.d0 - dy * t, qc = -s * dy;
    xi = T(2) * qc / (-qb - nsf_sqrt(qb * qb - T(4) * qa * qc));
    res = b.X0 + xi * b.w;
  } else {
    xi = (v - b.X0) / b.w;
  }
  const T om = T(1) - xi, p = xi * om, D = s + t * p;
  if (!INVERSE) res = b.Y0 + b.h * (s * xi * xi + b.d0 * p) / D;
  ld = T(2) * nsf_log(s) + nsf_log(b.d1 * xi * xi + T(2) * s * p + b.d0 * om * om) - T(2) * nsf_log(D);
  return res;
}
// The cotangents of the raw outputs replace them in u.  Parameter sweep (!USWEEP): gin is the cotangent of y and kap that of log y';
// returns the cotangent of a.  USWEEP (u = grad_z log q through the inverse layer a = f^-1(y), log q -= log y'(a)): gin is the cotangent of
// a; with abar = gin - d log y' / da the raw outputs receive -(abar / y') df/du - d log y'/du, and abar / y', that of y, is returned.
template <typename T, bool USWEEP>
__device__ __forceinline__ T nsf_spline_vjp(T *u, int K, T B, T a, T gin, T kap) {
  const int P = 3 * K - 1;
  if (!(a > -B && a < B)) {
    for (int r = 0; r < P; ++r) u[r * 16] = T(0);
    return gin;
  }
  nsf_widths(u, K, T(2) * B);
  nsf_widths(u + K * 16, K, T(2) * B);
  const NsfBin<T> b = nsf_bin(u, K, B, a, false);
  const T w = b.w, h = b.h, d0 = b.d0, d1 = b.d1;
  const T xi = (a - b.X0) / w, s = h / w, om = T(1) - xi, p = xi * om, t = d1 + d0 - T(2) * s, m2 = T(1) - T(2) * xi;
  const T D = s + t * p, N = s * xi * xi + d0 * p, Q = d1 * xi * xi + T(2) * s * p + d0 * om * om;
  const T hD2 = h / (D * D);
  const T g_xi = (T(2) * d1 * xi + T(2) * s * m2 - T(2) * d0 * om) / Q - T(2) * t * m2 / D;
  const T g_s = T(2) / s + T(2) * p / Q - T(2) * (T(1) - T(2) * p) / D;
  const T g_d0 = om * om / Q - T(2) * p / D, g_d1 = xi * xi / Q - T(2) * p / D;
  const T y_xi = hD2 * s * Q, y_s = hD2 * (xi * xi * D - N * (T(1) - T(2) * p)), y_d0 = hD2 * p * (D - N), y_d1 = -hD2 * N * p, y_h = N / D;
  T gy = gin, ret = T(0);
  if (USWEEP) {
    const T fa = s * s * Q / (D * D);
    ret = (gin - g_xi / w) / fa;
    gy = -ret;
    kap = T(-1);
  }
  const T c_xi = gy * y_xi + kap * g_xi, c_s = gy * y_s + kap * g_s, c_d0 = gy * y_d0 + kap * g_d0, c_d1 = gy * y_d1 + kap * g_d1;
  const T c_a = c_xi / w;
  if (!USWEEP) ret = c_a;
  // w_k, h_k; the knots to the left: X0 = -B + w_1 + ... + w_{k-1} takes -c_a, Y0 takes gy
  const T c_wk = -(c_xi * xi + c_s * s) / w, c_hk = gy * y_h + c_s / w;
  T dotw = c_wk * w, doth = c_hk * h;
  for (int j = 0; j < b.k; ++j) {
    dotw += -c_a * u[j * 16];
    doth += gy * u[(K + j) * 16];
  }
  dotw /= T(2) * B;
  doth /= T(2) * B;
  for (int j = 0; j < K; ++j) {   // softmax: c_u_j = w_j (c_w_j - sum_i c_w_i w_i / 2B)
    const T cw = j < b.k ? -c_a : j == b.k ? c_wk : T(0), ch = j < b.k ? gy : j == b.k ? c_hk : T(0);
    u[j * 16] = u[j * 16] * (cw - dotw);
    u[(K + j) * 16] = u[(K + j) * 16] * (ch - doth);
  }
  for (int j = 0; j < K - 1; ++j) {   // raw slope j belongs to knot j + 1: the bin's left knot is k, its right knot k + 1
    T *ud = u + (2 * K + j) * 16;
    const T cd = j == b.k - 1 ? c_d0 : j == b.k ? c_d1 : T(0);
    *ud = (j == b.k - 1 || j == b.k) ? cd * nsf_sigmoid(*ud) : T(0);
  }
  return ret;
}

// ---- the kernels -----------------------------------------------------------------------------------------------------------------------
// LDS: XC [128][16] | H [4][64][16] | S [64][16] | LD [64][16]
constexpr int kNsfFwdElems = 128 * 16 + 6 * kFlowBlk;
template <typename T, bool INVERSE>
__global__ __launch_bounds__(64) void k_nsf_forward(FlowArgs<T> g) {
  __shared__ double he[16], ss[16];
  T *XC = (T *)flow_lds, *Hb = XC + 128 * 16, *S = Hb + 4 * kFlowBlk, *LD = S + kFlowBlk;
  const FlowArch &a = g.a;
  const int d = a.d, lane = threadIdx.x, m0 = blockIdx.x * kFlowTile, P = nsf_rows(a), cpc = 64 / P;
  const int n_ok = g.M - m0 < 16 ? g.M - m0 : 16;
  const T B = (T)a.B;
  if (INVERSE) {
    flow_load_tile(g.Zin + (size_t)m0 * d, XC, d, n_ok);
  } else {
    flow_draw_tile(g.rng, XC, d, m0, n_ok);
    if (g.eps) flow_store_tile(g.eps + (size_t)m0 * d, XC, d, n_ok);
    if (g.X) flow_store_tile(g.X + (size_t)m0 * d, XC, d, 16);
  }
  if (lane < 16) {
    double h = 0.0;
    if (!INVERSE)
      for (int i = 0; i < d; ++i) h += (double)XC[i * 16 + lane] * (double)XC[i * 16 + lane];
    he[lane] = 0.5 * h;
    ss[lane] = 0.0;
  }
  for (int step = 1; step <= a.L; ++step) {
    const int l = INVERSE ? a.L + 1 - step : step;
    const int pa = (l & 1) ? 0 : 1, nA = flow_nA(d, l), nB = d - nA, out = nA * P, prevH = a.h[a.H - 1];
    flow_take_c(XC, Hb, nB, pa);
    const T *Wo = nsf_hidden_forward(a, g.params + nsf_layer_off(a, l), nB, Hb), *bo = Wo + (size_t)out * prevH;
    for (int i0 = 0; i0 < nA; i0 += cpc) {
      const int nc = nA - i0 < cpc ? nA - i0 : cpc;
      nsf_layer_forward(Wo, bo, out, prevH, i0 * P, nc * P, false, Hb + a.H * kFlowBlk, S);
      for (int e = lane; e < nc * 16; e += 64) {
        const int jl = e >> 4, m = e & 15, j = i0 + jl;
        T ld;
        XC[(2 * j + pa) * 16 + m] = nsf_spline_eval<T, INVERSE>(S + jl * P * 16 + m, a.K, B, XC[(2 * j + pa) * 16 + m], ld);
        LD[j * 16 + m] = ld;
      }
      __syncthreads();
    }
    if (lane < 16) {
      double s = 0.0;
      for (int j = 0; j < nA; ++j) s += (double)LD[j * 16 + lane];
      ss[lane] += s;
    }
    __syncthreads();
    if (!INVERSE && g.X) flow_store_tile(g.X + ((size_t)l * g.capM + m0) * d, XC, d, 16);
  }
  if (!INVERSE && g.Z) flow_store_tile(g.Z + (size_t)m0 * d, XC, d, n_ok);
  // log q = -1/2 |eps|^2 - d/2 log 2 pi - sum_l sum_i log y'_{l,i} (the forward pass summed |eps|^2 before the layers)
  if (INVERSE) {
    if (lane < n_ok) {
      double h = 0.0;
      for (int i = 0; i < d; ++i) h += (double)XC[i * 16 + lane] * (double)XC[i * 16 + lane];
      g.logq[m0 + lane] = (T)(-0.5 * h - 0.5 * d * kLog2Pi - ss[lane]);
    }
  } else if (g.lq && lane < n_ok) {
    g.lq[m0 + lane] = -he[lane] - 0.5 * d * kLog2Pi - ss[lane];
  }
}

// One layer of a backward sweep on a tile: G (the [d][16] cotangent block) moves from x^l to x^{l-1} (parameter sweep; the layer's
// parameter gradient goes to `part`) or, USWEEP, from x^{l-1} to x^l through the inverse layer with input VJPs only.
template <typename T, bool USWEEP>
__device__ void nsf_layer_sweep(const FlowArgs<T> &g, int l, int m0, int n_ok, T kappa, T *Hb, T *S, T *D0, T *D1, T *AV, T *G, double *part, bool first) {
  const FlowArch &a = g.a;
  const int d = a.d, lane = threadIdx.x, P = nsf_rows(a), cpc = 64 / P;
  const int pa = (l & 1) ? 0 : 1, nA = flow_nA(d, l), nB = d - nA, out = nA * P, prevH = a.h[a.H - 1];
  const T B = (T)a.B;
  const T *xp = g.X + ((size_t)(l - 1) * g.capM + m0) * d;
  for (int e = lane; e < round16(nB) * 16; e += 64) {
    const int j = e >> 4, m = e & 15;
    Hb[e] = j < nB ? xp[(size_t)m * d + 2 * j + 1 - pa] : T(0);
  }
  for (int e = lane; e < nA * 16; e += 64) AV[e] = xp[(size_t)(e & 15) * d + 2 * (e >> 4) + pa];
  __syncthreads();
  const long long loff = nsf_layer_off(a, l);
  const T *np = g.params + loff;
  const T *Wo = nsf_hidden_forward(a, np, nB, Hb), *bo = Wo + (size_t)out * prevH;
  const T *hin = Hb + a.H * kFlowBlk;
  double *pWo = USWEEP ? nullptr : part + loff + (Wo - np);
  typename Mfma16<T>::acc_t acc[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
  for (int i0 = 0; i0 < nA; i0 += cpc) {
    const int nc = nA - i0 < cpc ? nA - i0 : cpc, r0 = i0 * P, nr = nc * P;
    nsf_layer_forward(Wo, bo, out, prevH, r0, nr, false, hin, S);
    for (int e = lane; e < nc * 16; e += 64) {
      const int jl = e >> 4, m = e & 15, j = i0 + jl;
      T *gp = G + (2 * j + pa) * 16 + m;
      *gp = nsf_spline_vjp<T, USWEEP>(S + jl * P * 16 + m, a.K, B, AV[j * 16 + m], *gp, m < n_ok ? kappa : T(0));
    }
    __syncthreads();
    if (!USWEEP) nsf_weight_vjp(S, hin, out, prevH, r0, nr, pWo, pWo + (size_t)out * prevH, first);
    nsf_input_vjp(Wo, out, prevH, r0, nr, S, acc);
    __syncthreads();
  }
  nsf_store_vjp(acc, prevH, hin, D0);
  T *dcur = D0, *dnext = D1;
  const T *Wj = Wo;
  for (int j = a.H - 1; j >= 0; --j) {
    const int oj = a.h[j], ij = j > 0 ? a.h[j - 1] : nB;
    Wj -= (size_t)oj * ij + oj;
    const T *hj = Hb + j * kFlowBlk;
    if (!USWEEP) {
      double *pW = part + loff + (Wj - np);
      nsf_weight_vjp(dcur, hj, oj, ij, 0, oj, pW, pW + (size_t)oj * ij, first);
    }
    typename Mfma16<T>::acc_t acj[4] = {{0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}, {0, 0, 0, 0}};
    nsf_input_vjp(Wj, oj, ij, 0, oj, dcur, acj);
    nsf_store_vjp(acj, ij, j > 0 ? hj : (const T *)nullptr, dnext);
    T *tmp = dcur; dcur = dnext; dnext = tmp;
  }
  for (int e = lane; e < nB * 16; e += 64) G[(2 * (e >> 4) + 1 - pa) * 16 + (e & 15)] += dcur[e];
  __syncthreads();
}

// LDS: H [4][64][16] | S | D0 | D1 | AV | G [128][16]
constexpr int kNsfVjpElems = 8 * kFlowBlk + 128 * 16;
template <typename T>
__global__ __launch_bounds__(64) void k_nsf_vjp(FlowArgs<T> g, long long plen) {
  T *Hb = (T *)flow_lds, *S = Hb + 4 * kFlowBlk, *D0 = S + kFlowBlk, *D1 = D0 + kFlowBlk, *AV = D1 + kFlowBlk, *G = AV + kFlowBlk;
  const FlowArch &a = g.a;
  const int d = a.d, lane = threadIdx.x, tiles = (g.M + kFlowTile - 1) / kFlowTile;
  double *part = g.part + (size_t)blockIdx.x * plen;
  bool first = true;
  for (int tile = blockIdx.x; tile < tiles; tile += gridDim.x, first = false) {
    const int m0 = tile * kFlowTile;
    const int n_ok = g.M - m0 < 16 ? g.M - m0 : 16;
    if (g.kind == MIVI_ENT_STL) {   // u = grad_z log q(z), the parameters stopped: G runs from -eps to u
      flow_load_tile(g.X + (size_t)m0 * d, G, d, 16, T(-1));
      for (int l = 1; l <= a.L; ++l) nsf_layer_sweep<T, true>(g, l, m0, n_ok, T(0), Hb, S, D0, D1, AV, G, nullptr, false);
      for (int e = lane; e < 16 * d; e += 64) {
        const int m = e / d, i = e - m * d;
        G[i * 16 + m] = m < n_ok ? (T)((-g.Wg[(size_t)(m0 + m) * d + i] + G[i * 16 + m]) * (T)g.invM) : T(0);
      }
      __syncthreads();
    } else {
      flow_load_tile(g.Wg + (size_t)m0 * d, G, d, n_ok, (T)(-g.invM));
    }
    const T kappa = g.kind == MIVI_ENT_STL ? T(0) : (T)(-g.invM);
    for (int l = a.L; l >= 1; --l) nsf_layer_sweep<T, false>(g, l, m0, n_ok, kappa, Hb, S, D0, D1, AV, G, part, first);
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
bool nsf_prepare(mivi_ctx *c) {
  return by_dtype(c, [&](auto t) {
    using T = decltype(t);
    return flow_lds_attr<T>(&k_nsf_forward<T, false>, kNsfFwdElems) && flow_lds_attr<T>(&k_nsf_forward<T, true>, kNsfFwdElems) &&
           flow_lds_attr<T>(&k_nsf_vjp<T>, kNsfVjpElems);
  });
}

void launch_nsf_forward(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *Z, void *eps, bool save) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    FlowArgs<T> g = flow_args<T>(c, params, M);
    g.rng = rng;
    if (save && (c->cap_M % kFlowTile != 0 || M > c->cap_M)) return;   // (never: ensure_work's rounding; a partial last tile would write past its plane)
    g.X = save ? (T *)c->flow_X.p : nullptr;
    g.Z = (T *)Z;
    g.eps = (T *)eps;
    g.lq = save ? (double *)c->flow_lq.p : nullptr;
    hipLaunchKernelGGL((k_nsf_forward<T, false>), dim3((M + kFlowTile - 1) / kFlowTile), dim3(64), kNsfFwdElems * sizeof(T), c->stream, g);
  });
}

void launch_nsf_inverse(mivi_ctx *c, const void *params, const void *Z, int n, void *logq) {
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    FlowArgs<T> g = flow_args<T>(c, params, n);
    g.Zin = (const T *)Z;
    g.logq = (T *)logq;
    hipLaunchKernelGGL((k_nsf_forward<T, true>), dim3((n + kFlowTile - 1) / kFlowTile), dim3(64), kNsfFwdElems * sizeof(T), c->stream, g);
  });
}

template <typename T>
void launch_nsf_vjp(mivi_ctx *c, const FlowArgs<T> &g, int n_slices, long long plen) {
  hipLaunchKernelGGL(k_nsf_vjp<T>, dim3(n_slices), dim3(64), kNsfVjpElems * sizeof(T), c->stream, g, plen);
}
template void launch_nsf_vjp<float>(mivi_ctx *, const FlowArgs<float> &, int, long long);
template void launch_nsf_vjp<double>(mivi_ctx *, const FlowArgs<double> &, int, long long);

}  // namespace mivi
