// The RealNVP normalizing-flow family (MIVI_REALNVP; include/mivi.h holds the definition): the kernels of one RepGradELBO estimate, of rand
// and of logpdf.  api_flow.hip drives them.
//
// One workgroup is ONE wave and works on tiles of 16 samples.  A tile's quantities live in LDS as [row][16] blocks (the sample is the fast
// axis), every block padded with zero rows to a multiple of 16, so that the three products of a net's layer are whole 16 x 16 x 4 matrix-core
// steps (Mfma16, device_common.h: f32 and f64 differ in the accumulator's lane map only):
//   forward     h_j = W_j h_{j-1}        A = W_j (global, zero outside the matrix),  B = h_{j-1}
//   input VJP   delta_{j-1} = W_j' delta A = W_j' (global),                          B = delta
//   weight VJP  dW_j = delta h_{j-1}'    A = delta, B = h_{j-1}', the K axis is the tile's 16 samples
//   k_flow_forward   draws (the mean-field Philox stream) -> x^0 ... x^L = z; saves every x^l (flow_X) and the f64 log q per sample
//   k_flow_inverse   z -> eps through the inverse layers, log q per point (mivi_logpdf)
//   k_flow_vjp       workgroup s owns the tiles s, s + n_slices, ...: [sticking the landing: u = grad_z log q by a sweep l = 1 .. L through
//                    the inverse layers, input VJPs only]  then the sweep l = L .. 1 with the nets recomputed from the saved x^{l-1} (the same
//                    code as the forward pass: bitwise the same activations); the parameter gradients of its tiles are summed, tile after
//                    tile, into the slice's own f64 partial vector -- no atomics
//   k_flow_finish    gradient = the slices' partials summed in slice order; value = mean[-ell + log q]
#include "flow_tile.h"

namespace mivi {

long long flow_params_len(const FlowArch &a) {
  long long n = 0;
  if (a.K) {   // the neural spline flow: one net per layer, 3K - 1 outputs per transformed coordinate
    for (int l = 1; l <= a.L; ++l) n += flow_net_len(a, a.d - flow_nA(a.d, l), flow_nA(a.d, l) * nsf_rows(a));
    return n;
  }
  for (int l = 1; l <= a.L; ++l) n += 2 * flow_net_len(a, a.d - flow_nA(a.d, l), flow_nA(a.d, l));
  return n;
}
int flow_slices(const FlowArch &a, int M) {
  const long long tiles = (M + kFlowTile - 1) / kFlowTile, by_mem = (1ll << 25) / flow_params_len(a);   // the partials stay under 256 MB
  long long ns = tiles < kFlowMaxSlices ? tiles : kFlowMaxSlices;
  if (ns > by_mem) ns = by_mem;
  return ns < 1 ? 1 : (int)ns;
}

__device__ __forceinline__ float flow_exp(float x) { return expf(x); }
__device__ __forceinline__ double flow_exp(double x) { return exp(x); }
__device__ __forceinline__ float flow_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double flow_tanh(double x) { return tanh(x); }
// where layer l's parameters start: the layers before it are l / 2 odd ones and (l - 1) / 2 even ones
__device__ __forceinline__ long long flow_layer_off(const FlowArch &a, int l) {
  const int nA1 = flow_nA(a.d, 1), nA2 = flow_nA(a.d, 2);
  return 2 * ((long long)(l / 2) * flow_net_len(a, a.d - nA1, nA1) + (long long)((l - 1) / 2) * flow_net_len(a, a.d - nA2, nA2));
}

// One net forward on a tile.  Hb[0] holds the input (zero rows up to a multiple of 16); leaves the hidden activations in Hb[1 .. H] and the
// output (tanh of it: is_s) in OUT, each with zero rows up to a multiple of 16.
template <typename T>
__device__ void flow_net_forward(const FlowArch &a, const T *np, int nin, int nout, bool is_s, T *Hb, T *OUT) {
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  int prev = nin;
  const T *p = np;
  for (int j = 0; j <= a.H; ++j) {
    const int out = j < a.H ? a.h[j] : nout;
    const T *Wm = p, *bv = p + (size_t)out * prev;
    const T *in = Hb + j * kFlowBlk;
    T *dst = j < a.H ? Hb + (j + 1) * kFlowBlk : OUT;
    for (int o0 = 0; o0 < out; o0 += 16) {
      typename Mfma16<T>::acc_t acc = {0, 0, 0, 0};
      const int o = o0 + col;
      for (int k0 = 0; k0 < prev; k0 += 4) {
        const int k = k0 + kq;
        const T av = (o < out && k < prev) ? Wm[o + (size_t)k * out] : T(0);
        acc = Mfma16<T>::mma(av, in[k * 16 + col], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = o0 + Mfma16<T>::row(kq, r);
        T v = T(0);
        if (row < out) {
          v = acc[r] + bv[row];
          if (j < a.H) v = v > T(0) ? v : T(0.01) * v;
          else if (is_s) v = flow_tanh(v);
        }
        dst[row * 16 + col] = v;
      }
    }
    __syncthreads();
    p = bv + out;
    prev = out;
  }
}

// One net backward on a tile.  D0 holds the cotangent of the output layer's pre-activation (zero rows up to a multiple of 16, zero columns
// for samples past M); Hb what flow_net_forward left.  Returns the block (D0 or D1) that holds the cotangent of the net's input.  PARAM:
// the tile's parameter gradient goes into `part` (the slice's partial at the net's offset): stored if `first`, added otherwise.
template <typename T, bool PARAM>
__device__ T *flow_net_backward(const FlowArch &a, const T *np, int nin, int nout, const T *Hb, T *D0, T *D1, double *part, bool first) {
  const int lane = threadIdx.x, col = lane & 15, kq = lane >> 4;
  long long off[4];
  int win[4], wout[4];
  {
    long long o = 0;
    int prev = nin;
    for (int j = 0; j <= a.H; ++j) {
      const int out = j < a.H ? a.h[j] : nout;
      off[j] = o; win[j] = prev; wout[j] = out;
      o += (long long)out * prev + out;
      prev = out;
    }
  }
  T *dcur = D0, *dnext = D1;
  for (int j = a.H; j >= 0; --j) {
    const int in_ = win[j], out = wout[j];
    const T *Wm = np + off[j];
    const T *hin = Hb + j * kFlowBlk;
    if (PARAM) {
      double *pW = part + off[j], *pb = pW + (size_t)out * in_;
      for (int o0 = 0; o0 < out; o0 += 16)
        for (int i0 = 0; i0 < in_; i0 += 16) {
          typename Mfma16<T>::acc_t acc = {0, 0, 0, 0};
#pragma unroll
          for (int k0 = 0; k0 < 16; k0 += 4) acc = Mfma16<T>::mma(dcur[(o0 + col) * 16 + k0 + kq], hin[(i0 + col) * 16 + k0 + kq], acc);
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int row = o0 + Mfma16<T>::row(kq, r), ci = i0 + col;
            if (row < out && ci < in_) {
              const size_t e = row + (size_t)ci * out;
              pW[e] = first ? (double)acc[r] : pW[e] + (double)acc[r];
            }
          }
        }
      for (int o = lane; o < out; o += 64) {
        double s = 0.0;
        for (int m = 0; m < 16; ++m) s += (double)dcur[o * 16 + m];
        pb[o] = first ? s : pb[o] + s;
      }
    }
    for (int i0 = 0; i0 < in_; i0 += 16) {
      typename Mfma16<T>::acc_t acc = {0, 0, 0, 0};
      const int i = i0 + col;
      for (int k0 = 0; k0 < out; k0 += 4) {
        const int k = k0 + kq;
        const T av = (i < in_ && k < out) ? Wm[k + (size_t)i * out] : T(0);
        acc = Mfma16<T>::mma(av, dcur[k * 16 + col], acc);
      }
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = i0 + Mfma16<T>::row(kq, r);
        T v = T(0);
        if (row < in_) {
          v = acc[r];
          if (j > 0) v *= hin[row * 16 + col] > T(0) ? T(1) : T(0.01);
        }
        dnext[row * 16 + col] = v;
      }
    }
    __syncthreads();
    T *t = dcur; dcur = dnext; dnext = t;
  }
  return dcur;
}

// LDS: XC [128][16] | H [4][64][16] | S [64][16] | TT [64][16]
constexpr int kFlowFwdElems = 128 * 16 + 6 * kFlowBlk;
template <typename T, bool INVERSE>
__global__ __launch_bounds__(64) void k_flow_forward(FlowArgs<T> g) {
  __shared__ double he[16], ss[16];
  T *XC = (T *)flow_lds, *Hb = XC + 128 * 16, *S = Hb + 4 * kFlowBlk, *TT = S + kFlowBlk;
  const FlowArch &a = g.a;
  const int d = a.d, lane = threadIdx.x, m0 = blockIdx.x * kFlowTile;
  const int n_ok = g.M - m0 < 16 ? g.M - m0 : 16;
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
    const int pa = (l & 1) ? 0 : 1, nA = flow_nA(d, l), nB = d - nA;
    flow_take_c(XC, Hb, nB, pa);
    const T *sp = g.params + flow_layer_off(a, l), *tp = sp + flow_net_len(a, nB, nA);
    flow_net_forward(a, sp, nB, nA, true, Hb, S);
    flow_net_forward(a, tp, nB, nA, false, Hb, TT);
    for (int e = lane; e < nA * 16; e += 64) {
      const int i = 2 * (e >> 4) + pa, m = e & 15;
      const T x = XC[i * 16 + m];
      XC[i * 16 + m] = INVERSE ? (x - TT[e]) * flow_exp(-S[e]) : x * flow_exp(S[e]) + TT[e];
    }
    if (lane < 16) {
      double s = 0.0;
      for (int j = 0; j < nA; ++j) s += (double)S[j * 16 + lane];
      ss[lane] += s;
    }
    __syncthreads();
    if (!INVERSE && g.X) flow_store_tile(g.X + ((size_t)l * g.capM + m0) * d, XC, d, 16);
  }
  if (!INVERSE && g.Z) flow_store_tile(g.Z + (size_t)m0 * d, XC, d, n_ok);
  // log q = -1/2 |eps|^2 - d/2 log 2 pi - sum_l 1' s_l (the forward pass summed |eps|^2 before the layers)
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

// LDS: H [4][64][16] | S | D0 | D1 | AV | G [128][16]
constexpr int kFlowVjpElems = 8 * kFlowBlk + 128 * 16;
template <typename T>
__global__ __launch_bounds__(64) void k_flow_vjp(FlowArgs<T> g, long long plen) {
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
      for (int l = 1; l <= a.L; ++l) {
        const int pa = (l & 1) ? 0 : 1, nA = flow_nA(d, l), nB = d - nA;
        const T *xp = g.X + ((size_t)(l - 1) * g.capM + m0) * d;
        for (int e = lane; e < round16(nB) * 16; e += 64) {
          const int j = e >> 4, m = e & 15;
          Hb[e] = j < nB ? xp[(size_t)m * d + 2 * j + 1 - pa] : T(0);
        }
        for (int e = lane; e < nA * 16; e += 64) AV[e] = xp[(size_t)(e & 15) * d + 2 * (e >> 4) + pa];
        __syncthreads();
        const T *sp = g.params + flow_layer_off(a, l), *tp = sp + flow_net_len(a, nB, nA);
        flow_net_forward(a, sp, nB, nA, true, Hb, S);
        for (int e = lane; e < round16(nA) * 16; e += 64) {
          const int j = e >> 4, m = e & 15;
          T v = T(0);
          if (j < nA) {
            const T s = S[e];
            v = (-G[(2 * j + pa) * 16 + m] * AV[e] - T(1)) * (T(1) - s * s);
            AV[e] = flow_exp(-s);
          }
          D0[e] = v;
        }
        __syncthreads();
        const T *dc = flow_net_backward<T, false>(a, sp, nB, nA, Hb, D0, D1, nullptr, false);
        for (int e = lane; e < nB * 16; e += 64) G[(2 * (e >> 4) + 1 - pa) * 16 + (e & 15)] += dc[e];
        __syncthreads();
        flow_net_forward(a, tp, nB, nA, false, Hb, S);
        for (int e = lane; e < round16(nA) * 16; e += 64) {
          const int j = e >> 4, m = e & 15;
          D0[e] = j < nA ? -G[(2 * j + pa) * 16 + m] * AV[e] : T(0);
        }
        __syncthreads();
        dc = flow_net_backward<T, false>(a, tp, nB, nA, Hb, D0, D1, nullptr, false);
        for (int e = lane; e < nB * 16; e += 64) G[(2 * (e >> 4) + 1 - pa) * 16 + (e & 15)] += dc[e];
        for (int e = lane; e < nA * 16; e += 64) G[(2 * (e >> 4) + pa) * 16 + (e & 15)] *= AV[e];
        __syncthreads();
      }
      for (int e = lane; e < 16 * d; e += 64) {
        const int m = e / d, i = e - m * d;
        G[i * 16 + m] = m < n_ok ? (T)((-g.Wg[(size_t)(m0 + m) * d + i] + G[i * 16 + m]) * (T)g.invM) : T(0);
      }
      __syncthreads();
    } else {
      flow_load_tile(g.Wg + (size_t)m0 * d, G, d, n_ok, (T)(-g.invM));
    }
    const T kappa = g.kind == MIVI_ENT_STL ? T(0) : (T)(-g.invM);
    for (int l = a.L; l >= 1; --l) {
      const int pa = (l & 1) ? 0 : 1, nA = flow_nA(d, l), nB = d - nA;
      const T *xp = g.X + ((size_t)(l - 1) * g.capM + m0) * d;
      for (int e = lane; e < round16(nB) * 16; e += 64) {
        const int j = e >> 4, m = e & 15;
        Hb[e] = j < nB ? xp[(size_t)m * d + 2 * j + 1 - pa] : T(0);
      }
      for (int e = lane; e < nA * 16; e += 64) AV[e] = xp[(size_t)(e & 15) * d + 2 * (e >> 4) + pa];
      __syncthreads();
      const long long loff = flow_layer_off(a, l), nlen = flow_net_len(a, nB, nA);
      const T *sp = g.params + loff, *tp = sp + nlen;
      flow_net_forward(a, sp, nB, nA, true, Hb, S);
      for (int e = lane; e < round16(nA) * 16; e += 64) {
        const int j = e >> 4, m = e & 15;
        T v = T(0);
        if (j < nA) {
          const T s = S[e], es = flow_exp(s);
          v = (G[(2 * j + pa) * 16 + m] * AV[e] * es + (m < n_ok ? kappa : T(0))) * (T(1) - s * s);
          AV[e] = es;
        }
        D0[e] = v;
      }
      __syncthreads();
      const T *dc = flow_net_backward<T, true>(a, sp, nB, nA, Hb, D0, D1, part + loff, first);
      for (int e = lane; e < nB * 16; e += 64) G[(2 * (e >> 4) + 1 - pa) * 16 + (e & 15)] += dc[e];
      __syncthreads();
      flow_net_forward(a, tp, nB, nA, false, Hb, S);
      for (int e = lane; e < round16(nA) * 16; e += 64) {
        const int j = e >> 4, m = e & 15;
        D0[e] = j < nA ? G[(2 * j + pa) * 16 + m] : T(0);
      }
      __syncthreads();
      dc = flow_net_backward<T, true>(a, tp, nB, nA, Hb, D0, D1, part + loff + nlen, first);
      for (int e = lane; e < nB * 16; e += 64) G[(2 * (e >> 4) + 1 - pa) * 16 + (e & 15)] += dc[e];
      for (int e = lane; e < nA * 16; e += 64) G[(2 * (e >> 4) + pa) * 16 + (e & 15)] *= AV[e];
      __syncthreads();
    }
  }
}

// the gradient: the slices' partials in slice order; the last workgroup: value = -(sum ell / M) + mean log q
template <typename T>
__global__ __launch_bounds__(256) void k_flow_finish(long long plen, int n_slices, int n_grad_blocks, const double *__restrict__ part,
                                                   const double *__restrict__ lq, ValueIn vin, OutArgs out) {
  __shared__ double red[2 * 4];
  const int tid = threadIdx.x;
  if ((int)blockIdx.x < n_grad_blocks) {
    const long long t = (long long)blockIdx.x * 256 + tid;
    if (t >= plen) return;
    double s = 0.0;
    for (int k = 0; k < n_slices; ++k) s += part[(size_t)k * plen + t];
    ((T *)out.grad)[t] = (T)s;
    return;
  }
  double s_ell = 0.0, s_lq = 0.0;
  for (int i = tid; i < vin.n_ell_part; i += 256) s_ell += vin.ell_part[i];
  for (int i = tid; i < vin.n_ell; i += 256) s_ell += (double)((const T *)vin.ell)[i];
  for (int i = tid; i < out.M_local; i += 256) s_lq += lq[i];
  double v[2] = {s_ell, s_lq};
  block_sum_n<double, 256, 2>(v, red);
  if (tid == 0) {
    const double Mt = (double)out.M_total;
    const double value = -(v[0] + (double)out.M_local * vin.ell_const) / Mt + v[1] / Mt;
    *(T *)out.value = (T)value;
    if (!isfinite(value) && out.status) atomicOr(out.status, 1);
    if (out.elbo_rec) out.elbo_rec[out.rec_slot] = -value;
  }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------------
bool flow_prepare(mivi_ctx *c) {
  if (c->flow.K) return nsf_prepare(c);
  return by_dtype(c, [&](auto t) {
    using T = decltype(t);
    return flow_lds_attr<T>(&k_flow_forward<T, false>, kFlowFwdElems) && flow_lds_attr<T>(&k_flow_forward<T, true>, kFlowFwdElems) &&
           flow_lds_attr<T>(&k_flow_vjp<T>, kFlowVjpElems);
  });
}

void launch_flow_forward(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *Z, void *eps, bool save) {
  if (c->flow.K) return launch_nsf_forward(c, params, rng, M, Z, eps, save);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    FlowArgs<T> g = flow_args<T>(c, params, M);
    g.rng = rng;
    if (save && (c->cap_M % kFlowTile != 0 || M > c->cap_M)) return;   // (never: ensure_work's rounding; a partial last tile would write past its plane)
    g.X = save ? (T *)c->flow_X.p : nullptr;
    g.Z = (T *)Z;
    g.eps = (T *)eps;
    g.lq = save ? (double *)c->flow_lq.p : nullptr;
    hipLaunchKernelGGL((k_flow_forward<T, false>), dim3((M + kFlowTile - 1) / kFlowTile), dim3(64), kFlowFwdElems * sizeof(T), c->stream, g);
  });
}

void launch_flow_inverse(mivi_ctx *c, const void *params, const void *Z, int n, void *logq) {
  if (c->flow.K) return launch_nsf_inverse(c, params, Z, n, logq);
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    FlowArgs<T> g = flow_args<T>(c, params, n);
    g.Zin = (const T *)Z;
    g.logq = (T *)logq;
    hipLaunchKernelGGL((k_flow_forward<T, true>), dim3((n + kFlowTile - 1) / kFlowTile), dim3(64), kFlowFwdElems * sizeof(T), c->stream, g);
  });
}

void launch_flow_vjp_finish(mivi_ctx *c, const void *params, int M, int want_grad, const ValueIn &vin, const OutArgs &out) {
  const long long plen = flow_params_len(c->flow);
  const int ns = flow_slices(c->flow, M), ngb = want_grad ? (int)((plen + 255) / 256) : 0;
  by_dtype(c, [&](auto t) {
    using T = decltype(t);
    if (want_grad) {
      FlowArgs<T> g = flow_args<T>(c, params, M);
      g.X = (T *)c->flow_X.p;
      g.Wg = (const T *)c->W.p;
      g.part = (double *)c->flow_part.p;
      g.kind = out.ent_kind;
      g.invM = 1.0 / (double)out.M_total;
      if (c->flow.K) launch_nsf_vjp<T>(c, g, ns, plen);
      else hipLaunchKernelGGL(k_flow_vjp<T>, dim3(ns), dim3(64), kFlowVjpElems * sizeof(T), c->stream, g, plen);
    }
    hipLaunchKernelGGL(k_flow_finish<T>, dim3(ngb + 1), dim3(256), 0, c->stream, plen, ns, ngb, (const double *)c->flow_part.p, (const double *)c->flow_lq.p, vin, out);
  });
}

}  // namespace mivi
