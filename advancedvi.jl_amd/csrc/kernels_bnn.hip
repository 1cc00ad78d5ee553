// The Bayesian neural network target (include/mivi.h, mivi_set_target_bnn): theta = [vec W_1; b_1; ...; vec W_{H+1}; b_{H+1}] per sample
// column of Z -- every Monte-Carlo sample is a DIFFERENT network, so the work is M independent small MLP forward and backward passes over
// the same rows, each returning its own parameter gradient.  api_bnn.hip sets the target; eval_generic_target reaches launch_bnn_target.
//
//   k_bnn_rows     grid (sample of the chunk, row slice), 256 threads.  The workgroup stages ITS network into LDS once -- the hidden
//                  layers' weights as [in][out + 1] planes with every width padded to a multiple of 16 by zero rows and columns, the
//                  biases, the output row -- and walks its slice of the rows in tiles of 16 (through the row index vector, if a selection
//                  is set).  A tile's activations are [width][16] blocks (stride 17: both operand orders of a block read 64 banks).
//                  Every hidden product runs on the 16 x 16 x 4 matrix-core form of the element type (Mfma16): forward W_l (A) times
//                  a_{l-1} (B), wave w owning output rows 16 w ..; the output row as an A operand whose rows 1 .. 15 are zero; backward
//                  W_l' (A, the same plane read the other way) times delta_l (B); dW_l += delta_l a_{l-1}' with the tile's 16 rows as
//                  the K axis, its at most 48 output tiles dealt round-robin to the four waves and kept in registers across the slice.
//                  f, softplus, the residual and the log-likelihood terms are f64; tanh' comes from the saved a_l.  The f32 accumulators
//                  are flushed into the slice's f64 partial every kBnnFlush rows; bias and output-row gradients are f64 sums per thread.
//   k_bnn_finish   one workgroup per sample: the slices in slice order, likeadj, the prior, the Normal likelihood's constants -- all
//                  f64, rounded once into ell (M) and G (d x M) where eval_generic_target leaves them for the other generic targets.
//   k_bnn_forward  the same forward sweep on new rows, storing f (mivi_bnn_forward).
//   k_bnn_rows_head, k_bnn_forward_head   the same two for a network with n_out = 2 .. 64 outputs (a categorical likelihood with a softmax
//                  link, or independent Normals).  The output layer is then one more [in][out + 1] plane, padded to Pc = round16(n_out)
//                  like the hidden ones, and layer H + 1 of every sweep: the logits W_{H+1} a_H + b on the matrix cores (wave w owns output
//                  tile w) into one of the two delta blocks; the likelihood in f64 -- wave w takes tile rows 4 w .. 4 w + 3 with 16 lanes
//                  per row striding over the REAL classes, the row maximum and sum of exponentials by 16-lane shuffles, the label only ever
//                  COMPARED with the class index -- which overwrites the logits by delta_out in place; then dW_out += delta_out a_H' (its
//                  at most 16 tiles join the round-robin deal: up to 64 tiles, kBnnHeadWaveTiles = 16 per wave, in registers across the
//                  slice), db_out and delta_H = (W_out' delta_out)(1 - a_H^2) by the code of the hidden layers.
// Nothing is accumulated atomically and no geometry depends on the chunking of the samples: results are bitwise reproducible and the
// same for every partial cap.
#include "flow_tile.h"

namespace mivi {

constexpr int kBnnLda = kFlowTile + 1;   // stride of a [width][16] activation block
constexpr int kBnnFlush = 128;           // rows between two flushes of the f32 dW accumulators into the f64 partial
constexpr int kBnnWaveTiles = 12;        // dW output tiles per wave: 3 layers x 16 tiles over 4 waves
constexpr int kBnnHeadWaveTiles = 16;    // ... of the head kernel: the output layer's 16 tiles more
constexpr long long kBnnSliceRows = 256; // rows a slice aims at (slices: ceil(rows / 256) clamped to 1 .. 32)

// layer l = 1 .. H + 1 maps n[l - 1] -> n[l]; P: the hidden-side widths padded to 16.  Offsets into theta (woff, boff) and into LDS
struct BnnNet {
  int H, d;
  int n[5], P[5];            // (P[H + 1] = Pc, the padded width of the head: set when n[H + 1] >= 2 only)
  int woff[4], boff[4];      // theta: W_l, b_l at index l - 1
  int lw[4], lb[4], lwo;     // LDS: W_l ([P[l-1]][P[l] + 1]), b_l of the hidden layers (and of the head), the output row (P[H]; one output)
  int la[4], ldl[2];         // LDS: a_0 .. a_H, the two delta blocks
  int toff[5];               // dW tiles of layer l: [toff[l - 1], toff[l]) (the hidden layers; the head as layer H + 1)
  int lds_elems;
};

template <typename T>
struct BnnArgs {
  BnnNet net;
  int M, m0;                 // samples of this chunk; the chunk's first sample column in Z / ell / G
  long long n, nr;           // X's leading dimension; rows evaluated
  const T *X, *y;
  const long long *rows;     // the row selection (nr entries) or nullptr: rows 0 .. nr - 1
  const T *Z;                // d x M_total, ld d
  double *part;              // [n_sl][M][d]
  double *llp;               // [n_sl][M]
  int n_sl;
  long long rps;             // rows per slice, a multiple of 16
  T *G, *ell;                // d x M_total; M_total
  T *f;                      // k_bnn_forward: nr x M; k_bnn_forward_head: n_out x nr x M
  int likelihood, want_grad;
  double noise, prior_std, likeadj;
};

__device__ __forceinline__ float bnn_tanh(float x) { return tanhf(x); }
__device__ __forceinline__ double bnn_tanh(double x) { return tanh(x); }

// layers 1 .. nl as zero-padded planes and biases (no barrier)
template <typename T>
__device__ __forceinline__ void bnn_stage_planes(const BnnNet &nt, const T *th, T *S, int nl) {
  const int tid = threadIdx.x;
  for (int l = 1; l <= nl; ++l) {
    const int no = nt.n[l], ni = nt.n[l - 1], ldw = nt.P[l] + 1;
    T *W = S + nt.lw[l - 1], *b = S + nt.lb[l - 1];
    for (int e = tid; e < nt.P[l - 1] * ldw; e += 256) {
      const int i = e / ldw, o = e - i * ldw;
      W[e] = (o < no && i < ni) ? th[nt.woff[l - 1] + o + no * i] : T(0);
    }
    for (int e = tid; e < nt.P[l]; e += 256) b[e] = e < no ? th[nt.boff[l - 1] + e] : T(0);
  }
}

template <typename T>
__device__ __forceinline__ void bnn_stage_net(const BnnNet &nt, const T *th, T *S) {
  const int tid = threadIdx.x;
  bnn_stage_planes(nt, th, S, nt.H);
  for (int e = tid; e < nt.P[nt.H]; e += 256) S[nt.lwo + e] = e < nt.n[nt.H] ? th[nt.woff[nt.H] + e] : T(0);
  __syncthreads();
}

// the 16 rows at rr of the slice ending at rend -> rowi (or -1) and a_0 (zero rows up to P[0], zero columns past the slice)
template <typename T>
__device__ __forceinline__ void bnn_load_x(const BnnArgs<T> &a, T *S, long long *rowi, long long rr, long long rend) {
  const int tid = threadIdx.x;
  if (tid < kFlowTile) rowi[tid] = rr + tid < rend ? (a.rows ? a.rows[rr + tid] : rr + tid) : -1;
  __syncthreads();
  T *a0 = S + a.net.la[0];
  for (int e = tid; e < a.net.P[0] * kFlowTile; e += 256) {
    const int r = e & 15, k = e >> 4;
    const long long ri = rowi[r];
    a0[k * kBnnLda + r] = (ri >= 0 && k < a.net.n[0]) ? a.X[ri + (long long)k * a.n] : T(0);
  }
  __syncthreads();
}

// a_0 -> a_1 .. a_H in LDS
template <typename T>
__device__ __forceinline__ void bnn_hidden_tile(const BnnNet &nt, T *S) {
  using acc_t = typename Mfma16<T>::acc_t;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  for (int l = 1; l <= nt.H; ++l) {
    const T *W = S + nt.lw[l - 1], *b = S + nt.lb[l - 1], *ain = S + nt.la[l - 1];
    T *aout = S + nt.la[l];
    const int ldw = nt.P[l] + 1, K = nt.P[l - 1];
    for (int ot = w; ot < nt.P[l] / 16; ot += 4) {
      acc_t acc = acc_t{0, 0, 0, 0};
      for (int kk = 0; kk < K; kk += 4) acc = Mfma16<T>::mma(W[(kk + kq) * ldw + 16 * ot + col], ain[(kk + kq) * kBnnLda + col], acc);
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 16 * ot + Mfma16<T>::row(kq, r);
        aout[row * kBnnLda + col] = bnn_tanh(acc[r] + b[row]);   // (a padded row has zero weights and bias: tanh(0) = 0)
      }
    }
    __syncthreads();
  }
}

// a_0 -> a_1 .. a_H in LDS; f of tile row `tid` in threads 0 .. 15 (f64, the output bias added), 0 elsewhere
template <typename T>
__device__ __forceinline__ double bnn_forward_tile(const BnnNet &nt, T *S, double bout) {
  using acc_t = typename Mfma16<T>::acc_t;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  bnn_hidden_tile(nt, S);
  double f = 0.0;
  if (w == 0) {   // the output row as a 16-row A operand whose rows 1 .. 15 are zero: C[0][col] is register 0 of lanes 0 .. 15
    const T *wo = S + nt.lwo, *aH = S + nt.la[nt.H];
    acc_t acc = acc_t{0, 0, 0, 0};
    for (int kk = 0; kk < nt.P[nt.H]; kk += 4) acc = Mfma16<T>::mma(col == 0 ? wo[kk + kq] : T(0), aH[(kk + kq) * kBnnLda + col], acc);
    if (kq == 0) f = (double)acc[0] + bout;
  }
  return f;
}

// the wave's dW tiles of layers 1 .. nl -> the slice's f64 partial (added to it after the first flush); the accumulators restart at zero
template <typename T, int NT>
__device__ __forceinline__ void bnn_flush(const BnnNet &nt, typename Mfma16<T>::acc_t (&acc)[NT], double *part, bool add, int nl) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
#pragma unroll
  for (int t = 0; t < NT; ++t) {
    int g = w + 4 * t;
    if (g < nt.toff[nl]) {
      int l = 1;
      while (g >= nt.toff[l]) ++l;
      g -= nt.toff[l - 1];
      const int itn = nt.P[l - 1] / 16, ot = g / itn, it = g - ot * itn, i = 16 * it + col;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o = 16 * ot + Mfma16<T>::row(kq, r);
        if (o < nt.n[l] && i < nt.n[l - 1]) {
          double *dst = part + nt.woff[l - 1] + o + nt.n[l] * i;
          *dst = add ? *dst + (double)acc[t][r] : (double)acc[t][r];
        }
        acc[t][r] = T(0);
      }
    }
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bnn_rows(BnnArgs<T> a) {
  using acc_t = typename Mfma16<T>::acc_t;
  T *S = reinterpret_cast<T *>(flow_lds);
  __shared__ long long rowi[kFlowTile];
  __shared__ T res[kFlowTile];
  const BnnNet &nt = a.net;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, kq = lane >> 4;
  const int ml = blockIdx.x, sl = blockIdx.y;
  const T *th = a.Z + (size_t)(a.m0 + ml) * nt.d;
  bnn_stage_net(nt, th, S);
  const double bout = (double)th[nt.d - 1], in2 = 1.0 / (a.noise * a.noise);
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  double *part = a.part + ((size_t)sl * a.M + ml) * nt.d;
  acc_t acc[kBnnWaveTiles];
#pragma unroll
  for (int t = 0; t < kBnnWaveTiles; ++t) acc[t] = acc_t{0, 0, 0, 0};
  double gb[3] = {0.0, 0.0, 0.0}, gwo = 0.0, gbo = 0.0, ll = 0.0;
  bool flushed = false;
  int since = 0;
  const T *wo = S + nt.lwo, *aH = S + nt.la[nt.H];
  for (long long rr = rbeg; rr < rend; rr += kFlowTile) {
    bnn_load_x(a, S, rowi, rr, rend);
    const double f = bnn_forward_tile(nt, S, bout);
    if (tid < kFlowTile) {   // the likelihood of tile row tid, in f64
      double rs = 0.0;
      if (rowi[tid] >= 0) {
        const double y = (double)a.y[rowi[tid]];
        if (a.likelihood == 0) {
          const double e = exp(-fabs(f));
          ll += y * f - (fmax(f, 0.0) + log1p(e));
          rs = y - (f >= 0.0 ? 1.0 : e) / (1.0 + e);
        } else {
          const double u = y - f;
          ll -= 0.5 * u * u * in2;
          rs = u * in2;
        }
      }
      gbo += rs;
      res[tid] = (T)rs;
    }
    if (!a.want_grad) continue;
    __syncthreads();
    T *D = S + nt.ldl[0], *Dn = S + nt.ldl[1];
    if (tid < nt.P[nt.H]) {   // the output row's gradient; delta_H = w_out res (1 - a_H^2)
      double s = 0.0;
#pragma unroll
      for (int r = 0; r < kFlowTile; ++r) s += (double)aH[tid * kBnnLda + r] * (double)res[r];
      gwo += s;
    }
    for (int e = tid; e < nt.P[nt.H] * kFlowTile; e += 256) {
      const int j = e >> 4, r = e & 15;
      const T av = aH[j * kBnnLda + r];
      D[j * kBnnLda + r] = wo[j] * res[r] * (T(1) - av * av);
    }
    __syncthreads();
#pragma unroll
    for (int l = 3; l >= 1; --l) {
      if (l <= nt.H) {
        const T *ain = S + nt.la[l - 1];
        if (tid < nt.P[l]) {   // db_l: the row sums of delta_l
          double s = 0.0;
#pragma unroll
          for (int r = 0; r < kFlowTile; ++r) s += (double)D[tid * kBnnLda + r];
          gb[l - 1] += s;
        }
        const int t0 = nt.toff[l - 1], tn = nt.toff[l] - t0, itn = nt.P[l - 1] / 16;
#pragma unroll
        for (int t = 0; t < kBnnWaveTiles; ++t) {   // dW_l += delta_l a_{l-1}': K is the tile's 16 rows
          const int g = w + 4 * t - t0;
          if (g >= 0 && g < tn) {
            const int ot = g / itn, it = g - ot * itn;
#pragma unroll
            for (int kk = 0; kk < kFlowTile; kk += 4)
              acc[t] = Mfma16<T>::mma(D[(16 * ot + col) * kBnnLda + kk + kq], ain[(16 * it + col) * kBnnLda + kk + kq], acc[t]);
          }
        }
        if (l > 1) {   // delta_{l-1} = (W_l' delta_l) (1 - a_{l-1}^2), from the saved activations
          const T *W = S + nt.lw[l - 1];
          const int ldw = nt.P[l] + 1;
          for (int it = w; it < itn; it += 4) {
            acc_t c = acc_t{0, 0, 0, 0};
            for (int kk = 0; kk < nt.P[l]; kk += 4) c = Mfma16<T>::mma(W[(16 * it + col) * ldw + kk + kq], D[(kk + kq) * kBnnLda + col], c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = 16 * it + Mfma16<T>::row(kq, r);
              const T av = ain[i * kBnnLda + col];
              Dn[i * kBnnLda + col] = c[r] * (T(1) - av * av);
            }
          }
        }
        __syncthreads();
        T *sw = D;
        D = Dn;
        Dn = sw;
      }
    }
    if constexpr (sizeof(T) == 4) {
      since += kFlowTile;
      if (since >= kBnnFlush) {
        bnn_flush<T>(nt, acc, part, flushed, nt.H);
        flushed = true;
        since = 0;
      }
    }
  }
  ll = wave_sum(ll);     // (threads 0 .. 15 of wave 0 hold the terms)
  gbo = wave_sum(gbo);
  if (tid == 0) a.llp[(size_t)sl * a.M + ml] = ll;
  if (!a.want_grad) return;
  bnn_flush<T>(nt, acc, part, flushed, nt.H);
#pragma unroll
  for (int l = 1; l <= 3; ++l)
    if (l <= nt.H && tid < nt.n[l]) part[nt.boff[l - 1] + tid] = gb[l - 1];
  if (tid < nt.n[nt.H]) part[nt.woff[nt.H] + tid] = gwo;
  if (tid == 0) part[nt.d - 1] = gbo;
}

template <typename T>
__global__ __launch_bounds__(256) void k_bnn_forward(BnnArgs<T> a) {
  T *S = reinterpret_cast<T *>(flow_lds);
  __shared__ long long rowi[kFlowTile];
  const BnnNet &nt = a.net;
  const int tid = threadIdx.x, m = blockIdx.x, sl = blockIdx.y;
  const T *th = a.Z + (size_t)m * nt.d;
  bnn_stage_net(nt, th, S);
  const double bout = (double)th[nt.d - 1];
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  for (long long rr = rbeg; rr < rend; rr += kFlowTile) {
    bnn_load_x(a, S, rowi, rr, rend);
    const double f = bnn_forward_tile(nt, S, bout);
    if (tid < kFlowTile && rowi[tid] >= 0) a.f[rr + tid + a.nr * (long long)m] = (T)f;
  }
}

// ---- the multi-output head (n_out >= 2): layer H + 1 is a plane like the hidden ones -------------------------------------------------------
// logits = W_{H+1} a_H + b_{H+1} of the tile -> the [Pc][16] block L (a padded class: 0); wave w owns output tile w
template <typename T>
__device__ __forceinline__ void bnn_head_logits(const BnnNet &nt, T *S, T *L) {
  using acc_t = typename Mfma16<T>::acc_t;
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, col = lane & 15, kq = lane >> 4;
  const T *W = S + nt.lw[nt.H], *b = S + nt.lb[nt.H], *aH = S + nt.la[nt.H];
  const int ldw = nt.P[nt.H + 1] + 1, K = nt.P[nt.H];
  for (int ot = w; ot < nt.P[nt.H + 1] / 16; ot += 4) {
    acc_t acc = acc_t{0, 0, 0, 0};
    for (int kk = 0; kk < K; kk += 4) acc = Mfma16<T>::mma(W[(kk + kq) * ldw + 16 * ot + col], aH[(kk + kq) * kBnnLda + col], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = 16 * ot + Mfma16<T>::row(kq, r);
      L[row * kBnnLda + col] = acc[r] + b[row];
    }
  }
  __syncthreads();
}

// The likelihood of the tile in f64: the logits in L are overwritten by delta_out (0 in rows past the slice and in padded classes); returns
// this lane's log-likelihood terms.  Wave w takes tile rows 4 w .. 4 w + 3, 16 lanes per row, the lanes striding over the classes: the
// maximum and the sum of exponentials of a row are over its n_out REAL classes.  The label is compared with the class index and never
// used as one, so a label outside 0 .. n_out - 1 (device-resident data are not checked) matches no class and addresses nothing.
template <typename T>
__device__ __forceinline__ double bnn_head_delta(const BnnArgs<T> &a, T *L, const long long *rowi, double in2) {
  const int lane = threadIdx.x & 63, c0 = lane & 15, r = 4 * (threadIdx.x >> 6) + (lane >> 4);
  const int C = a.net.n[a.net.H + 1], Pc = a.net.P[a.net.H + 1];
  const long long ri = rowi[r];
  double ll = 0.0;
  if (a.likelihood == 0) {
    double mx = -INFINITY, se = 0.0;
    for (int c = c0; c < C; c += 16) mx = fmax(mx, (double)L[c * kBnnLda + r]);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o, 16));
    for (int c = c0; c < C; c += 16) se += exp((double)L[c * kBnnLda + r] - mx);
#pragma unroll
    for (int o = 8; o > 0; o >>= 1) se += __shfl_xor(se, o, 16);
    const double lse = mx + log(se), yv = ri >= 0 ? (double)a.y[ri] : -1.0;
    for (int c = c0; c < Pc; c += 16) {
      double dl = 0.0;
      if (ri >= 0 && c < C) {
        const double lg = (double)L[c * kBnnLda + r];
        const bool hit = (double)c == yv;
        if (hit) ll += lg - lse;
        dl = (hit ? 1.0 : 0.0) - exp(lg - lse);
      }
      L[c * kBnnLda + r] = (T)dl;
    }
  } else {
    for (int c = c0; c < Pc; c += 16) {
      double dl = 0.0;
      if (ri >= 0 && c < C) {
        const double u = (double)a.y[ri + a.n * (long long)c] - (double)L[c * kBnnLda + r];
        ll -= 0.5 * u * u * in2;
        dl = u * in2;
      }
      L[c * kBnnLda + r] = (T)dl;
    }
  }
  __syncthreads();
  return ll;
}

template <typename T>
__global__ __launch_bounds__(256) void k_bnn_rows_head(BnnArgs<T> a) {
  using acc_t = typename Mfma16<T>::acc_t;
  T *S = reinterpret_cast<T *>(flow_lds);
  __shared__ long long rowi[kFlowTile];
  __shared__ double red[4];
  const BnnNet &nt = a.net;
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 15, kq = lane >> 4;
  const int ml = blockIdx.x, sl = blockIdx.y, nl = nt.H + 1;
  const T *th = a.Z + (size_t)(a.m0 + ml) * nt.d;
  bnn_stage_planes(nt, th, S, nl);
  __syncthreads();
  const double in2 = 1.0 / (a.noise * a.noise);
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  double *part = a.part + ((size_t)sl * a.M + ml) * nt.d;
  acc_t acc[kBnnHeadWaveTiles];
#pragma unroll
  for (int t = 0; t < kBnnHeadWaveTiles; ++t) acc[t] = acc_t{0, 0, 0, 0};
  double gb[4] = {0.0, 0.0, 0.0, 0.0}, ll = 0.0;
  bool flushed = false;
  int since = 0;
  for (long long rr = rbeg; rr < rend; rr += kFlowTile) {
    bnn_load_x(a, S, rowi, rr, rend);
    bnn_hidden_tile(nt, S);
    T *D = S + nt.ldl[0], *Dn = S + nt.ldl[1];
    bnn_head_logits(nt, S, D);
    ll += bnn_head_delta(a, D, rowi, in2);
    if (!a.want_grad) continue;
#pragma unroll
    for (int l = 4; l >= 1; --l) {   // the head is layer H + 1 of the sweep
      if (l <= nl) {
        const T *ain = S + nt.la[l - 1];
        if (tid < nt.P[l]) {   // db_l: the row sums of delta_l
          double s = 0.0;
#pragma unroll
          for (int r = 0; r < kFlowTile; ++r) s += (double)D[tid * kBnnLda + r];
          gb[l - 1] += s;
        }
        const int t0 = nt.toff[l - 1], tn = nt.toff[l] - t0, itn = nt.P[l - 1] / 16;
#pragma unroll
        for (int t = 0; t < kBnnHeadWaveTiles; ++t) {   // dW_l += delta_l a_{l-1}': K is the tile's 16 rows
          const int g = w + 4 * t - t0;
          if (g >= 0 && g < tn) {
            const int ot = g / itn, it = g - ot * itn;
#pragma unroll
            for (int kk = 0; kk < kFlowTile; kk += 4)
              acc[t] = Mfma16<T>::mma(D[(16 * ot + col) * kBnnLda + kk + kq], ain[(16 * it + col) * kBnnLda + kk + kq], acc[t]);
          }
        }
        if (l > 1) {   // delta_{l-1} = (W_l' delta_l) (1 - a_{l-1}^2), from the saved activations
          const T *W = S + nt.lw[l - 1];
          const int ldw = nt.P[l] + 1;
          for (int it = w; it < itn; it += 4) {
            acc_t c = acc_t{0, 0, 0, 0};
            for (int kk = 0; kk < nt.P[l]; kk += 4) c = Mfma16<T>::mma(W[(16 * it + col) * ldw + kk + kq], D[(kk + kq) * kBnnLda + col], c);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int i = 16 * it + Mfma16<T>::row(kq, r);
              const T av = ain[i * kBnnLda + col];
              Dn[i * kBnnLda + col] = c[r] * (T(1) - av * av);
            }
          }
        }
        __syncthreads();
        T *sw = D;
        D = Dn;
        Dn = sw;
      }
    }
    if constexpr (sizeof(T) == 4) {
      since += kFlowTile;
      if (since >= kBnnFlush) {
        bnn_flush<T>(nt, acc, part, flushed, nl);
        flushed = true;
        since = 0;
      }
    }
  }
  ll = block_sum<double, 256>(ll, red);
  if (tid == 0) a.llp[(size_t)sl * a.M + ml] = ll;
  if (!a.want_grad) return;
  bnn_flush<T>(nt, acc, part, flushed, nl);
#pragma unroll
  for (int l = 1; l <= 4; ++l)
    if (l <= nl && tid < nt.n[l]) part[nt.boff[l - 1] + tid] = gb[l - 1];
}

template <typename T>
__global__ __launch_bounds__(256) void k_bnn_forward_head(BnnArgs<T> a) {
  T *S = reinterpret_cast<T *>(flow_lds);
  __shared__ long long rowi[kFlowTile];
  const BnnNet &nt = a.net;
  const int tid = threadIdx.x, m = blockIdx.x, sl = blockIdx.y, C = nt.n[nt.H + 1];
  bnn_stage_planes(nt, a.Z + (size_t)m * nt.d, S, nt.H + 1);
  __syncthreads();
  T *L = S + nt.ldl[0];
  const long long rbeg = (long long)sl * a.rps, rend = rbeg + a.rps < a.nr ? rbeg + a.rps : a.nr;
  for (long long rr = rbeg; rr < rend; rr += kFlowTile) {
    bnn_load_x(a, S, rowi, rr, rend);
    bnn_hidden_tile(nt, S);
    bnn_head_logits(nt, S, L);
    for (int e = tid; e < C * kFlowTile; e += 256) {
      const int r = e / C, c = e - r * C;
      if (rowi[r] >= 0) a.f[c + (long long)C * (rr + r + a.nr * (long long)m)] = L[c * kBnnLda + r];
    }
    __syncthreads();   // (the next tile's bnn_load_x writes rowi)
  }
}

template <typename T>
__global__ __launch_bounds__(256) void k_bnn_finish(BnnArgs<T> a) {
  __shared__ double red[4];
  const int tid = threadIdx.x, ml = blockIdx.x, d = a.net.d;
  const T *z = a.Z + (size_t)(a.m0 + ml) * d;
  const double ip2 = 1.0 / (a.prior_std * a.prior_std);
  double tt = 0.0;
  for (int i = tid; i < d; i += 256) {
    const double zi = (double)z[i];
    tt += zi * zi;
    if (a.want_grad) {
      double x = 0.0;
      for (int sl = 0; sl < a.n_sl; ++sl) x += a.part[((size_t)sl * a.M + ml) * d + i];
      a.G[(size_t)(a.m0 + ml) * d + i] = (T)(a.likeadj * x - zi * ip2);
    }
  }
  tt = block_sum<double, 256>(tt, red);
  if (tid == 0) {
    double ll = 0.0;
    for (int sl = 0; sl < a.n_sl; ++sl) ll += a.llp[(size_t)sl * a.M + ml];
    if (a.likelihood == 1) ll -= (double)a.nr * (double)a.net.n[a.net.H + 1] * (log(a.noise) + 0.5 * kLog2Pi);
    a.ell[a.m0 + ml] = (T)(a.likeadj * ll - 0.5 * tt * ip2 - (double)d * (log(a.prior_std) + 0.5 * kLog2Pi));
  }
}

// ---- the launches' geometry: a function of the architecture, the rows and the cap alone ------------------------------------------------
// (one output: the layout the one-output kernels have always had; n_out >= 2: the head as layer H + 1, no output row)
static BnnNet bnn_net(const mivi_bnn_t &b, int p) {
  BnnNet nt{};
  nt.H = b.n_hidden;
  nt.n[0] = p;
  for (int l = 1; l <= nt.H; ++l) nt.n[l] = b.hidden[l - 1];
  nt.n[nt.H + 1] = b.n_out >= 2 ? b.n_out : 1;
  const bool head = nt.n[nt.H + 1] >= 2;
  const int nl = head ? nt.H + 1 : nt.H;   // layers staged as planes
  int off = 0, lds = 0;
  for (int l = 0; l <= nl; ++l) nt.P[l] = (nt.n[l] + 15) & ~15;
  for (int l = 1; l <= nt.H + 1; ++l) {
    nt.woff[l - 1] = off;
    off += nt.n[l] * nt.n[l - 1];
    nt.boff[l - 1] = off;
    off += nt.n[l];
  }
  nt.d = off;
  for (int l = 1; l <= nl; ++l) {
    nt.lw[l - 1] = lds;
    lds += nt.P[l - 1] * (nt.P[l] + 1);
    nt.lb[l - 1] = lds;
    lds += nt.P[l];
    nt.toff[l] = nt.toff[l - 1] + (nt.P[l] / 16) * (nt.P[l - 1] / 16);
  }
  if (!head) {
    nt.lwo = lds;
    lds += nt.P[nt.H];
  }
  int widest = head ? nt.P[nl] : 0;   // (the logits and delta_out live in a delta block)
  for (int l = 0; l <= nt.H; ++l) {
    nt.la[l] = lds;
    lds += nt.P[l] * kBnnLda;
    widest = nt.P[l] > widest ? nt.P[l] : widest;
  }
  for (int k = 0; k < 2; ++k) {
    nt.ldl[k] = lds;
    lds += widest * kBnnLda;
  }
  nt.lds_elems = lds;
  return nt;
}

// the LDS of a workgroup of the head kernels: the dynamic block and k_bnn_rows_head's static arrays (rowi, red)
size_t bnn_head_lds_bytes(const mivi_bnn_t &b, int p, size_t esize) {
  return (size_t)bnn_net(b, p).lds_elems * esize + kFlowTile * sizeof(long long) + 4 * sizeof(double);
}

static RowSlices bnn_slices(long long nr) { return row_slices(nr, kBnnSliceRows, 32); }
static int bnn_chunk(const mivi_ctx *c, const RowSlices &g, int M) {   // samples per chunk under the cap
  return samples_under_cap(c->bnn_rows.cap ? c->bnn_rows.cap : kBnnPartCap, (size_t)g.n_sl * c->cfg.d * sizeof(double), M);
}

bool bnn_reserve(mivi_ctx *c, int M) {
  const RowSlices g = bnn_slices(c->bnn_rows.nr);
  const size_t mc = (size_t)bnn_chunk(c, g, M);
  return !ensure(c, c->bnn_part, (size_t)g.n_sl * mc * c->cfg.d * sizeof(double), false) &&
         !ensure(c, c->bnn_ll, (size_t)g.n_sl * mc * sizeof(double), false);
}

template <typename T>
static BnnArgs<T> bnn_args(const mivi_ctx *c) {
  BnnArgs<T> a{};
  a.net = bnn_net(c->bnn, c->bnn_p);
  a.likelihood = c->bnn.likelihood;
  a.noise = c->bnn.noise;
  a.prior_std = c->bnn.prior_std;
  return a;
}

template <typename T>
static bool bnn_impl(mivi_ctx *c, int M, int want_grad) {
  const RowSlices g = bnn_slices(c->bnn_rows.nr);
  const int Mc = bnn_chunk(c, g, M);
  BnnArgs<T> a = bnn_args<T>(c);
  const auto rows_kernel = a.net.n[a.net.H + 1] >= 2 ? k_bnn_rows_head<T> : k_bnn_rows<T>;
  if (!flow_lds_attr<T>(rows_kernel, a.net.lds_elems)) return false;
  a.n = c->bnn_rows.n;
  a.nr = c->bnn_rows.nr;
  a.X = (const T *)c->bnn_X;
  a.y = (const T *)c->bnn_y;
  a.rows = c->bnn_rows.sel ? (const long long *)c->bnn_rows.idx.p : nullptr;
  a.Z = (const T *)c->Z.p;
  a.part = (double *)c->bnn_part.p;
  a.llp = (double *)c->bnn_ll.p;
  a.n_sl = g.n_sl;
  a.rps = g.rps;
  a.G = (T *)c->W.p;
  a.ell = (T *)c->ell.p;
  a.want_grad = want_grad;
  a.likeadj = c->bnn_rows.likeadj;
  const size_t lds = (size_t)a.net.lds_elems * sizeof(T);
  for (int m0 = 0; m0 < M; m0 += Mc) {   // chunks of samples: the f64 partials stay under their cap
    a.m0 = m0;
    a.M = M - m0 < Mc ? M - m0 : Mc;
    hipLaunchKernelGGL(rows_kernel, dim3(a.M, g.n_sl), dim3(256), lds, c->stream, a);
    hipLaunchKernelGGL(k_bnn_finish<T>, dim3(a.M), dim3(256), 0, c->stream, a);
  }
  return true;
}

// false: device allocation of the partials failed, or the runtime refused the kernel its LDS
bool launch_bnn_target(mivi_ctx *c, int M, int want_grad) {
  if (!bnn_reserve(c, M)) return false;
  return by_dtype(c, [&](auto t) { return bnn_impl<decltype(t)>(c, M, want_grad); });
}

template <typename T>
static bool bnn_forward_impl(mivi_ctx *c, const void *theta, int M, const void *Xnew, long long n_new, void *f) {
  const RowSlices g = bnn_slices(n_new);
  BnnArgs<T> a = bnn_args<T>(c);
  const auto forward_kernel = a.net.n[a.net.H + 1] >= 2 ? k_bnn_forward_head<T> : k_bnn_forward<T>;
  if (!flow_lds_attr<T>(forward_kernel, a.net.lds_elems)) return false;
  a.n = a.nr = n_new;
  a.X = (const T *)Xnew;
  a.Z = (const T *)theta;
  a.f = (T *)f;
  a.n_sl = g.n_sl;
  a.rps = g.rps;
  hipLaunchKernelGGL(forward_kernel, dim3(M, g.n_sl), dim3(256), (size_t)a.net.lds_elems * sizeof(T), c->stream, a);
  return true;
}

bool launch_bnn_forward(mivi_ctx *c, const void *theta, int M, const void *Xnew, long long n_new, void *f) {
  return by_dtype(c, [&](auto t) { return bnn_forward_impl<decltype(t)>(c, theta, M, Xnew, n_new, f); });
}

}  // namespace mivi
