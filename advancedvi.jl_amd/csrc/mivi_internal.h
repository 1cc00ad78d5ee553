// Internal declarations shared by the libmivi translation units (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/mivi.h"
#include "philox.h"
#include "switches.h"

namespace mivi {

constexpr double kLog2Pi = 1.8378770664093454835606594728112;

// --------------------------------------------------------------------------------------------
// Kernel argument blocks (plain structs passed by value)
// --------------------------------------------------------------------------------------------
struct RngArgs {
  uint64_t seed;
  uint64_t idx_base;        // estimate index = idx_base + (idx_ptr ? *idx_ptr : 0)
  const uint64_t *idx_ptr;  // device counter (graph replay) or nullptr
  int m_offset;             // first GLOBAL sample column of this context
};

enum TargetKind : int {
  TGT_NONE = 0,
  TGT_DIAG_GAUSS = 1,
  TGT_DENSE_GAUSS = 2,
  TGT_LOGREG = 3,
  TGT_FUNNEL = 4,
  TGT_CALLBACK = 5
};

// What the Stacked bijector does to one coordinate (kernels_bijector.hip).  The legacy mask of mivi_set_bijector_stacked holds 0 / 1:
// its exp kind IS BIJ_LOWER with lb = 0.
enum BijCode : int {
  BIJ_ID = 0,
  BIJ_LOWER = 1,      // x = lb + e^eta
  BIJ_UPPER = 2,      // x = ub - e^eta
  BIJ_BOTH = 3,       // x = lb + (ub - lb) sigma(eta)
  BIJ_ORD_HEAD = 4,   // first coordinate of an ordered block: x = eta
  BIJ_ORD = 5         // x_k = x_{k-1} + e^eta_k
};

// Fused funnel target (mean-field): the only cross-row coupling of Neal's funnel is S_m = sum_i x_im^2 per sample, needed by
// row 0's gradient and by ell -- and every use of it is LINEAR in S_m with a per-column weight any workgroup can re-derive
// from the eps stream (exp(-2 e1_m), exp(-2 e1_m) eps_0m).  So the main kernel's workgroups (rows >= 1) leave two scalar
// partials each,  A = sum_{i,m} x_im^2 exp(-2 e1_m)  and  B = sum_{i,m} x_im^2 exp(-2 e1_m) eps_0m  over their own rows, fold
// -A/2 into their ell partial, and whoever assembles the value adds the O(M) per-column terms and finishes row 0.
struct FunnelFin {
  const double *ab;    // [2][n_part] the A and B partials of the main kernel's workgroups  (nullptr = no funnel work)
  int n_part;
  const void *params;  // [mu; sigma]
  RngArgs rng;
  int d4, M;
  double sigma_v;
  const void *row0;    // nullptr: row 0's (mu, sigma) are params[0], params[d]; else {mu_0, sigma_0} published by the row-0 workgroup of the SAME
                       // launch (k_mf_funnel_sgd_loop): read with agent-scope atomic loads
  const unsigned *wait_word;   // k_mf_funnel_sgd_loop: the A / B (and every other) partial of this step is complete once wait_word[b] >= wait_val
  unsigned wait_val;           // for every row quad b < wait_n (one flag per workgroup: 512 read-modify-writes on ONE counter took 8 us);
  int wait_n, wait_budget;     // waited for (bounded, status bit 8) AFTER the per-column work, which needs none of them
  double *mirror;              // ... then copied in ONE batch of loads (one memory round trip instead of one per partial kind) into this LDS image,
  const double *mirror_src;    // which the partial pointers of the ValueIn (and `ab`) then point into
  int mirror_n;
};

// reduction inputs of the objective value, summed in a fixed order by one workgroup
struct ValueIn {
  FunnelFin fn;
  const double *ell_part;  // per-workgroup partial sums of sum_m ell_m (variable part)
  int n_ell_part;
  const double *ell_part2; // second set (the launching kernel's own partials)
  int n_ell_part2;
  const void *ell;         // per-sample ell (T), generic target route
  int n_ell;
  const double *he_part;   // partial sums of sum_m 0.5|eps_m|^2
  int n_he_part;
  const double *ld_part;   // [2][n_ld_part]: partial sums of log C_ii, then counts of non-positive C_ii (or nullptr)
  int n_ld_part;
  double ell_const;        // constant added per sample (target normaliser)
  // a non-normal base distribution (mivi_set_base_dist; 0 = Normal: the two constants are not read): he_part then holds the partial sums of
  // the variable part of -sum log phi(u), base_c0 = -(log phi's constant) per element, base_H = H(phi)
  int base;
  double base_c0, base_H;
};

// how results are emitted
struct OutArgs {
  void *grad;        // T[params_len]  (final mode)
  void *value;       // T[1]           (final mode)
  void *partials;    // T[params_len+2] (partials mode, un-normalised)
  int partials_mode; // 0 final, 1 partials
  long long scalars_off;  // index of [sum ell, sum 0.5 eps^2] inside the partials buffer
  int ent_kind;
  int M_total;       // global n_samples (normaliser)
  int M_local;
  int *status;       // device status word: bit0 nonfinite value, bit1 non-positive scale diag
  double *elbo_rec;  // optional: elbo_rec[rec_slot] = -value (optimize loop)
  int rec_slot;
  // partials mode on the peer-to-peer route, DIRECT: every entry of the partial vector is stored straight into its OWNER's staging area
  // (kernels_p2p.hip: no ring slot, no push pass).  p2p_direct: device-resident P2PDirectTab; (p2p_gi, p2p_v): the exchange group this estimate
  // belongs to, counted from the exchange kernel's start, and its place in the group.  Second-generation full-rank f32 kernels only.
  const void *p2p_direct;
  int p2p_gi, p2p_v;
};
struct P2PDirectTab {   // where the ranks' staging areas are mapped in this process (lane 0 of the exchange)
  char *stage[8];
  long long n;          // slice length (elements)
  int R, rank, GV, pad;
  const unsigned *ctr;  // the exchange lane's counters: ctr[0] = exchanges completed (the next group's epoch is ctr[0] + 1 + p2p_gi)
};

// Optimiser step fused into the VJP epilogue (device-resident optimisation loop, full-rank f32): every lower-triangle
// tile applies Descent / Adam (+ ClipScale on the diagonal) to its own parameters right where the gradient entry is
// produced, so the separate update kernel and the gradient round trip through HBM disappear.  rule < 0: off.
struct FusedUpdate {
  int rule = -1;              // 0 Descent, 1 Adam (optim_rules.h: bitwise the same arithmetic as kernels_update.hip)
  void *params;               // the parameter vector being optimised (same buffer the estimate reads)
  void *state;                // Adam: [m (params_len); v (params_len)]
  const long long *t_ptr;     // Adam step count = t_base + *t_ptr
  long long t_base;
  double eta, b1, b2, eps, clip_eps;
  int do_clip = 0;            // ClipScale on the scale diagonal after the step (explicit: epsilon <= 0 is a legal ClipScale)
};

template <typename T>
struct MfArgs {
  int d;
  int M;               // local samples processed by this launch
  int n_cc;            // column chunks (gridDim.y)
  int cols_per_cc;
  const T *params;     // [mu; sigma]
  RngArgs rng;
  int target;          // TGT_DIAG_GAUSS (fused) or TGT_NONE (W from G buffer)
  const T *t_mean;     // diag gauss mean[d]
  const T *t_istd;     // 1/std[d]
  const T *G;          // generic route: d x M gradient of log pi (ld = d)
  int want_grad;
  // scratch
  double *row_part;    // [n_cc][2*d4*4] partial row sums when n_cc > 1
  double *sc_part;     // [4 or 6][n_blocks] scalar partials: ell, 0.5 eps^2, log sigma, #bad sigma (+ funnel A, B)
  ValueIn vin;
  OutArgs out;
  long long *dbg;      // optional timeline: dbg[block*8 + k] = wall_clock64() stamps (nullptr = off)
  int has_prev;        // extra workgroup (blockIdx.x == ceil(d/4)) assembles the previous estimate's value
  ValueIn prev_vin;
  OutArgs prev_out;
};

template <typename T>
struct SampleArgs {  // rand(rng, q, M) -> Z (and eps)
  int d, M;
  const T *params;
  RngArgs rng;
  T *Z;       // d x M, ld = d
  T *eps;     // d x M, ld = ld_eps (or nullptr)
  int ld_eps;
  T *epsT;    // M x d transposed, epsT[m + k*ld_epsT] (or nullptr)
  int ld_epsT;
  double *he_part;  // per-block partial of sum 0.5 eps^2 (or nullptr)
};

template <typename T>
struct FrArgs {
  int d, M, dP, MP;
  const T *params;     // [mu; vec C]
  const T *eps;        // eps[i + m*dP]
  const T *epsT;       // epsT[m + k*MP]
  T *Z;                // Z[i + m*d] or nullptr
  T *W;                // W[i + m*d]: grad log pi (+ STL term)
  T *RT;               // (Z - t_mean)^T: RT[m + k*MP]  (dense target)
  int fused_target;    // TGT_NONE: write Z; TGT_DIAG_GAUSS: write W + ell partial; TGT_DENSE_GAUSS: write Z,RT
  const T *t_mean;
  const T *t_istd;
  const T *t_prec;     // precision matrix, ld = dP, zero padded
  double *ell_part;    // written by sample/target kernels
  double *ld_part;     // [2][nb]: per diagonal block sum log C_ii, then #non-positive C_ii (VJP kernel)
  ValueIn vin;
  OutArgs out;
  long long *dbg;      // optional timeline (nullptr = off)
  // work distribution + heterogeneous workgroups (MFMA kernel only)
  const int2 *work_tab;
  int n_work;          // index of the value workgroup (sample kernel) or INT_MAX
  int n_pre;           // leading workgroups that generate the next estimate's eps (VJP kernel)
  SampleArgs<T> next_eps;
  ValueIn prev_vin;
  OutArgs prev_out;
  FusedUpdate upd;     // VJP kernel, final mode only
  const T *adam_cc;    // LDS: the two Adam bias corrections of this step (set by the kernel)
};

struct ValueJob {      // deferred objective-value assembly of the previous estimate
  ValueIn vin;
  OutArgs out;
};
struct EpsJob {        // eps generation for the next estimate
  RngArgs rng;
  int parity;
};
// speculative eps prefetch across single calls: the VJP kernel of estimate (seed, idx) also generates eps of
// (seed, idx + 1) into the other parity; a following call for exactly that estimate skips its eps kernel.
// Looked up, published and dropped by api_estimate.hip (eps_spec_*); everyone else may only clear() it.
struct EpsSpec {
  bool valid = false;
  RngArgs rng{};
  int M = 0, parity = 0;
  int capturing = 0;
  unsigned long long capture_id = 0;
  void clear() { valid = false; }
};

template <typename T>
struct ColTargetArgs {  // standalone per-column targets: Z -> (ell, G)
  int d, M, kind;
  const T *Z;
  T *G;
  T *ell;
  const T *t_mean;
  const T *t_istd;
  double sigma_v;
  int want_grad;
  int constrained;   // funnel: theta_1 = s itself (no built-in exp bijector / log-Jacobian)
};

// The RealNVP family's architecture (mivi_flow_t behind mivi_create_flow) as the kernels take it, and the layout of its parameter vector:
// layers l = 1 .. L, each [s net; t net], a net [vec W_1; b_1; ...; vec W_{H+1}; b_{H+1}] from |B_l| inputs to |A_l| outputs.
// The neural spline flow (MIVI_NSF, mivi_spline_flow_t behind mivi_create_spline_flow) is the same architecture with K > 0 bins on
// [-B, B]: ONE net per layer from |B_l| inputs to |A_l| (3K - 1) outputs, coordinate-major.  K = 0: RealNVP.
struct FlowArch {
  int d, L, H;
  int h[3];
  int K;
  double B;
};
__host__ __device__ inline int nsf_rows(const FlowArch &a) { return 3 * a.K - 1; }   // output rows per transformed coordinate: u^w (K), u^h (K), u^d (K - 1)
__host__ __device__ inline int flow_nA(int d, int l) { return (l & 1) ? (d + 1) / 2 : d / 2; }   // |A_l|: the even coordinates for odd l, the odd ones for even l
__host__ __device__ inline long long flow_net_len(const FlowArch &a, int nin, int nout) {
  long long n = 0;
  int prev = nin;
  for (int j = 0; j < a.H; ++j) { n += (long long)a.h[j] * prev + a.h[j]; prev = a.h[j]; }
  return n + (long long)nout * prev + nout;
}

// --------------------------------------------------------------------------------------------
// Context
// --------------------------------------------------------------------------------------------
// Device memory of the library.  A DevBuf OWNS what `ensure` gave it (api_core.hip: the one function that allocates, next to release(), the
// one that frees) and frees it when it is released or destroyed; or it is a VIEW of memory another buffer owns (borrow: a child context's
// target vectors and status word), which it never frees.  Move-only: a copy would be a second owner.  p and bytes are there to be read;
// ensure, borrow and release are what writes them.
struct __attribute__((visibility("hidden"))) DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  bool owned = false;
  DevBuf() = default;
  DevBuf(const DevBuf &) = delete;
  DevBuf &operator=(const DevBuf &) = delete;
  DevBuf(DevBuf &&o) noexcept { *this = static_cast<DevBuf &&>(o); }
  DevBuf &operator=(DevBuf &&o) noexcept { std::swap(p, o.p); std::swap(bytes, o.bytes); std::swap(owned, o.owned); return *this; }   // (o takes what this held, and frees it)
  ~DevBuf() { release(); }
  void borrow(void *ptr, size_t n) { release(); p = ptr; bytes = n; }   // a view of [ptr, ptr + n): whoever owns it outlives this buffer
  void release();                                                       // frees what it owns, forgets what it borrowed: the buffer is empty
};

// The HIP handles of the library have owners of the same kind.  A Stream, an Event or a GraphExec holds ONE handle the library created and
// destroys it when it is reset or destroyed; move-only.  They are filled by make_stream / make_event (api_core.hip) and capture_graph
// (api_graph.hip) and by nothing else: those three, and handle_destroy below them, are the only places that name HIP's create / destroy
// calls.  A stream the CALLER owns (mivi_config_t.stream, mivi_set_stream) is never put into one.  None of them may have static storage
// duration: its destructor would run after the HIP runtime is gone (the note at MIVI_FB_DBG, kernels_fullrank_batch.hip).
#pragma GCC visibility push(hidden)
void handle_destroy(hipStream_t h);       // api_core.hip
void handle_destroy(hipEvent_t h);        // api_core.hip
void handle_destroy(hipGraphExec_t h);    // api_graph.hip
void count_handles(int delta);            // api_core.hip: the handles held in this process (mivi_batch_info what = 6)
#pragma GCC visibility pop
template <class H>
struct __attribute__((visibility("hidden"))) Handle {
  Handle() = default;
  Handle(const Handle &) = delete;
  Handle &operator=(const Handle &) = delete;
  Handle(Handle &&o) noexcept { std::swap(h, o.h); }
  Handle &operator=(Handle &&o) noexcept { std::swap(h, o.h); return *this; }   // (o takes what this held, and destroys it)
  ~Handle() { reset(); }
  H get() const { return h; }
  explicit operator bool() const { return h != nullptr; }
  void reset() { if (h) { handle_destroy(h); count_handles(-1); } h = nullptr; }
  void adopt(H created) { reset(); h = created; if (h) count_handles(1); }       // the three makers' only
 private:
  H h = nullptr;
};
using Stream = Handle<hipStream_t>;
using Event = Handle<hipEvent_t>;
using GraphExec = Handle<hipGraphExec_t>;

// The double-buffered two-stream exchange of the sharded batches: the exchange + finalisation of step i run on `stream` under the main
// stream's kernels of step i + 1, the buffers they read in two sets (i & 1).  ensure_pipe (api_core.hip) fills all five handles or none.
// Per step:  reuse (the exchange of step i - 2 has released this set) -> the main stream's kernels -> hand_over (part[i & 1] recorded on
// main, the pipe's stream waits for it and is what *xs names afterwards) -> the exchange on *xs -> finish (done[i & 1] recorded there);
// after the last step join: main waits for the done of the last min(n, 2) steps.  join_after_error is for a loop that leaves with an error
// after `n` hand-overs: it closes step n - 1 where the pipe's stream stands and joins the same way, unchecked -- the first error is the one
// reported, and no work that reads the caller's buffers stays queued on a stream the caller's does not wait for.  (api_common.h)
struct __attribute__((visibility("hidden"))) ExchangePipe {
  Stream stream;
  Event part[2], done[2];
  explicit operator bool() const { return (bool)stream; }
  mivi_status_t reuse(mivi_ctx *c, hipStream_t main, int i);
  mivi_status_t hand_over(mivi_ctx *c, hipStream_t main, int i, hipStream_t *xs);
  mivi_status_t finish(mivi_ctx *c, int i);
  mivi_status_t join(mivi_ctx *c, hipStream_t main, int n);
  void join_after_error(hipStream_t main, int n);
};

// third-generation batch engine (kernels_fullrank_batch.hip): work tables per lane count, per-lane work buffers (base + lane * stride)
struct __attribute__((visibility("hidden"))) FbTab {
  DevBuf prod, vjp, prod2, prod3;         // work tables: the draw's product, the VJP, the dense target's product, the sticking-the-landing product
  int n_prod = 0, n_vjp = 0, n_prod2 = 0, L = 0, M = 0;
};
struct __attribute__((visibility("hidden"))) FbTables {
  FbTab tab[4];                           // per lane count (the full step's, the last shorter step's, other batch lengths'), round robin
  int next_tab = 0;
  DevBuf CA, epsP, WV, ell, he, ld, grads, values;   // operand planes (tril(C) once per call; eps -- ONE orientation since round 6 -- and W per lane)
  DevBuf cscale, pscale, tscale, winv, rinv;               // power-of-two scales of the planes (fr_planes.h): rows of tril(C) / P / C^-T [2][d]; W per lane [M / 128][d]; R per lane [d / 128][M]
  DevBuf PA, RP;                          // dense-Gaussian target: planes of P (once per target), R = Z - m per lane
  bool PA_valid = false;
  DevBuf Tinv, TA, Eye;                   // sticking-the-landing estimators: C^-T (f32), its planes (once per call), the identity the solve takes
  DevBuf parts;                           // sharded batches: the lanes' shard-additive partial vectors (fb_part_len floats each), what one all-reduce sums
  int cap_L = 0, cap_M = 0, cap_LR = 0, cap_LP = 0;
};
struct FbStep {
  const void *params;
  int M, L;
  RngArgs rng;                            // lane l draws estimate rng_index(rng) + l
  void *grads; long long grad_stride;     // lane l's gradient (elements)
  void *values; long long value_stride;
  void *grad_last, *value_last;           // lane_last writes these instead (nullptr: none)
  int lane_last;
  int write_upper;                        // lanes write the exact zeros above the diagonal (0: their buffers hold them already)
  int dense;                              // dense-Gaussian target: two products per lane
  int stl;                                // sticking-the-landing estimators: W += C^-T eps as one more product per lane
  const FbTab *tab;
  int obj;                                // objective mode (mivi_estimate_objective): the lanes are consecutive blocks of n_mc samples of ONE estimate index; values only
  int ent_kind;                           // objective mode: the entropy estimator of the value
  int values_only;                        // no gradient is wanted (mivi_estimate_gradient_each without grads; objective mode): no VJP tile runs
  void *parts; long long part_stride;     // sharded batches: the VJP leaves lane l's UNNORMALISED partial vector at parts + l part_stride instead of a gradient
};

// What a cached hipGraphExec was recorded for (api_graph.hip): a call replays it only if every field matches.
enum GraphKind {
  GRAPH_NONE = 0,
  GRAPH_CHAIN,           // `count` chained estimates on one stream
  GRAPH_FORKED_CHAINS,   // one chain per context (`lanes` of them) behind a fork event
  GRAPH_LANE_BRANCHES,   // branches of `per_branch` lane-batched contexts, `lanes` contexts in all
  GRAPH_LOOP,            // the optimisation loop as a graph of launches (`loop`)
  GRAPH_SHARDED,         // a sharded batch (`mode`, `route`)
};
struct GraphKey {
  GraphKind kind = GRAPH_NONE;
  int count = 0;
  const void *params = nullptr;
  void *value = nullptr;
  void *grad = nullptr;
  int lanes = 0, per_branch = 0;   // GRAPH_FORKED_CHAINS / GRAPH_LANE_BRANCHES
  int route = 0, mode = 0;         // GRAPH_SHARDED: mivi_comm_route, the sequence (api_dist.hip dist_sequence); GRAPH_LOOP: mode = first_batch + 1 of mivi_optimize_loop_batches (0: not over a schedule)
  mivi_loop_t loop{};              // GRAPH_LOOP: the configuration the captured loop was built for
};
struct GraphCache {
  GraphExec exec;
  GraphKey key;
  bool matches(const GraphKey &k) const;
  void drop();   // destroys the cached hipGraphExec, if any, and empties the slot
};

// Lane-batched estimates (second-generation full-rank kernels): up to four contexts -- the LANES of one graph branch -- run their estimates
// with c->rec set.  The launchers then record their argument blocks here instead of launching, and the driver issues ONE launch per kernel
// for all lanes (launch_lanes_*; blockIdx.y = lane).  While `closing` is false the estimates' kernels record: launch_eps (a chain's first
// draw), launch_lds_prod32, launch_stl2 (if the recorder has the STL part), launch_lds_vjp.  While it is true only launch_value_only (a
// chain's closing value kernel) does.  The argument blocks of the product / VJP and of the STL term stay private to their units.
struct LaneKernelArgs;   // kernels_fullrank_lds.hip: a lane's product(s) and VJP
struct LaneStlArgs;      // kernels_stl.hip: a lane's solve jobs and combining product
void lane_args_resize(LaneKernelArgs *&p, int lanes);   // frees p; lanes > 0: p = new zeroed blocks for `lanes` lanes
void lane_args_resize(LaneStlArgs *&p, int lanes);
struct LaneRecorder {
  struct Lane {
    int n_prod, n_vjp, n_stl, n_eps;   // launches recorded since reset_lane (n_eps: since reset_step)
    bool vjp_refused;                  // a VJP the lanes' launch cannot serve came by: 64 x 64 tiles, or a fused optimiser update
  };
  Lane lane[4] = {};
  LaneKernelArgs *kern = nullptr;
  LaneStlArgs *stl = nullptr;          // nullptr: no STL part (launch_stl2 launches as usual)
  SampleArgs<float> eps[4];            // per branch: the first draws of the lanes that made one ...
  int eps_grid[4];
  ValueIn value_in[4];                 // ... and the closing values, in the order they came
  OutArgs value_out[4];
  int n_value = 0;
  bool closing = false;

  LaneRecorder(int lanes, bool with_stl) {
    lane_args_resize(kern, lanes);
    if (with_stl) lane_args_resize(stl, lanes);
  }
  ~LaneRecorder() {
    lane_args_resize(kern, 0);
    lane_args_resize(stl, 0);
  }
  LaneRecorder(const LaneRecorder &) = delete;
  LaneRecorder &operator=(const LaneRecorder &) = delete;
  void reset_step() { for (Lane &l : lane) l.n_eps = 0; }
  void reset_lane(int l) { lane[l].n_prod = lane[l].n_vjp = lane[l].n_stl = 0; lane[l].vjp_refused = false; }
  // did lane l's estimate take the route the lanes' launches serve?  Exactly one sampling product (and the dense target's, if any: their
  // kinds are checked by launch_lanes_prod), one VJP on 32 x 32 tiles without a fused update, one STL term if any.
  bool lane_took_route(int l, bool dense, bool with_stl) const {
    return lane[l].n_prod == (dense ? 2 : 1) && lane[l].n_vjp == 1 && !lane[l].vjp_refused && (!with_stl || lane[l].n_stl == 1);
  }
};

}  // namespace mivi

// The streams and events a context created, every one in its owner.  A base of mivi_ctx, so that they are destroyed AFTER the context's
// buffers are freed (members go before bases): no buffer outlives the stream its last launch ran on.
struct mivi_ctx_streams {
  static constexpr int kMaxKids = 15;   // up to sixteen contexts (eight are used); at most FOUR graph branches (a forked graph with five branches crashed inside hipGraphLaunch,
                                       // hip::Graph::UpdateStreams, after a re-capture on ROCm 7.0's runtime; four is also the number of hardware queues)
  hipStream_t stream = nullptr;   // what the context launches on: the CALLER's stream (or the null stream), or a view of `own`
  mivi::Stream own;               // mivi_config_t.own_stream: the non-blocking stream the context created for itself
  mivi::Stream cap_stream;        // internal stream used only for graph capture (api_graph.hip)
  // Pipelined exchange (mivi_estimate_gradient_dist_n, api_dist.hip): the collective of estimate t runs on pipe.stream under the kernels of
  // t + 1, the partial vectors double-buffered (dist_P, dist_P2).  The peer-to-peer pipeline runs its persistent exchange kernel there
  // between part[0] and done[0], which is why the stream has a hardware queue of its own (dist_batch).
  mivi::ExchangePipe pipe;
  // the batch engine's sharded batches (api_batch.hip fb_batch, dist): the all-reduce + finalisation of step s on fb_pipe.stream under the
  // kernels of step s + 1 (a plain non-blocking stream of its own: pipe.stream carries the CU mask the peer-to-peer pipeline needs)
  mivi::ExchangePipe fb_pipe;
  mivi::Event ev_fork, ev_join[kMaxKids];   // interleaved chains: the fork of a recording's branches, the join of child j's
  __attribute__((visibility("hidden"))) ~mivi_ctx_streams() = default;   // (the owners' work; said only to keep it out of the exported symbols)
};

// Every device buffer below is a member and nothing else: ensure() fills it where it is needed, the context's destruction returns it.
struct mivi_ctx : mivi_ctx_streams {
  mivi_config_t cfg;
  std::string err;
  int target = mivi::TGT_NONE;
  int M_total = 0;
  size_t esize = 4;

  // target data
  mivi::DevBuf t_mean, t_istd, t_prec;
  double t_const = 0.0;  // per-sample constant of log pi
  double funnel_sigma_v = 1.5;
  int funnel_constrained = 0;
  // Stacked bijector (mivi_set_bijector_stacked): per-coordinate kind (0 identity, 1 exp) and per-column sum of eta over exp rows
  mivi::DevBuf bij_mask, bij_ld;
  // ... and its extended form (mivi_set_bijector_stacked_ex, kernels_bijector.hip): the host description per coordinate (BijCode; lb, ub),
  // its device copy (uploaded by the _ex setter, or on the first constrained rand / logpdf behind the legacy setter), the eta the backward
  // pass reads (d x cap_M, only with bij_ext) and the scratch of mivi_logpdf_constrained
  std::vector<uint8_t> bij_code_h;
  std::vector<double> bij_bnd_h;
  mivi::DevBuf bij_code, bij_bnd, bij_eta, bij_scr;
  bool bij_ext = false;   // a truncated / ordered block is present: launch_bij_forward / _backward take the kernels of kernels_bijector.hip
  bool bij_ord = false;   // ... an ordered one: the segmented scan runs
  bool bij_tab = false;   // bij_code / bij_bnd on the device match the host description
  // collective behind the C ABI (mivi_comm_init): RCCL communicator + padded partial / packed-final buffers
  void *comm = nullptr;
  int comm_rank = 0, comm_world = 1;
  mivi::DevBuf dist_P, dist_S, dist_F;
  bool bij_on = false;
  mivi::DevBuf dist_P2, dist_ring[6];       // the pipelined exchange's second partial vector; ring of partial vectors (two for the RCCL pipeline, eight = two groups of four for the peer-to-peer pipeline)
  int p2p_pipe_state = 1;   // persistent peer-to-peer pipeline in batched calls: 1 on, -1 off (mivi_p2p_set_pipeline: serial steps)
  int dist_route = 0;   // mivi_comm_set_route: 0 by size, 1 ncclAllReduce, 2 ncclReduceScatter / ncclAllGather, 3 peer-to-peer kernel
  // peer-to-peer exchange over xGMI (kernels_p2p.hip): one uncached allocation per rank [stage | final | flags], mapped into the peers by IPC
  mivi::DevBuf p2p_buf;   // (fine-grained device memory)
  void *p2p_peer[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};   // mapped bases (own entry = p2p_buf)
  bool p2p_opened[8] = {false, false, false, false, false, false, false, false};                   // hipIpcOpenMemHandle'd (to be closed)
  mivi::DevBuf rows_eps;   // kernels_fullrank_rows.hip: eps of all steps of a device-resident loop call
  mivi::DevBuf gen_scratch;  // kernels_meanfield.hip k_mf_gen_loop: DoG / DoWG partial norms of every step, arrival flags
  mivi::DevBuf many_buf;     // mivi_optimize_loop_many: the runs' table, status words, targets, ELBO records and last values (many_layout, api_optimize.hip)
  mivi::DevBuf p2p_tab, p2p_ctr, p2p_scratch, p2p_direct;   // (p2p_direct: P2PDirectTab, what the partial kernels need to store straight into the owners' staging areas)
  bool p2p_on = false;
  bool p2p_distinct = false;     // the attached exchange areas include one of ANOTHER device (not only this process's own contexts on this device)
  bool p2p_verified = false;     // mivi_p2p_selfcheck passed on every rank: only then does the automatic route take the peer-to-peer kernel at world > 1
  int p2p_rank = 0, p2p_world = 1, p2p_G = 1, p2p_vs = 0, p2p_spin = 1 << 21;
  long long p2p_n = 0, p2p_cn = 0;
  size_t p2p_lane_bytes = 0, p2p_off_fin = 0, p2p_off_arr = 0, p2p_off_farr = 0;
  // logreg
  const void *lr_X = nullptr;
  const uint8_t *lr_y = nullptr;
  mivi::DevBuf lr_X_own, lr_y_own, lr_scratch, lr_part, lr_Xrm, lr_xmax, lr_XA, lr_XB, lr_ZP;   // (lr_xmax: bits of max |X|, the scale of X's f16 splits)
  // minibatch view (AdvancedVI.subsample, docs/src/tutorials/subsampling.md:99-102): the full data set stays resident,
  // mivi_logreg_select_rows gathers the batch rows into lr_Xsub / lr_ysub / lr_Xrm_sub and points the active fields at them
  const void *lr_X_full = nullptr;
  const uint8_t *lr_y_full = nullptr;
  int64_t lr_n_full = 0;
  double lr_likeadj_full = 1.0;
  const void *lr_Xrm_act = nullptr;      // row-major copy the MFMA kernels read (full or batch)
  mivi::DevBuf lr_Xsub, lr_ysub, lr_Xrm_sub, lr_idx;
  int lr_route = 0;                        // 0 auto (by problem size), 1 matrix-core kernels, 2 VALU kernels (mivi_set_logreg_route)
  int64_t lr_n = 0;
  int lr_variant = 0;
  double lr_likeadj = 1.0;
  // schedule of minibatches (mivi_logreg_set_batch_schedule): n_batches x batch rows of the full data set, resident as int32, and the
  // estimate index of every batch (if given).  While one is set lr_n = batch and lr_likeadj is the schedule's; the selected batch lr_sched_k
  // is a host-side field -- a launch passes lr_sched_rows + k * batch by value -- and nothing is gathered ahead of an estimate.
  mivi::DevBuf lr_sched_rows, lr_sched_idx;
  int lr_sched_n = 0;                      // batches (0: no schedule)
  int lr_sched_k = 0;                      // the selected batch (mivi_logreg_seek_batch; the loop's recorder walks it)
  int lr_sched_kernels = 0;                // 0 by size | 1 the fused minibatch kernel | 2 device gather + the resident-data kernels
  bool lr_sched_has_idx = false;
  int lr_loop_first = -1;                  // >= 0 while mivi_optimize_loop_batches runs: step t of the loop evaluates batch lr_loop_first + t
  // callback
  mivi_logdensity_and_gradient_fn cb_grad = nullptr;
  mivi_logdensity_fn cb_value = nullptr;
  void *cb_user = nullptr;
  mivi_logdensity_gradient_and_hessian_fn cb_hess = nullptr;   // second-order plugin (mivi_gauss_expected_grad_hess2)
  void *cb_hess_user = nullptr;
  std::vector<char> h_Z, h_G, h_ell;

  // work buffers (sized for `cap_M` samples)
  int cap_M = 0;
  // buffers indexed [cur] are double-buffered so that, inside a captured graph, eps generation of estimate t+1
  // and the value assembly of estimate t overlap the contractions of the neighbouring estimates
  mivi::DevBuf eps[2], epsT[2], ell_part[2], he_part[2], sc_part[2], ld_part[2];
  mivi::DevBuf tabA, tabB, tabD;   // XCD-aware work tables of the MFMA kernels
  mivi::DevBuf stl_CT, stl_Dinv;   // transposed scale + inverted diagonal blocks (full-rank STL, f32)
  mivi::DevBuf stl_F;              // second-generation STL solve: packed operands (stl_dinv.h: pivot inverses + off-diagonal blocks, fragment order)
  bool want_stl_pack = false, stl_pack_done = false;   // Stein estimator: ask the sampling kernel to carry the solve's riders
  mivi::DevBuf stl_X;              // second-generation STL solve: X of the lower half + updated right-hand side of the upper half
  // second-generation full-rank kernels (kernels_fullrank_lds.hip): VJP work lists (32 x 32 and 64 x 64 tiles)
  mivi::DevBuf lds_tabV, lds_tabV64, lds_tabS;   // (lds_tabS: the strips of k_fr_vjp32s)
  int lds_nV = 0, lds_nV64 = 0, lds_nS = 0, lds_M = -1;
  bool d_idx_valid = false;          // the device-side estimate counter (d_idx[0]) is known to hold d_idx_expect
  uint64_t d_idx_expect = 0;
  mivi::DevBuf lds_tabSt;            // Stein accumulation stage: the full square of 64 x 64 tiles
  int lds_nSt = 0, lds_st_d = -1;
  mivi::ValueJob *defer_value = nullptr;   // non-null: run_estimate_lds(stop_after_target) hands its value job over instead of launching it
  bool value_deferred = false;
  int he_n[2] = {0, 0};            // number of sum-0.5-eps^2 partials behind he_part[parity] (depends on who drew eps)
  int nA = 0, nB = 0, nD = 0, tab_M = -1;
  int cur = 0;
  int mf_nblk = 0;
  mivi::DevBuf Z, W, RT, ell, X;
  mivi::DevBuf row_part, status, d_idx, acc, tmp_params, tmp_out;
  mivi::DevBuf obj_vals;   // mivi_estimate_objective on the batch engine: the lanes' values
  mivi::DevBuf stein_A, stein_g;   // Stein estimator: eps G^T accumulator (dP x dP, T) and the f64 column sums of G
  mivi::DevBuf sg_S, sg_d;         // score-gradient estimator (kernels_score.hip): -E diag(f - mean f) laid out like eps (full-rank); f64 [|eps_m|^2; dense ell_m; f_m - mean f] (3 x cap_M)
  int sg_cap = 0;                  // samples sg_d is sized for
  mivi::DevBuf ms_work, ms_part;   // the measure-space updates' one scratch pair, ensured by each update to its own need and holding nothing between calls.  Square-root NGD (kernels_ngd.hip): [Cc; G; T; v] padded to whole tiles | the diagonal tiles' f64 partials + the ticket.  Natural gradient (kernels_natgrad.hip): f64 [Gh; Sigma; W; A; X] padded to whole tiles + the inverted diagonal tiles | the panels' f64 log sums and bad-pivot counts + the mean's four vectors.  Batch and match (kernels_bam.hip): f64 [A; Dinv; Q, Ut, Zt, SQ, Y; M, E1, ME; gbar, ubar, zbar] | the objective's tile partials, then the panels' pairs
  mivi::DevBuf bam_host;   // api_measure.hip: [Sigma (d x d); u (d x n); G (d x n); fisher, logpi_avg, elbo / entropy (16 bytes each)] of the batch-and-match _host entries
  mivi::DevBuf ngd_est, natgrad_host;   // api_measure.hip: [logpi_avg or entropy (16 bytes); grad (d); hess (d x d)] of the _steps loops and the _host updates; [S; Sigma] of mivi_natgrad_update_host / Sigma of mivi_wass_update_host
  mivi::DevBuf h2_acc;             // second-order branch of the logistic-regression / funnel targets: f64 sums (kernels_hess2.hip)
  mivi::DevBuf lowr_E, lowr_V, lowr_prep, lowr_sx, lowr_part;   // low-rank family (kernels_lowrank.hip): the draws (d + r) x cap_M; V = Sigma^-1 (z - m), d x cap_M (t before that); the f64 prep block; f64 [s (r x cap_M); x (r x cap_M); |t|^2 (cap_M); log q (cap_M)]; the VJP's f64 partials, 8 slices x params_len
  // RealNVP family (kernels_flow.hip): its architecture (L = 0: not a flow context); every layer's input and the last one's output, (L + 1) x cap_M x d;
  // the f64 log q per sample; the VJP's f64 partials, flow_slices x params_len
  mivi::FlowArch flow{};
  mivi::DevBuf flow_X, flow_lq, flow_part;
  // base distribution of the location-scale families (mivi_set_base_dist; base_dist.h, kernels_basedist.hip, api_basedist.hip)
  int base = MIVI_BASE_NORMAL;
  double base_nu = 0.0, base_c0 = 0.0, base_H = 0.0;   // TDist's degrees of freedom; -(constant of log phi); H(phi) -- f64, computed once on the host
  mivi::DevBuf bd_U, bd_R;   // mean-field: the draws laid out like eps (ld dP, zero padded); both families, sticking-the-landing kinds: the plane -psi(U), same layout
  // mivi_logpdf (api_logpdf.hip, kernels_logpdf.hip): scratch of its own, so that a call between two estimates touches nothing of theirs.
  // lp_dinv: the inverted 32 x 32 diagonal blocks (full-rank); lp_scal: f64 [sum log C_ii] (low-rank: the prep block of kernels_lowrank.hip);
  // lp_work: the f64 X of a chunk when it does not fit LDS (full-rank), t and f64 [s; x; |t|^2; log q] of a chunk (low-rank); lp_host: [Z; log q; u] of the _host form
  mivi::DevBuf lp_dinv, lp_scal, lp_work, lp_host;
  mivi::DevBuf dog_part;   // DoG / DoWG on large parameter vectors: 512 x 2 partial norms + the step size
  const uint64_t *idx_src = nullptr;   // mivi_set_index_source
  mivi::EpsSpec pre;   // the eps speculation across single calls
  long long *dbg = nullptr;   // timeline buffer supplied through mivi_debug_timeline (tools only)
  int dP = 0, MP = 0;

  mivi::GraphCache graph;
  int graph_records = 0;   // graphs recorded into the cache slot so far (mivi_batch_info what = 4: a test can tell a replay from a re-capture)
  mivi::FbTables fb;   // batch engine buffers (mivi_estimate_gradient_n / _each on the third-generation route)

  // Interleaved chains (mivi_estimate_gradient_n, full-rank + Gaussian targets): estimates at fixed parameters are independent, so a
  // batch is dealt round-robin onto `1 + n_kids` chains -- this context and child contexts with their own work buffers and streams --
  // whose kernels overlap on the device (the product of one chain's estimate runs beside the VJP of another's).
  int idx_stride = 1;            // estimate-index step between consecutive estimates of THIS context's chain
  bool is_child = false;         // t_mean / t_istd / t_prec and status are views of the parent's (sync_kid, ensure_kids)
  int n_cu = 0;                  // compute units of the device, LDS bytes a workgroup may take: what the launch-free loops with a grid-wide
  size_t lds_max = 64 * 1024;    // exchange per step check their grids against (hipOccupancyMaxActiveBlocksPerMultiprocessor x n_cu >= grid)
  bool exchange_lost = false;    // a grid-wide exchange expired once on this context (status bit 8): those loops are not taken again
  int last_status_bits = 0;      // the sticky device flags read_status saw last
  int last_loop = 0;             // the DeviceLoopId the last mivi_optimize_loop call ran on, 0: the graph of launches (mivi_batch_info what = 7)
  mivi::DevBuf snap;             // parameters / optimiser state / average before a loop with a grid-wide exchange (restored if it is lost)
  mivi_ctx *kids[kMaxKids] = {};
  int n_kids = 0;
  unsigned long long target_gen = 0, kid_gen = ~0ull;   // parent: bumped whenever a captured graph is invalidated; child: the generation it mirrors
  bool dist_capture_refused = false;   // the sharded batch could not be captured into a hipGraph (RCCL route): issued eagerly from then on
  bool dist_direct = false;      // sharded estimates on the peer-to-peer route: the partial kernels store straight into the owners' staging areas
  bool dist_lane4 = false;       // pipelined sharded batches: the compute chain is lane-batched (four contexts per launch)
  mivi::LaneRecorder *rec = nullptr;   // lane-batched estimates: non-null while this context is lane `lane_id` of a branch whose launchers record
  int lane_id = 0;                     // into `rec` instead of launching (set and cleared by LaneScope, api_common.h)
  mivi::DevBuf kid_out[kMaxKids];       // value (16 bytes) + gradient of the child chains that do not hold the batch's last estimate

  // The communicator and the peer-to-peer areas (mivi_p2p_detach closes the peers' IPC handles before the area is released), the graph cache;
  // then the buffers go (members), then the streams and events (the base).  The wait for the stream and the children are mivi_destroy's.
  ~mivi_ctx() { (void)mivi_comm_destroy(this); graph.drop(); }
};

#pragma GCC visibility push(hidden)   // api_core.hip: the library's device memory (DevBuf); internal to libmivi like everything in api_common.h
// b holds at least `bytes` bytes (0: 16) afterwards.  Grow-only: a buffer that is large enough is kept, with its contents; otherwise it is
// released and allocated anew (fine_grained: as fine-grained device memory, the peer-to-peer area), and zeroed by a memset on c->stream if `zero`.
mivi_status_t ensure(mivi_ctx *c, mivi::DevBuf &b, size_t bytes, bool zero, bool fine_grained = false);
mivi_status_t ensure_zeroed(mivi_ctx *c, mivi::DevBuf &b, size_t bytes);         // ensure, and the first `bytes` bytes are zero (a memset on c->stream) whether the buffer was kept or not
mivi_status_t upload(mivi_ctx *c, mivi::DevBuf &b, const void *src, size_t bytes);   // ensure, then a synchronous copy of `bytes` host bytes into it
int32_t live_allocations();   // what this process holds of them right now, over all contexts (mivi_batch_info what = 5)
// api_core.hip: the library's streams and events.  Each leaves its owner filled, or reports through c->err and leaves it as it was.
// own_queue: a stream with a hardware queue of its own (dist_batch says who needs one and why); a plain non-blocking stream otherwise, and
// whenever the context lives on the null stream or the runtime refuses.  timing = false: hipEventDisableTiming.
mivi_status_t make_stream(mivi_ctx *c, mivi::Stream &s, bool own_queue);
mivi_status_t make_event(mivi_ctx *c, mivi::Event &e, bool timing);
mivi_status_t ensure_pipe(mivi_ctx *c, mivi::ExchangePipe &p, bool own_queue);   // nothing to do on a filled pipe; all five handles or none
int32_t live_handles();       // streams, events and graph execs the library holds right now in this process (mivi_batch_info what = 6)
#pragma GCC visibility pop

// The one precision dispatch of the host launch layer: f(T{}) with T the context's element type, its result returned.  A launch whose two
// precisions differ in nothing but T goes through it; one whose precisions take different routes keeps its explicit test on cfg.dtype.
template <typename F>
inline auto by_dtype(const mivi_ctx *c, F &&f) { return c->cfg.dtype == MIVI_F32 ? f(float{}) : f(double{}); }

namespace mivi {

// kernels_meanfield.hip
struct ValueJob;
void launch_mf_main(mivi_ctx *c, const void *params, const RngArgs &rng, int M, int want_grad, const void *G,
                    const ValueIn &vin, const OutArgs &out, const ValueJob *prev = nullptr);
// ---- the launch-free loops ------------------------------------------------------------------------------------------------------------
// mivi_optimize_loop walks kDeviceLoops (api_common.h: one row per launch-free optimisation loop, in priority order; first match).  A row
// is defined beside its kernel; `takes` is the WHOLE condition of the row apart from the two the dispatcher owns (no_device_loops, and
// allow_exchange for a row that exchanges).
enum DeviceLoopId : int { LOOP_GRAPH = 0, LOOP_MF_SGD = 1, LOOP_LR_SMALL = 2, LOOP_MF_GEN = 3, LOOP_FR_SMALL = 4, LOOP_FR_ROWS = 5, LOOP_MF_FUNNEL_SGD = 6,
                          LOOP_MANY = 16 };   // LOOP_MANY | row id: mivi_optimize_loop_many ran on that row's kernel, workgroup k = run k
struct LoopBufs {       // what the dispatcher owns (c->X)
  void *value, *grad;   // the value word (8 elements), the gradient scratch (params_len elements)
  double *rec, *area;   // the f64 ELBO record (n_steps doubles) and, behind it, the hist / partials area: the largest hist_doubles of the table (+ 8)
};
// mivi_optimize_loop_many: independent runs of one shape in ONE launch, workgroup (0, k) = run k.  What differs between the runs reaches the
// kernel through a device table (one ManyRun per run) and run-major arrays; a short prologue of the kernel offsets its pointers by the run.
struct ManyRun {
  uint64_t seed, idx0;     // the run's Philox seed and first estimate index
  double eta, ell_const;   // its step size; the per-sample constant of its diagonal-Gaussian target
};
struct ManyLaunch {
  int n_runs;
  const ManyRun *runs;             // device, [n_runs]
  int *status;                     // device, [n_runs]: bit 1 non-finite objective, bit 2 non-positive scale diagonal -- a word per run
  const void *t_mean, *t_istd;     // diagonal-Gaussian target: device T[n_runs d], or nullptr = the context's target for every run
  const uint8_t *y;                // logistic regression: device uint8[n_runs n], or nullptr = the context's y for every run
  const void *X;                   // ... device X (n x p column-major) of run 0, or nullptr = the context's X for every run
  long long x_stride;              // ... elements between the runs' X (0: one shared matrix)
};
constexpr int kManyGridY = 65535;  // runs per launch (gridDim.y); more runs: further launches of the same kernel at a run offset
constexpr int kExchangesNever = 1 << 30;
struct DeviceLoop {
  int id;
  bool (*takes)(const mivi_ctx *c, const mivi_loop_t &l, bool general);   // pure host predicate
  int exchanges_from;                                                     // rules >= this exchange grid-wide every step (0: all, 2: DoG / DoWG -- two global norms)
  mivi_status_t (*reserve)(mivi_ctx *c, const mivi_loop_t &l);            // the loop's own buffers (rows_eps, gen_scratch); nullptr: none
  size_t (*hist_doubles)(const mivi_ctx *c, int n_steps);                 // what it needs of LoopBufs::area; nullptr: nothing
  bool (*launch)(mivi_ctx *c, void *params, const mivi_loop_t &l, const LoopBufs &b);   // false: not launched (an exchanging grid not resident, the LDS refused): the next row
  // mivi_optimize_loop_many (nullptr: the row has no such form).  takes_many: the row's condition with ONE workgroup per run; launch_many:
  // every array run-major (params, l.opt_state_dev, l.avg_params_dev; b.rec [n_runs][n_steps], b.value [n_runs]), no exchange of any kind
  bool (*takes_many)(const mivi_ctx *c, const mivi_loop_t &l) = nullptr;
  bool (*launch_many)(mivi_ctx *c, void *params, const mivi_loop_t &l, const LoopBufs &b, const ManyLaunch &m) = nullptr;
};
DeviceLoop loop_mf_sgd(), loop_mf_gen(), loop_mf_funnel_sgd(), loop_fr_small(), loop_fr_rows(), loop_lr_small();   // the rows: kernels_meanfield / _fullrank_small / _fullrank_rows / _logreg_small.hip
// simple: what the fused paths implement (Descent / Adam, at most ClipScale, no averager); general := !simple || (Adam with other betas than
// their defaults: the general loops take them from the call).  The fast class is exactly !general: simple && (rule == 0 || default Adam).
inline bool loop_general(const mivi_loop_t &l) {
  const bool simple = l.rule <= 1 && l.op <= 1 && l.averager == 0;
  return !simple || (l.rule == 1 && !(l.beta1 == 0.9 && l.beta2 == 0.999 && l.adam_eps == 1e-8));
}
inline double loop_clip_eps(const mivi_loop_t &l) { return l.op == 1 ? l.clip_epsilon : (double)NAN; }   // NaN = no ClipScale
// kernels_meanfield.hip: the launch-free batches of estimates at FIXED parameters (mivi_estimate_gradient_n, mivi_profile_kernel which = 5) --
// their predicates (the optimisation loops' too) and the layout of their one scratch buffer, `_scratch_doubles` doubles carved from its base
bool mf_diag_loop_ok(const mivi_ctx *c);     // mean-field, diagonal-Gaussian target, no Stacked bijector, a bounded n_mc
bool mf_funnel_loop_ok(const mivi_ctx *c);   // mean-field, fused (unconstrained) funnel target, no Stacked bijector, a bounded n_mc
struct MfEstScratch { double *hist, *elbo; void *sc, *lanes, *e0; };   // sc, e0: the funnel's finishing scratch and eps[0, m] table; lanes: the estimate lanes' gradients
size_t mf_est_loop_scratch_doubles(const mivi_ctx *c, int n);
MfEstScratch mf_est_loop_carve(const mivi_ctx *c, void *base, int n);
size_t mf_funnel_loop_scratch_doubles(const mivi_ctx *c, int n);
MfEstScratch mf_funnel_loop_carve(const mivi_ctx *c, void *base, int n);
// rule 0 Descent / 1 Adam: the optimisation loop (loop_mf_sgd); rule -1: n_steps estimates at fixed parameters
void launch_mf_sgd_loop(mivi_ctx *c, void *params, void *opt_state, uint64_t idx0, long long t0, int n_steps, int rule,
                        double eta, double clip_eps, double *hist, double *elbo, void *grad_out = nullptr, void *lane_scratch = nullptr,
                        void *value_last = nullptr);   // value_last: the last step's objective value as an element of T (written by the value kernel)
void launch_mf_funnel_loop(mivi_ctx *c, const void *params, uint64_t idx0, int n_steps, double *hist, double *elbo, void *scratch,
                           void *value, void *grad, void *lane_scratch, void *e0_tab = nullptr);
void launch_sample_mf(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *Z, void *eps, int ld_eps,
                      double *he_part);

// kernels_fullrank.hip
int launch_eps(mivi_ctx *c, const RngArgs &rng, int M);   // returns the number of he_part entries the draw leaves
void launch_fr_sample(mivi_ctx *c, const void *params, int M, int fused_target, void *Z, const ValueJob *prev = nullptr);
void launch_fr_vjp(mivi_ctx *c, const void *params, int M, const OutArgs &out, const EpsJob *next = nullptr,
                   const ValueJob *self = nullptr, const FusedUpdate *upd = nullptr);
int fr_ld_blocks(const mivi_ctx *c);
// Build + upload the first-generation MFMA kernels' work tables for M samples per launch, once per M (nothing to do for f64, nor for the
// other families without the dense target).  A driver calls it before its first launch_fr_* / fr_*_blocks for that M; false: an allocation
// or upload failed.  prepare_tables: the same and the second-generation work lists where the shape takes them (lds_prepare), ahead of a capture.
__attribute__((visibility("hidden"))) bool fr_prepare(mivi_ctx *c, int M);
bool prepare_tables(mivi_ctx *c, int M);
void launch_fr_dense_target(mivi_ctx *c, int M, int want_grad);
void launch_rt_from_z(mivi_ctx *c, int M);
void launch_fr_stl(mivi_ctx *c, const void *params, int M, const void *rhs = nullptr, void *out = nullptr);
void launch_stein_outer(mivi_ctx *c, int M, void *A, double *gsum, int first, double scale);
void launch_stein_finish(mivi_ctx *c, double n, const double *gsum, const double *ell_sum, const void *ell_single, void *grad, void *logpi_avg);
void launch_stein_gsum(mivi_ctx *c, int M, double *gsum, int first);   // gsum (+)= G 1 (the second-order branch: no eps G^T product)
void launch_const_hess(mivi_ctx *c, void *hess);                      // hess = the built-in Gaussian targets' constant Hessian
// kernels_hess2.hip: the sample average of the Hessians of the built-in logistic-regression / funnel targets (second-order branch)
bool target_has_hess2(const mivi_ctx *c);
size_t target_hess2_bytes(const mivi_ctx *c);
bool target_hess2_begin(mivi_ctx *c);
void target_hess2_accumulate(mivi_ctx *c, int Mc);
void target_hess2_finish(mivi_ctx *c, int n_samples, void *hess);
int fr_sample_blocks(const mivi_ctx *c, int M);   // workgroups (= ell partials) of launch_fr_sample / launch_fr_dense_target: read off the tables
int fr_dense_blocks(const mivi_ctx *c, int M);    // fr_prepare built (f32; 0 if it has not)
int eps_blocks(const mivi_ctx *c, int M);

// kernels_fullrank_lds.hip (f32, d and M multiples of 64)
enum LdsReduceMode : int { R_DIAG = 0, R_DENSE_R = 1, R_DENSE_G = 2, R_PLAIN = 3 };
bool lds_path_shape_ok(const mivi_ctx *c, int M);
bool lds_prepare(mivi_ctx *c, int M);          // work lists + slab buffer for M samples per launch (false: allocation failed)
int lds_ld_blocks(const mivi_ctx *c);
int lds_eps_blocks(const mivi_ctx *c, int M);
void launch_lds_prod32(mivi_ctx *c, const void *params, int M, bool dense, int mode, void *Z, const EpsJob *next, bool want_ld,
                       bool with_dinv = false);   // with_dinv: trailing workgroups invert the 64x64 diagonal blocks of C (STL)
int lds_prod32_tiles(const mivi_ctx *c, int M);
void launch_lds_prod64(mivi_ctx *c, const void *params, int M, bool dense, int mode, void *Z, const EpsJob *next, bool want_ld);
int lds_prod64_tiles(const mivi_ctx *c, int M);
bool lds_use_prod64(const mivi_ctx *c, int M);   // large shapes: unsplit 64 x 64 tiles
int lds_prod32_eps_blocks(const mivi_ctx *c, int M);
bool lds_use_prod32(const mivi_ctx *c, int M);
// what a LaneRecorder holds, issued on c->stream for lanes 0 .. lanes - 1 (false: the lanes' recorded launches do not match; nothing was launched)
bool launch_lanes_prod(mivi_ctx *c, const LaneRecorder &rec, int lanes, int which);   // one launch for all lanes (blockIdx.y = lane); which: 0 sampling, 1 dense target
bool launch_lanes_vjp(mivi_ctx *c, const LaneRecorder &rec, int lanes);
void launch_lanes_eps(mivi_ctx *c, const LaneRecorder &rec, int lanes);              // kernels_fullrank.hip: the first draws of the lanes that made one, as one launch
bool launch_lanes_stl(mivi_ctx *c, const LaneRecorder &rec, int lanes, bool with_F);   // kernels_stl.hip: one solve launch with all lanes' jobs + one combining product
void launch_lanes_value(mivi_ctx *c, const void *params, LaneRecorder &rec);         // kernels_update.hip: the recorded closing value kernels as one launch
void launch_lds_vjp(mivi_ctx *c, const void *params, int M, const OutArgs &out, const ValueJob *self, const FusedUpdate *upd);
bool lds_stein_ok(const mivi_ctx *c, int M);
bool launch_lds_stein_outer(mivi_ctx *c, int M, void *A, double *gsum, int first, double scale, double n, void *grad, void *logpi,
                            const ValueJob *self);   // false: its tile table could not be uploaded (nothing was launched)
void invalidate_graph(mivi_ctx *c);            // api_core.hip: drop the cached hipGraphExec and the eps speculation

// kernels_fullrank_batch.hip (f32, diagonal-Gaussian target, d % 128 == 0, M % 128 == 0): L estimates at the same parameters per launch
// every workgroup of `grid` resident at once?  (loops whose workgroups exchange partials every step by spin-wait: checked at launch, never assumed)
bool grid_resident(const mivi_ctx *c, const void *kernel, int block, size_t dyn_lds, long long grid);
bool fb_shape_ok(const mivi_ctx *c, int M);
bool fb_whole_tiles(const mivi_ctx *c, int M);        // d and M multiples of 128: no padding (what the dense target, the STL term and the sharded batches need)
mivi_status_t fb_objective(mivi_ctx *c, const void *params, uint64_t idx, int lanes, int entropy, void *values);   // api_batch.hip: lanes x n_mc samples of estimate idx on the batch engine (MIVI_ERR_UNSUPPORTED: not an engine configuration)
const FbTab *fb_prepare(mivi_ctx *c, int M, int L);   // work tables for L lanes (nullptr: allocation failed)
size_t fb_plane_words(const mivi_ctx *c, int M);      // 4-byte words of one lane's operand planes (eps in one orientation, W)
size_t fb_cplane_words(const mivi_ctx *c);            // ... of tril(C)'s
void fb_launch_eps(mivi_ctx *c, const FbStep &s, bool with_cplanes, hipStream_t stream);   // a step's draws (+ tril(C)'s planes, once per call)
void fb_launch_pplanes(mivi_ctx *c, hipStream_t stream);
void fb_launch_tplanes(mivi_ctx *c, hipStream_t stream);
size_t fb_part_len(const mivi_ctx *c);                                     // floats of a lane's partial vector on the engine (a multiple of four)
void fb_launch_finalize_parts(mivi_ctx *c, const FbStep &s, hipStream_t stream);   // (summed) partial vectors -> the lanes' values and gradients
void fb_launch_compute(mivi_ctx *c, const FbStep &s, hipStream_t stream, int which = 15);  // product(s) + target -> VJP + values (which: bit 0 product, 1 VJP, 2 the dense target's product, 3 the sticking-the-landing product)

// kernels_stl.hip (f32, d in {256, 512, 1024, 2048}, M % 32 == 0)
bool stl2_shape_ok(const mivi_ctx *c, int M);
void launch_stl2(mivi_ctx *c, const void *params, int M, bool dinv_done = false, const void *rhs = nullptr, void *out = nullptr,
                 bool overwrite = false);   // rhs (ld dP) / out (ld d) default to eps / W; overwrite: out = X instead of out += X   // W += C^-T eps: dinv64 -> solve (lower half) -> update -> solve (upper half)

// kernels_targets.hip
void launch_col_target(mivi_ctx *c, int M, int want_grad);
void launch_bij_forward(mivi_ctx *c, int M);                        // Z <- binv(Z) in place, bij_ld[m] = sum_exp eta
void launch_bij_backward(mivi_ctx *c, int M, int want_grad, bool add_to_ell);   // G <- J' G + 1_exp; ell[m] += bij_ld[m]
// kernels_bijector.hip: the same two steps with truncated / ordered blocks (what the two launchers above take when c->bij_ext), and the
// inverse direction of mivi_logpdf_constrained
void launch_bijx_forward(mivi_ctx *c, int M, void *Z, void *save, void *ld);   // Z <- binv(Z) in place; save (or NULL) <- eta; ld (or NULL) <- ladj
void launch_bijx_backward(mivi_ctx *c, int M, int want_grad, bool add_to_ell);
void launch_bijx_inverse(mivi_ctx *c, int n, const void *X, void *eta, double *ladj, int *flag);   // eta <- b(X); flag: 1 outside the support, 2 NaN
void launch_bijx_finish(mivi_ctx *c, int n, void *logq, const double *ladj, const int *flag);     // logq <- logq - ladj, or -inf / NaN by flag
bool launch_logreg_target(mivi_ctx *c, int M, int want_grad);   // false: scratch allocation failed
int logreg_kernel_bits(const mivi_ctx *c, int M);         // mivi_logreg_kernels
bool logreg_uses_mfma(const mivi_ctx *c, int M);          // the matrix-core route (needs Z^T staged in RT)
bool logreg_reserve(mivi_ctx *c, int M);                        // size the scratch ahead of a graph capture
bool logreg_prepare_f32(mivi_ctx *c);   // row-major padded copy of X for the MFMA route (false: allocation failed)

// kernels_score.hip: the score-gradient (VarGrad) estimator's own kernels (api_score.hip drives them)
void launch_sg_dense_ell(mivi_ctx *c, int M);                          // sg_d[cap + m] = 0.5 r_m' g_m from Z and W = G = -P R (dense-Gaussian target)
void launch_sg_norms(mivi_ctx *c, const RngArgs &rng, int M);         // sg_d[m] = |eps_m|^2 (full-rank: from eps[0]; mean-field: redrawn from Philox)
void launch_sg_stats(mivi_ctx *c, const void *params, int M, bool ell_f64, void *value, void *elbo);   // f, mean f, weights, value, elbo, status flags
void launch_sg_scale(mivi_ctx *c, int M);                              // full-rank: sg_S = -eps diag(f - mean f) (pads zero), W = 0
void launch_sg_mf_grad(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *grad);   // mean-field: [d/dmu; d/dsigma]

// kernels_ngd.hip: KLMinSqrtNaturalGradDescent's update (klminsqrtnaturalgraddescent.jl:108-119) on [m; vec C] in place
// (both updates work in the context's one scratch pair ms_work / ms_part, which the caller ensures to the update's *_bytes before the launch;
// ngd_tile.h holds what their kernels share)
size_t ngd_work_bytes(const mivi_ctx *c);    // of c->ms_work (0: the one-workgroup kernel needs none)
size_t ngd_part_bytes(const mivi_ctx *c);    // of c->ms_part: the diagonal tiles' partials + their ticket (0: the one-workgroup kernel needs none)
void launch_ngd_update(mivi_ctx *c, void *params, const void *grad, const void *hess, double eta, const void *logpi, void *entropy, void *elbo);
// kernels_natgrad.hip: KLMinNaturalGradDescent's state (klminnaturalgraddescent.jl:83-87) and update (:129-145) on [m; vec C] and [S; Sigma] in place
size_t natgrad_work_bytes(const mivi_ctx *c);   // of c->ms_work (0: the one-workgroup kernels need none)
size_t natgrad_part_bytes(const mivi_ctx *c);   // of c->ms_part
void launch_natgrad_init(mivi_ctx *c, void *params, void *state);
// its blocked factorisation alone, on a caller's padded float64 work matrix: A = Lr' Lr, Lr (diagonal tiles included) in A's lower triangle
void launch_natgrad_factor(mivi_ctx *c, int d, double *A, double *Dinv, double *part);
// ... and the finish of an update that factored the index-reversed Sigma': C' into params, entropy(q') / elbo / flags from `part`
void launch_natgrad_factor_fin(mivi_ctx *c, const double *A, const double *part, void *params, const void *logpi, void *entropy, void *elbo);
// kernels_bam.hip: FisherMinBatchMatch (fisherminbatchmatch.jl) -- Sigma of `init` (:76), the objective (:81-111) and the update (:143-155)
size_t bam_work_bytes(const mivi_ctx *c);   // of c->ms_work (the update)
size_t bam_part_bytes(const mivi_ctx *c);   // of c->ms_part (the update)
int bam_fisher_tiles(const mivi_ctx *c, int M);   // the partials launch_bam_fisher leaves for M samples
void launch_bam_init(mivi_ctx *c, const void *params, void *state);
void launch_bam_fisher(mivi_ctx *c, const void *params, int M, const void *u, size_t ldu, const void *G, double *part);
void launch_bam_objective(mivi_ctx *c, const void *params, const double *part, int n_part, double n, const void *ell_sum, void *fisher, void *logpi_avg,
                          void *elbo);   // fisher = sum(part) / n; logpi_avg = *ell_sum / n and elbo = logpi_avg + entropy(q) where asked for
void launch_bam_update(mivi_ctx *c, void *params, void *state, const void *u, size_t ldu, const void *G, int B, double lambda, void *entropy);
void launch_natgrad_update(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double eta, int ensure_posdef, const void *logpi,
                           void *entropy, void *elbo);
// kernels_wass.hip: KLMinWassFwdBwd's update (klminwassfwdbwd.jl:105-114) on [m; vec C] and Sigma in place (its `init` state is launch_bam_init's)
size_t wass_work_bytes(const mivi_ctx *c);   // of c->ms_work
size_t wass_part_bytes(const mivi_ctx *c);   // of c->ms_part
void launch_wass_update(mivi_ctx *c, void *params, void *state, const void *grad, const void *hess, double eta, const void *logpi, void *entropy,
                        void *elbo);

// kernels_lowrank.hip: the low-rank family's estimate (api_lowrank.hip drives it)
size_t lowr_prep_doubles(int d, int r);                                        // f64 entries of c->lowr_prep
int lowr_vjp_slices(int M);                                                    // slices of the sample axis the VJP leaves partials for (<= 8)
// the Woodbury stage on points that are not the context's own draws (mivi_logpdf): t (d x cap, the element type), the prep block and the
// f64 [s; x; |t|^2; log q] block (2 r + 2) x cap, all the caller's; nullptr everywhere below: the context's lowr_V / lowr_prep / lowr_sx (cap_M)
struct LowrPoints {
  void *t;
  double *prep, *sx;
  size_t cap;
};
void launch_lowr_draw_prep(mivi_ctx *c, const RngArgs &rng, int M, const void *params, double *prep = nullptr);   // (u1; u2) of M columns -> lowr_E; params != nullptr: A^-1, sum log D, 1/2 logdet A -> prep (default lowr_prep); M = 0: the parameter half alone
void launch_lowr_sample(mivi_ctx *c, const void *params, int M, void *Z, bool with_t);   // Z = D o u1 + U u2 + m (with_t: t = u1 + D^-1 U u2 -> lowr_V)
void launch_lowr_woodbury(mivi_ctx *c, const void *params, int M, bool want_v, const LowrPoints *pts = nullptr);   // t -> s, x, log q (want_v: V over t)
double *lowr_logq_of(const mivi_ctx *c, const LowrPoints &pts);   // where launch_lowr_woodbury leaves the f64 log q of pts' columns
void launch_lowr_vjp_finish(mivi_ctx *c, const void *params, int M, int want_grad, const ValueIn &vin, const OutArgs &out);   // W = G (and V, x, the draws) -> out.grad; out.value, the non-finite flag, the elbo record

// kernels_nsf.hip: the neural spline flow's kernels; the launchers below branch to them on a context whose flow.K > 0 (launch_nsf_vjp,
// which takes the typed argument block, is declared beside FlowArgs in flow_tile.h)
bool nsf_prepare(mivi_ctx *c);
void launch_nsf_forward(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *Z, void *eps, bool save);
void launch_nsf_inverse(mivi_ctx *c, const void *params, const void *Z, int n, void *logq);
// kernels_flow.hip: the RealNVP family's estimate, rand and logpdf (api_flow.hip drives them)
long long flow_params_len(const FlowArch &a);
int flow_slices(const FlowArch &a, int M);   // slices of the sample axis the VJP leaves partials for (<= 64, and at most 256 MB of them)
bool flow_prepare(mivi_ctx *c);              // the kernels' LDS attributes, once per context (false: the runtime refused)
void launch_flow_forward(mivi_ctx *c, const void *params, const RngArgs &rng, int M, void *Z, void *eps, bool save);   // draws -> Z (eps: the draws, or nullptr); save: every x^l -> flow_X, log q -> flow_lq
void launch_flow_inverse(mivi_ctx *c, const void *params, const void *Z, int n, void *logq);   // log q at the caller's points (n <= kSampleChunk per launch)
void launch_flow_vjp_finish(mivi_ctx *c, const void *params, int M, int want_grad, const ValueIn &vin, const OutArgs &out);   // W = grad ell (and flow_X, flow_lq) -> out.grad; out.value, the non-finite flag, the elbo record

// kernels_logpdf.hip: logpdf(q, z) at the caller's points (api_logpdf.hip drives them); n <= kSampleChunk columns per launch
void launch_stl_dinv32(mivi_ctx *c, const void *params, void *DinvT);   // kernels_fullrank.hip: k_stl_prep's diagonal workgroups alone
void launch_lp_logdet(mivi_ctx *c, const void *params, double *scal);   // scal[0] = sum log C_ii (f64); the non-positive-scale flag
void launch_lp_mf(mivi_ctx *c, const void *params, const void *Z, int n, void *logq, void *std, const double *scal);
bool lp_fwd_x_in_lds(const mivi_ctx *c);   // 16 f64 columns of X fit LDS beside the solve's partials (otherwise X lives in xg, f64 d x n)
void launch_lp_fwd(mivi_ctx *c, const void *params, const void *Z, int n, const void *Dinv, void *logq, void *std, double *xg, const double *scal);
void launch_lp_lowr_t(mivi_ctx *c, const void *params, const void *Z, int n, void *tbuf);   // t = D^-1 (z - m)
void launch_lp_store(mivi_ctx *c, int n, const double *lq, void *logq);

// kernels_basedist.hip: the draw stage and the mean-field kernels of a non-normal base (api_basedist.hip drives them)
void launch_bd_draw(mivi_ctx *c, const RngArgs &rng, int M, void *U, void *UT, void *R);   // U (ld dP), UT (ld MP; or nullptr), R = -psi(U) (ld dP; or nullptr); he_part[cur]: eps_blocks partials of the variable part of -sum log phi(u)
void launch_bd_mf_sample(mivi_ctx *c, const void *params, int M, const void *U, void *Z);   // Z = sigma o U + m
void launch_bd_mf_grad(mivi_ctx *c, const void *params, int M, const void *U, const void *R, const OutArgs &out);   // W (and R / sigma) -> [dm; dsigma]

// kernels_p2p.hip: phases bit 0 push, 1 reduce + finalise, 2 unpack (7 = the whole exchange in one launch)
void launch_p2p_handover4(mivi_ctx *c, unsigned *ready, unsigned ready_val, const unsigned *const *freed, const unsigned *freed_min, int n);
void launch_p2p_exchange(mivi_ctx *c, const void *params, const void *const *P, int ring, void *value, void *grad, int phases, int lane, int lanes,
                         int count, const unsigned *ready, unsigned *freed, bool direct = false);   // one lane: estimates lane, lane + lanes, ... < count; P[t % ring]
void launch_p2p_handover(mivi_ctx *c, unsigned *ready, unsigned ready_val, const unsigned *freed, unsigned freed_min);

// kernels_update.hip
void launch_finalize(mivi_ctx *c, const void *params, const void *partials, void *value, void *grad);
void launch_finalize_slice(mivi_ctx *c, const void *params, const void *sum, long long g0, long long n, void *fin);
void launch_unpack_final(mivi_ctx *c, const void *fin, void *value, void *grad);
void launch_prox(mivi_ctx *c, void *params, double stepsize, const void *dog_state, int dog_kind);
void launch_poly_average(mivi_ctx *c, void *avg, const void *params, double avg_eta, const long long *t_ptr, long long t_base);
void launch_dog_update(mivi_ctx *c, void *params, const void *grad, void *state, int kind);
bool launch_dog_update_fused(mivi_ctx *c, void *params, const void *grad, void *state, int kind, double clip_eps, void *avg,
                             double avg_eta, const long long *t_ptr, long long t_base);
void launch_logreg_gather(mivi_ctx *c, int64_t b, const int32_t *rows = nullptr);   // batch rows lr_idx[0..b) (rows: that device list instead, a batch of the schedule) of the full data set -> lr_Xsub / lr_ysub / lr_Xrm_sub
int logreg_batch_route(const mivi_ctx *c, int M);   // a scheduled context: 1 the fused minibatch kernel (kernels_logreg_batch.hip), 2 device gather + the resident-data kernels; 0: no schedule
bool lr_batch_fits(const mivi_ctx *c, int M);       // kernels_logreg_batch.hip: a minimal slab of the fused minibatch kernel fits the LDS
bool lr_batch_prepare(mivi_ctx *c, int M);          // its LDS attribute, ahead of a capture
void launch_lr_batch(mivi_ctx *c, int M, int want_grad, const int32_t *rows, double *ll_part, void *g_part, int *n_slabs);   // ll_part[slab][M], g_part[slab][M][p]
int lr_batch_slabs(const mivi_ctx *c, int M);
void launch_value_only(mivi_ctx *c, const void *params, const ValueIn &vin, const OutArgs &out);   // on c->stream
void launch_clip(mivi_ctx *c, void *params, double epsilon);
void launch_descent(mivi_ctx *c, void *params, const void *grad, double eta, double clip_eps = NAN);   // NaN: no ClipScale
void launch_adam(mivi_ctx *c, void *params, const void *grad, void *state, const int64_t *t_ptr, int64_t t_base,
                 double eta, double b1, double b2, double eps, double clip_eps = NAN);
void launch_cocob(mivi_ctx *c, void *params, const void *grad, void *state, double alpha, double clip_eps = (double)NAN);
void launch_bump(mivi_ctx *c, uint64_t *ctr, uint64_t by);

}  // namespace mivi
