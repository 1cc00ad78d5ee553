// libmivi C ABI (include/mivi.h), part 1: context management, target / bijector set-up, small setters, the host-side RNG restatement.
// Reference call stack being replaced: SURVEY.md section 3.2 (estimate_gradient! -> _value_and_gradient! -> AD of
// estimate_repgradelbo_ad_forward).  The other parts: api_estimate.hip (one estimate), api_batch.hip (estimates at fixed
// parameters), api_objective.hip (estimate_objective, the Gaussian-expectation gradient / Hessian), api_dist.hip (sharded
// estimates), api_optimize.hip (update rules, the device-resident loop), api_profile.hip (per-kernel timing entries),
// api_graph.hip (hipGraph capture, the context's graph cache and its replay).
#include <atomic>
#include <climits>
#include <cstddef>
#include <cstdlib>

#include "api_common.h"

// ---- one-thread kernels shared by the api_*.hip units (declared in api_common.h) ----
// weighted accumulation of chunk objective values
__global__ void k_acc_value_f32(double *acc, const float *v, double w, int first) { acc[0] = (first ? 0.0 : acc[0]) + w * (double)v[0]; }
__global__ void k_acc_value_f64(double *acc, const double *v, double w, int first) { acc[0] = (first ? 0.0 : acc[0]) + w * v[0]; }
__global__ void k_store_value_f32(float *out, const double *acc) { out[0] = (float)acc[0]; }
// acc = w * sum of n values (objective mode of the batch engine: the lanes' values), a fixed order: thread t sums entries t, t + 256, .. in
// f64, the 256 partials are added in index order by thread 0
__global__ __launch_bounds__(256) void k_mean_values_f32(double *acc, const float *v, int n, double w) {
  __shared__ double part[256];
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += 256) s += (double)v[i];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    double t = 0.0;
    for (int i = 0; i < 256; ++i) t += part[i];
    acc[0] = w * t;
  }
}
__global__ void k_store_value_f64(double *out, const double *acc) { out[0] = acc[0]; }
// device counters of the graph-batched calls, set BY VALUE (an async copy from a stack local may outlive the caller's frame)
__global__ void k_set_u64x2(uint64_t *dst, uint64_t a, uint64_t b, int n) { dst[0] = a; if (n > 1) dst[1] = b; }
__global__ void k_bump_u64(uint64_t *dst, uint64_t by) { dst[0] += by; }
// latency floor (mivi_profile_kernel which = 9): a kernel that does nothing, launched with the grid / block / LDS footprint of a real one
__global__ void k_empty(int *sink) {
  extern __shared__ int lds_dyn[];
  if (sink && threadIdx.x == 0 && blockIdx.x == 0x7fffffff) sink[0] = lds_dyn[0];
}


mivi_status_t fail(mivi_ctx *c, mivi_status_t s, const char *msg) {
  if (c) c->err = msg;
  return s;
}

// ---- the environment switches (switches.h): this table is the one place where libmivi reads the environment ----
namespace mivi {
namespace {
enum SwitchKind {
  SW_PRESENCE,      // bool: set to anything (also "0") = on
  SW_ON_UNLESS_0,   // bool: on; "=0" (atoi) turns it off
  SW_OFF_UNLESS_1,  // bool: off; "=1" (atoi) turns it on
  SW_INT,           // int: atoi of the value, `def` when unset, clamped to lo .. hi
  SW_STRING         // const char *: the value itself, nullptr when unset
};
constexpr int kNoLo = INT_MIN, kNoHi = INT_MAX;
struct SwitchRow { const char *name; SwitchKind kind; size_t field; int def, lo, hi; const char *meaning; };
#define SW(f) offsetof(Switches, f)
const SwitchRow kSwitchTable[] = {
    {"MIVI_FR_GEN1", SW_PRESENCE, SW(fr_gen1), 0, 0, 0, "full-rank f32: first-generation tile kernels at every shape (lds_path_shape_ok)"},
    {"MIVI_STEIN_GEN1", SW_PRESENCE, SW(stein_gen1), 0, 0, 0, "Stein accumulation stage on the first-generation kernel (lds_stein_ok)"},
    {"MIVI_STL_GEN1", SW_PRESENCE, SW(stl_gen1), 0, 0, 0, "sticking-the-landing solve: not the second-generation packed solve (stl2_shape_ok)"},
    {"MIVI_STL_VALU", SW_PRESENCE, SW(stl_valu), 0, 0, 0, "first-generation solve on the vector ALU, not the 16-column look-ahead solve (launch_fr_stl)"},
    {"MIVI_LR_F32_LOGITS", SW_PRESENCE, SW(lr_f32_logits), 0, 0, 0, "logistic regression: f32-MFMA logits kernel (the one d % 4 != 0 takes), no operand planes"},
    {"MIVI_LR_NO_PLANES", SW_PRESENCE, SW(lr_no_planes), 0, 0, 0, "logistic regression: logits with X split in the tile (k_lr_logits_f16x2)"},
    {"MIVI_LR_NO_XPLANES", SW_PRESENCE, SW(lr_no_xplanes), 0, 0, 0, "logistic regression: X^T R with the splits made in the tile (k_lr_xtr_f16x2)"},
    {"MIVI_NO_FUSED_LOOP", SW_PRESENCE, SW(no_fused_loop), 0, 0, 0, "no launch-free loop kernels: batches and optimisation loops as graphs of launches"},
    {"MIVI_NO_FUSED_UPDATE", SW_PRESENCE, SW(no_fused_update), 0, 0, 0, "graph loop: the optimiser step as a kernel of its own, not in the VJP epilogue"},
    {"MIVI_FORCE_EXCHANGE_LOST", SW_PRESENCE, SW(force_exchange_lost), 0, 0, 0, "test hook (tests/test_gpu_loop_oracle.py): the first exchanging loop call counts as lost"},
    {"MIVI_BATCH_GEN3", SW_ON_UNLESS_0, SW(batch_gen3), 0, 0, 0, "=0: batches off the third-generation engine, on the lane-batched second-generation kernels"},
    {"MIVI_FB_STL", SW_ON_UNLESS_0, SW(fb_stl), 0, 0, 0, "=0: sticking-the-landing batches off the engine (lane-batched kernels + solves)"},
    {"MIVI_PROD_QUAD", SW_ON_UNLESS_0, SW(prod_quad), 0, 0, 0, "=0: four lanes' sampling products as k_fr_prod32m tiles, not k_fr_prod32q"},
    {"MIVI_P2P_DIRECT", SW_OFF_UNLESS_1, SW(p2p_direct), 0, 0, 0, "=1: sharded partials staged straight into the peers' buffers (mivi_p2p_partials_direct)"},
    {"MIVI_GRAPH_MIN", SW_INT, SW(graph_min), 6, kNoLo, kNoHi, "smallest full-rank batch that is captured as a graph (shorter: an eager chain)"},
    {"MIVI_CHAINS", SW_INT, SW(chains), 0, kNoLo, kNoHi, "> 0: that many interleaved contexts per batch (0: by shape)"},
    {"MIVI_FB_LANES", SW_INT, SW(fb_lanes), 80, 1, 256, "estimates per step of the batch engine"},
    {"MIVI_LANE_BATCH", SW_INT, SW(lane_batch), -1, kNoLo, kNoHi, "contexts per graph branch: 0 = every context on a branch of its own, 1 .. 4, < 0 = by shape"},
    {"MIVI_VJP_STRIP", SW_INT, SW(vjp_strip), 3, 0, 32, "tiles per workgroup of the lane-batched VJP (k_fr_vjp32s); 0 = one each (k_fr_vjp32m)"},
    {"MIVI_VJP_TILE", SW_INT, SW(vjp_tile), 0, kNoLo, kNoHi, "32 / 64 pins the second-generation VJP's tile size (0: by shape)"},
    {"MIVI_RCCL_LIB", SW_STRING, SW(rccl_lib), 0, 0, 0, "path of the RCCL library to load (unset: the loader's search)"},
#ifdef MIVI_DEV
    {"MIVI_FB_DBG", SW_PRESENCE, SW(fb_dbg), 0, 0, 0, "batch engine: per-workgroup clock stamps, summarised on stderr"},
    {"MIVI_STL_STAMPS", SW_PRESENCE, SW(stl_stamps), 0, 0, 0, "second-generation solve: per-block clock stamps on stderr"},
    {"MIVI_FB_KNOCK", SW_INT, SW(fb_knock), 0, kNoLo, kNoHi, "batch engine: work-skipping bits (operand loads / MFMAs / epilogue / stores)"},
    {"MIVI_FB_RING", SW_INT, SW(fb_ring), 0, kNoLo, kNoHi, "4 / 8 pins the engine product's ring depth (tools/fb_lane_curve.py)"},
    {"MIVI_KNOCK", SW_INT, SW(knock), 0, kNoLo, kNoHi, "second-generation kernels: work-skipping bits"},
#endif
};
#undef SW
Switches read_switches() {
  Switches s{};
  for (const SwitchRow &r : kSwitchTable) {
    const char *v = getenv(r.name);
    void *f = (char *)&s + r.field;
    switch (r.kind) {
      case SW_PRESENCE: *(bool *)f = v != nullptr; break;
      case SW_ON_UNLESS_0: *(bool *)f = !(v && atoi(v) == 0); break;
      case SW_OFF_UNLESS_1: *(bool *)f = v && atoi(v) == 1; break;
      case SW_INT: { const int x = v ? atoi(v) : r.def; *(int *)f = x < r.lo ? r.lo : (x > r.hi ? r.hi : x); break; }
      case SW_STRING: *(const char **)f = v; break;
    }
  }
  return s;
}
}  // namespace
const Switches &switches() {
  static const Switches s = read_switches();
  return s;
}

bool grid_resident(const mivi_ctx *c, const void *kernel, int block, size_t dyn_lds, long long grid) {
  int nb = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, kernel, block, dyn_lds) != hipSuccess) { (void)hipGetLastError(); return false; }
  return c->n_cu > 0 && (long long)nb * c->n_cu >= grid;
}
}  // namespace mivi

// ---- the library's device memory: ensure allocates, DevBuf::release frees, and nothing else in libmivi does either ----
static std::atomic<int32_t> g_live_allocations{0};   // allocations held in this process (mivi_batch_info what = 5)
int32_t live_allocations() { return g_live_allocations.load(); }

void mivi::DevBuf::release() {
  if (owned && p) { (void)hipFree(p); --g_live_allocations; }
  p = nullptr; bytes = 0; owned = false;
}

mivi_status_t ensure(mivi_ctx *c, DevBuf &b, size_t bytes, bool zero, bool fine_grained) {
  if (b.bytes >= bytes && b.p) return MIVI_OK;
  b.release();
  if (bytes == 0) bytes = 16;
  void *p = nullptr;
  HIPCHK(c, fine_grained ? hipExtMallocWithFlags(&p, bytes, hipDeviceMallocFinegrained) : hipMalloc(&p, bytes));
  ++g_live_allocations;
  b.p = p; b.bytes = bytes; b.owned = true;
  if (zero) HIPCHK(c, hipMemsetAsync(b.p, 0, bytes, c->stream));
  return MIVI_OK;
}

mivi_status_t ensure_zeroed(mivi_ctx *c, DevBuf &b, size_t bytes) {
  if (mivi_status_t s = ensure(c, b, bytes, false)) return s;
  HIPCHK(c, hipMemsetAsync(b.p, 0, bytes ? bytes : b.bytes, c->stream));
  return MIVI_OK;
}

mivi_status_t upload(mivi_ctx *c, DevBuf &b, const void *src, size_t bytes) {
  if (mivi_status_t s = ensure(c, b, bytes, false)) return s;
  HIPCHK(c, hipMemcpy(b.p, src, bytes, hipMemcpyHostToDevice));
  return MIVI_OK;
}

// ---- the library's streams and events: make_stream / make_event create, handle_destroy destroys, and nothing else in libmivi does either ----
static std::atomic<int32_t> g_live_handles{0};   // streams, events and graph execs held in this process (mivi_batch_info what = 6)
int32_t live_handles() { return g_live_handles.load(); }
void mivi::count_handles(int delta) { g_live_handles += delta; }
void mivi::handle_destroy(hipStream_t h) { (void)hipStreamDestroy(h); }
void mivi::handle_destroy(hipEvent_t h) { (void)hipEventDestroy(h); }

mivi_status_t make_stream(mivi_ctx *c, Stream &s, bool own_queue) {
  hipStream_t h = nullptr;
  uint32_t mask[16];   // all CUs enabled = no restriction: the mask is there for the queue it brings
  for (int k = 0; k < 16; ++k) mask[k] = 0xFFFFFFFFu;
  if (own_queue && c->stream != nullptr && hipExtStreamCreateWithCUMask(&h, 16, mask) != hipSuccess) {
    (void)hipGetLastError();
    h = nullptr;
  }
  if (!h) HIPCHK(c, hipStreamCreateWithFlags(&h, hipStreamNonBlocking));
  s.adopt(h);
  return MIVI_OK;
}

mivi_status_t make_event(mivi_ctx *c, Event &e, bool timing) {
  hipEvent_t h = nullptr;
  HIPCHK(c, timing ? hipEventCreate(&h) : hipEventCreateWithFlags(&h, hipEventDisableTiming));
  e.adopt(h);
  return MIVI_OK;
}

mivi_status_t ensure_pipe(mivi_ctx *c, ExchangePipe &p, bool own_queue) {
  if (p) return MIVI_OK;
  ExchangePipe made;   // (a failed attempt destroys what it made and leaves p empty: the next call tries again)
  mivi_status_t s = make_stream(c, made.stream, own_queue);
  for (int k = 0; k < 2 && s == MIVI_OK; ++k)
    if (!(s = make_event(c, made.part[k], false))) s = make_event(c, made.done[k], false);
  if (s == MIVI_OK) p = std::move(made);
  return s;
}

// A captured graph bakes buffer pointers, leading dimensions and work-list contents; the eps speculation remembers a buffer
// parity.  Anything that reallocates or rewrites those calls this.
namespace mivi {
void invalidate_graph(mivi_ctx *c) {
  c->pre.clear();
  ++c->target_gen;
  c->graph.drop();
}
}  // namespace mivi

// work buffers for up to M samples per launch
mivi_status_t ensure_work(mivi_ctx *c, int M) {
  const int d = c->cfg.d;
  const size_t es = c->esize;
  mivi_status_t s;
  if (M > c->cap_M) {
    invalidate_graph(c);   // the work buffers below are reallocated and MP / dP change under any cached graph
    // a capacity change re-zeros the padded RNG buffers (their padding must stay 0 / finite)
    const int capM = round_up(M, 64);
    c->dP = round_up(d, 64);
    c->MP = capM;
    const int d4 = (d + 3) / 4;
    // per-workgroup ell partials: the XCD-interleaved work tables have up to 8*ceil(nb/8)*ncb slots
    size_t n_part = 8 * (size_t)(((d + 31) / 32 + 7) / 8) * (size_t)((capM + 31) / 32) + 64;
    size_t n_he = (size_t)((d + 15) / 16) * (size_t)(capM / 64 + 1);
    const size_t n_he_mf = (size_t)((d4 + 255) / 256) * (size_t)capM;
    if (n_he_mf > n_he) n_he = n_he_mf;
    const size_t ncc = (size_t)(capM / 256 + 2);
    for (int b = 0; b < 2; ++b) {
      if (c->cfg.family == MIVI_FULLRANK) {
        if ((s = ensure_zeroed(c, c->eps[b], (size_t)c->dP * c->MP * es))) return s;
        if ((s = ensure_zeroed(c, c->epsT[b], (size_t)c->dP * c->MP * es))) return s;
      }
      if ((s = ensure(c, c->ell_part[b], n_part * sizeof(double), false))) return s;
      if ((s = ensure(c, c->he_part[b], (n_he + 64) * sizeof(double), false))) return s;
      if ((s = ensure(c, c->sc_part[b], 6 * ncc * d4 * sizeof(double) + 64, false))) return s;
      if ((s = ensure(c, c->ld_part[b], 2 * (size_t)((d + 31) / 32) * sizeof(double) + 64, false))) return s;
    }
    if (c->target == TGT_DENSE_GAUSS || (c->target == TGT_LOGREG && c->cfg.dtype == MIVI_F32)) {
      if ((s = ensure_zeroed(c, c->RT, (size_t)c->dP * c->MP * es))) return s;
    }
    if (c->cfg.family == MIVI_FULLRANK && (c->cfg.entropy == MIVI_ENT_STL || c->cfg.entropy == MIVI_ENT_STL_ZERO_GRAD)) {
      if ((s = ensure(c, c->stl_CT, (size_t)c->dP * c->dP * es, true))) return s;
      if ((s = ensure(c, c->stl_Dinv, (size_t)((d + 63) / 64) * 4096 * es, false))) return s;   // 32x32 or 64x64 diagonal inverses
      if ((s = ensure(c, c->stl_X, ((size_t)d * capM + (size_t)(d / 2) * (d / 2)) * es + 4096, false))) return s;   // X2, Y1, F (kernels_stl.hip)
      if (d % 128 == 0 && (s = ensure(c, c->stl_F, mivi::stl_pack_units(d) * 4, false))) return s;   // + developer stamp page (MIVI_STL_STAMPS)
    }
    if (c->cfg.family == MIVI_LOWRANK && (s = ensure_work_lowrank(c, capM))) return s;
    if (is_flow(c) && (s = ensure_work_flow(c, capM))) return s;
    if (c->base != MIVI_BASE_NORMAL && (s = ensure_work_base(c, capM))) return s;
    if ((s = ensure(c, c->Z, (size_t)d * capM * es, false))) return s;
    if ((s = ensure(c, c->W, (size_t)d * capM * es, false))) return s;
    if ((s = ensure(c, c->ell, (size_t)capM * es, false))) return s;
    if (c->bij_on && (s = ensure(c, c->bij_ld, (size_t)capM * es, false))) return s;
    if (c->bij_on && c->bij_ext && (s = ensure(c, c->bij_eta, (size_t)d * capM * es, false))) return s;   // eta for the backward pass
    if ((s = ensure(c, c->row_part, ncc * d4 * 8 * sizeof(double), false))) return s;
    c->cap_M = capM;
  }
  return MIVI_OK;
}


int32_t mivi_version(void) { return MIVI_VERSION_MAJOR * 1000 + MIVI_VERSION_MINOR; }

const char *mivi_last_error(const mivi_ctx_t *ctx) { return ctx ? ctx->err.c_str() : "null context"; }

int64_t mivi_params_len(const mivi_ctx_t *c) {
  const int64_t d = c->cfg.d;
  if (c->cfg.family == MIVI_LOWRANK) return 2 * d + d * (int64_t)c->cfg.rank;
  if (is_flow(c)) return flow_params_len(c->flow);
  return c->cfg.family == MIVI_MEANFIELD ? 2 * d : d + d * d;
}
int64_t mivi_partials_len(const mivi_ctx_t *c) {
  const int64_t d = c->cfg.d;
  if (c->cfg.family == MIVI_LOWRANK || is_flow(c)) return 0;   // no sharded estimates
  return (c->cfg.family == MIVI_MEANFIELD ? 2 * d : d + d * (d + 1) / 2) + 2;
}

mivi_status_t mivi_create(const mivi_config_t *cfg, mivi_ctx_t **out) {
  if (cfg && cfg->family == MIVI_REALNVP) {
    fprintf(stderr, "libmivi: mivi_create: the RealNVP family (MIVI_REALNVP) takes its architecture through mivi_create_flow\n");
    return MIVI_ERR_BAD_ARG;
  }
  if (cfg && cfg->family == MIVI_NSF) {
    fprintf(stderr, "libmivi: mivi_create: the neural spline flow family (MIVI_NSF) takes its architecture through mivi_create_spline_flow\n");
    return MIVI_ERR_BAD_ARG;
  }
  return create_context(cfg, nullptr, out);
}

// mivi_create, and mivi_create_flow (api_flow.hip) behind its own checks: `flow` is the architecture of a MIVI_REALNVP context
mivi_status_t create_context(const mivi_config_t *cfg, const mivi::FlowArch *flow, mivi_ctx_t **out) {
  if (!cfg || !out) return MIVI_ERR_BAD_ARG;
  if (cfg->d <= 0 || cfg->n_mc <= 0) return MIVI_ERR_BAD_ARG;
  if (cfg->dtype != MIVI_F32 && cfg->dtype != MIVI_F64) return MIVI_ERR_BAD_ARG;
  if (cfg->family != MIVI_MEANFIELD && cfg->family != MIVI_FULLRANK && cfg->family != MIVI_LOWRANK && !((cfg->family == MIVI_REALNVP || cfg->family == MIVI_NSF) && flow)) return MIVI_ERR_BAD_ARG;
  if (cfg->family == MIVI_LOWRANK) {   // (rank is read for this family only)
    if (cfg->rank < 1 || cfg->rank > MIVI_LOWRANK_MAX_RANK) return MIVI_ERR_BAD_ARG;
    if (cfg->m_offset != 0 || (cfg->m_total != 0 && cfg->m_total != cfg->n_mc)) return MIVI_ERR_UNSUPPORTED;   // no sharded low-rank estimates
  }
  if (cfg->entropy < 0 || cfg->entropy > MIVI_ENT_STL_ZERO_GRAD) return MIVI_ERR_BAD_ARG;
  if (cfg->m_offset < 0) return MIVI_ERR_BAD_ARG;
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0 || cfg->device < 0 || cfg->device >= ndev) {
    fprintf(stderr, "libmivi: no usable HIP device %d (found %d): this library has no CPU fallback\n", cfg->device, ndev);
    return MIVI_ERR_HIP;
  }
  mivi_ctx *c = new mivi_ctx();
  c->cfg = *cfg;
  if (flow) c->flow = *flow;
  c->esize = cfg->dtype == MIVI_F32 ? 4 : 8;
  {
    int v = 0;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, cfg->device) == hipSuccess && v > 0) c->n_cu = v;
    if (hipDeviceGetAttribute(&v, hipDeviceAttributeMaxSharedMemoryPerBlock, cfg->device) == hipSuccess && v > 0) c->lds_max = (size_t)v;
    (void)hipGetLastError();
  }
  c->M_total = cfg->m_total > 0 ? cfg->m_total : cfg->n_mc;
  if (hipSetDevice(cfg->device) != hipSuccess) { delete c; return MIVI_ERR_HIP; }
  mivi_status_t s;
  if (!cfg->own_stream) {
    c->stream = (hipStream_t)cfg->stream;   // NULL = the null stream
  } else {
    if ((s = make_stream(c, c->own, false))) { delete c; return s; }
    c->stream = c->own.get();
  }
  if ((s = ensure(c, c->status, 64, true)) ||
      (s = ensure(c, c->d_idx, 64, true)) || (s = ensure(c, c->acc, 64, true)) ||
      (s = ensure(c, c->dog_part, (2 * 512 + 8) * sizeof(double), true)) ||
      (s = ensure(c, c->tmp_params, (size_t)mivi_params_len(c) * c->esize, false)) ||
      (s = ensure(c, c->tmp_out, ((size_t)mivi_params_len(c) + 16) * c->esize, false))) {
    delete c;
    return s;
  }
  *out = c;
  return MIVI_OK;
}

mivi_status_t mivi_destroy(mivi_ctx_t *c) {
  if (!c) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  (void)hipStreamSynchronize(c->stream);
  for (int j = 0; j < c->n_kids; ++j) (void)mivi_destroy(c->kids[j]);   // (before their views of this context's buffers dangle)
  delete c;
  return MIVI_OK;
}

mivi_status_t mivi_set_stream(mivi_ctx_t *c, void *s) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (c->own) { (void)hipStreamSynchronize(c->own.get()); c->own.reset(); }
  c->stream = (hipStream_t)s;   // NULL = the null stream
  c->pre.clear();
  c->graph.drop();   // (not invalidate_graph: the children's generation stays)
  return MIVI_OK;
}


// waits for the context's stream and reports (then clears) the sticky device flags of the estimates since the last read
mivi_status_t mivi_synchronize(mivi_ctx_t *c) {
  if (!c) return MIVI_ERR_BAD_ARG;
  return read_status(c);
}

// ---------------------------------------------------------------------------------------------
// targets
// ---------------------------------------------------------------------------------------------
double host_get(const void *p, int dtype, size_t i) {
  return dtype == MIVI_F32 ? (double)((const float *)p)[i] : ((const double *)p)[i];
}
static mivi_status_t upload_vec(mivi_ctx *c, DevBuf &b, const std::vector<double> &v) {
  if (c->cfg.dtype != MIVI_F32) return upload(c, b, v.data(), v.size() * 8);
  const std::vector<float> f(v.begin(), v.end());
  return upload(c, b, f.data(), f.size() * 4);
}

mivi_status_t mivi_set_target_diag_gauss(mivi_ctx_t *c, const void *mean, const void *stdv) {
  if (!c || !mean || !stdv) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int d = c->cfg.d;
  std::vector<double> m(d), is(d);
  double cst = -0.5 * d * kLog2Pi;
  for (int i = 0; i < d; ++i) {
    const double s = host_get(stdv, c->cfg.dtype, i);
    if (!(s > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "diag_gauss: std must be positive");
    m[i] = host_get(mean, c->cfg.dtype, i);
    is[i] = 1.0 / s;
    cst -= log(s);
  }
  mivi_status_t s;
  if ((s = upload_vec(c, c->t_mean, m)) || (s = upload_vec(c, c->t_istd, is))) return s;
  c->t_const = cst;
  c->target = TGT_DIAG_GAUSS;
  invalidate_graph(c);
  return MIVI_OK;
}

mivi_status_t mivi_set_target_dense_gauss(mivi_ctx_t *c, const void *mean, const void *Lh) {
  if (!c || !mean || !Lh) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int d = c->cfg.d;
  const int dP = round_up(d, 64);
  std::vector<double> L((size_t)d * d, 0.0), Li((size_t)d * d, 0.0), m(d);
  double logdet = 0.0;
  for (int j = 0; j < d; ++j)
    for (int i = j; i < d; ++i) L[(size_t)j * d + i] = host_get(Lh, c->cfg.dtype, (size_t)j * d + i);
  for (int i = 0; i < d; ++i) {
    m[i] = host_get(mean, c->cfg.dtype, i);
    const double lii = L[(size_t)i * d + i];
    if (!(lii > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "dense_gauss: Cholesky diagonal must be positive");
    logdet += 2.0 * log(lii);
  }
  // Li = L^-1 (lower), column by column (forward substitution), fp64 on the host
  for (int j = 0; j < d; ++j) {
    Li[(size_t)j * d + j] = 1.0 / L[(size_t)j * d + j];
    for (int i = j + 1; i < d; ++i) {
      double s = 0.0;
      for (int k = j; k < i; ++k) s += L[(size_t)k * d + i] * Li[(size_t)j * d + k];
      Li[(size_t)j * d + i] = -s / L[(size_t)i * d + i];
    }
  }
  // P = Li^T Li, padded to dP x dP (zeros)
  std::vector<double> P((size_t)dP * dP, 0.0);
  for (int i = 0; i < d; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = 0.0;
      for (int k = i; k < d; ++k) s += Li[(size_t)i * d + k] * Li[(size_t)j * d + k];
      P[(size_t)j * dP + i] = s;
      P[(size_t)i * dP + j] = s;
    }
  mivi_status_t s;
  if ((s = upload_vec(c, c->t_mean, m)) || (s = upload_vec(c, c->t_prec, P))) return s;
  c->t_const = -0.5 * logdet - 0.5 * d * kLog2Pi;
  c->target = TGT_DENSE_GAUSS;
  c->fb.PA_valid = false;   // (the batch engine's planes of P)
  c->cap_M = 0;  // force (re)allocation of RT
  invalidate_graph(c);
  return MIVI_OK;
}

mivi_status_t mivi_set_target_logreg(mivi_ctx_t *c, const void *X, const uint8_t *y, int64_t n, int32_t variant,
                                     double likeadj, int32_t on_device) {
  if (!c || !X || !y || n <= 0 || (variant != 0 && variant != 1) || c->cfg.d < 2) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int p = c->cfg.d - 1;
  if (on_device) {
    c->lr_X = X;
    c->lr_y = y;
  } else {
    mivi_status_t s;
    if ((s = ensure(c, c->lr_X_own, (size_t)n * p * c->esize, false)) || (s = ensure(c, c->lr_y_own, (size_t)n, false)))
      return s;
    HIPCHK(c, hipMemcpy(c->lr_X_own.p, X, (size_t)n * p * c->esize, hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(c->lr_y_own.p, y, (size_t)n, hipMemcpyHostToDevice));
    c->lr_X = c->lr_X_own.p;
    c->lr_y = (const uint8_t *)c->lr_y_own.p;
  }
  c->lr_n = n;
  c->lr_variant = variant;
  c->lr_likeadj = likeadj;
  c->lr_X_full = c->lr_X;
  c->lr_y_full = c->lr_y;
  c->lr_n_full = n;
  c->lr_likeadj_full = likeadj;
  c->lr_sched_n = c->lr_sched_k = 0;   // (a schedule of batches named rows of the previous data set)
  c->t_const = 0.0;
  c->target = TGT_LOGREG;
  c->cap_M = 0;   // (re)allocate the transposed-sample buffer
  if (c->cfg.dtype == MIVI_F32 && !logreg_prepare_f32(c)) return fail(c, MIVI_ERR_HIP, "logistic regression: row-major copy allocation failed");
  c->lr_Xrm_act = c->cfg.dtype == MIVI_F32 ? c->lr_Xrm.p : nullptr;
  invalidate_graph(c);
  return MIVI_OK;
}

// the gathered copy of a batch of b rows (launch_logreg_gather): both orientations for f32; then the active fields on it
static mivi_status_t ensure_batch_copy(mivi_ctx *c, int64_t b) {
  const int p = c->cfg.d - 1;
  mivi_status_t s;
  if ((s = ensure(c, c->lr_Xsub, (size_t)b * p * c->esize, false)) || (s = ensure(c, c->lr_ysub, (size_t)b, false))) return s;
  if (c->cfg.dtype == MIVI_F32 && (s = ensure(c, c->lr_Xrm_sub, (size_t)((b + 15) / 16 * 16) * ((p + 31) / 32 * 32) * sizeof(float), false))) return s;
  return MIVI_OK;
}
static void point_at_batch_copy(mivi_ctx *c, int64_t b, double likeadj) {
  c->lr_X = c->lr_Xsub.p;
  c->lr_y = (const uint8_t *)c->lr_ysub.p;
  c->lr_n = b;
  c->lr_likeadj = likeadj;
  c->lr_Xrm_act = c->cfg.dtype == MIVI_F32 ? c->lr_Xrm_sub.p : nullptr;
}

mivi_status_t mivi_logreg_select_rows(mivi_ctx_t *c, const int64_t *idx, int64_t b, double likeadj) {
  if (!c || b < 0 || (b > 0 && !idx)) return MIVI_ERR_BAD_ARG;
  if (c->target != TGT_LOGREG || !c->lr_X_full) return fail(c, MIVI_ERR_NO_TARGET, "no logistic-regression target set");
  (void)hipSetDevice(c->cfg.device);
  if (b > 0) {   // (checked before anything changes: a failed call leaves the previous selection -- rows or a schedule -- in force)
    if (!(likeadj > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive");
    for (int64_t j = 0; j < b; ++j)
      if (idx[j] < 0 || idx[j] >= c->lr_n_full) return fail(c, MIVI_ERR_BAD_ARG, "batch row index out of range");
  }
  invalidate_graph(c);
  c->lr_sched_n = c->lr_sched_k = 0;   // the row selection replaces a schedule of batches
  if (b == 0) {   // back to the full data set
    c->lr_X = c->lr_X_full;
    c->lr_y = c->lr_y_full;
    c->lr_n = c->lr_n_full;
    c->lr_likeadj = c->lr_likeadj_full;
    c->lr_Xrm_act = c->cfg.dtype == MIVI_F32 ? c->lr_Xrm.p : nullptr;
    return MIVI_OK;
  }
  mivi_status_t s;
  if ((s = ensure(c, c->lr_idx, (size_t)b * sizeof(int64_t), false)) || (s = ensure_batch_copy(c, b))) return s;
  // the previous estimate may still be reading the batch buffers: order the upload behind it
  HIPCHK(c, hipStreamSynchronize(c->stream));
  HIPCHK(c, hipMemcpy(c->lr_idx.p, idx, (size_t)b * sizeof(int64_t), hipMemcpyHostToDevice));
  launch_logreg_gather(c, b);
  HIPCHK(c, hipGetLastError());
  point_at_batch_copy(c, b, likeadj);
  return MIVI_OK;
}

// ---- a schedule of minibatches resident on the device (include/mivi.h) ----
// THE guard of every entry that reads the logistic regression's data set outside launch_logreg_target (the Hessian, measure-space, score,
// partials / sharded / peer-to-peer and profile entries: refuse_non_gaussian reaches it for them): on a scheduled context the active
// fields name the gather buffers, which hold whatever batch was gathered last.  Call it before reading a buffer.
mivi_status_t refuse_batch_schedule(mivi_ctx *c, const char *entry) {
  if (c->lr_sched_n <= 0) return MIVI_OK;
  c->err = std::string(entry) + ": not supported while a schedule of minibatches is set (mivi_logreg_set_batch_schedule): select the rows with mivi_logreg_select_rows";
  return MIVI_ERR_UNSUPPORTED;
}

mivi_status_t mivi_logreg_set_batch_schedule(mivi_ctx_t *c, const mivi_batch_schedule_t *sp) {
  if (!c || !sp) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_flow(c, "mivi_logreg_set_batch_schedule")) return rs;
  if (c->target != TGT_LOGREG || !c->lr_X_full) return fail(c, MIVI_ERR_NO_TARGET, "no logistic-regression target set");
  const mivi_batch_schedule_t &sc = *sp;
  if (sc.n_batches < 0 || sc.kernels < 0 || sc.kernels > 2) return fail(c, MIVI_ERR_BAD_ARG, "batch schedule: n_batches >= 0 and kernels in 0 .. 2");
  if (sc.n_batches == 0) return mivi_logreg_select_rows(c, nullptr, 0, 1.0);
  if (!sc.rows_host) return MIVI_ERR_BAD_ARG;
  if (sc.batch < 1 || sc.batch > INT32_MAX) return fail(c, MIVI_ERR_BAD_ARG, "batch schedule: a batch has at least one row");
  if (!(sc.likeadj > 0.0)) return fail(c, MIVI_ERR_BAD_ARG, "likelihood adjustment must be positive");
  if (c->lr_n_full > INT32_MAX) return fail(c, MIVI_ERR_UNSUPPORTED, "batch schedule: the rows are kept as int32");
  const size_t total = (size_t)sc.n_batches * (size_t)sc.batch;
  std::vector<int32_t> rows(total);
  for (size_t j = 0; j < total; ++j) {
    if (sc.rows_host[j] < 0 || sc.rows_host[j] >= c->lr_n_full) return fail(c, MIVI_ERR_BAD_ARG, "batch row index out of range");
    rows[j] = (int32_t)sc.rows_host[j];
  }
  (void)hipSetDevice(c->cfg.device);
  const bool has_idx = sc.estimate_idx_host != nullptr;
  const void *was[5] = {c->lr_sched_rows.p, c->lr_sched_idx.p, c->lr_Xsub.p, c->lr_ysub.p, c->lr_Xrm_sub.p};
  mivi_status_t s;
  if ((s = ensure(c, c->lr_sched_rows, total * sizeof(int32_t), false)) || (has_idx && (s = ensure(c, c->lr_sched_idx, (size_t)sc.n_batches * sizeof(uint64_t), false))) ||
      (s = ensure_batch_copy(c, sc.batch))) {
    (void)mivi_logreg_select_rows(c, nullptr, 0, 1.0);   // (a buffer of the previous selection may be gone: the full data set)
    return s;
  }
  const void *now[5] = {c->lr_sched_rows.p, c->lr_sched_idx.p, c->lr_Xsub.p, c->lr_ysub.p, c->lr_Xrm_sub.p};
  // a recorded loop walks rows + k * batch and the index table by address: it stays valid when a schedule of the same shape replaces one
  // in place (a chunked driver), everything else re-records
  const bool in_place = c->lr_sched_n > 0 && c->lr_sched_k == 0 && c->lr_n == sc.batch && c->lr_sched_kernels == sc.kernels && c->lr_likeadj == sc.likeadj &&
                        c->lr_sched_has_idx == has_idx && memcmp(was, now, sizeof(was)) == 0;
  if (!in_place) invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the previous schedule
  HIPCHK(c, hipMemcpy(c->lr_sched_rows.p, rows.data(), total * sizeof(int32_t), hipMemcpyHostToDevice));
  if (has_idx) HIPCHK(c, hipMemcpy(c->lr_sched_idx.p, sc.estimate_idx_host, (size_t)sc.n_batches * sizeof(uint64_t), hipMemcpyHostToDevice));
  c->lr_sched_n = sc.n_batches;
  c->lr_sched_k = 0;
  c->lr_sched_kernels = sc.kernels;
  c->lr_sched_has_idx = has_idx;
  point_at_batch_copy(c, sc.batch, sc.likeadj);   // (where the device-gather route leaves the selected batch; the fused kernel reads the resident data set)
  return MIVI_OK;
}

mivi_status_t mivi_logreg_seek_batch(mivi_ctx_t *c, int32_t k) {
  if (!c) return MIVI_ERR_BAD_ARG;
  if (mivi_status_t rs = refuse_flow(c, "mivi_logreg_seek_batch")) return rs;
  if (c->lr_sched_n <= 0) return fail(c, MIVI_ERR_BAD_ARG, "no batch schedule set (mivi_logreg_set_batch_schedule)");
  if (k < 0 || k >= c->lr_sched_n) return fail(c, MIVI_ERR_BAD_ARG, "batch index outside the schedule");
  invalidate_graph(c);
  c->lr_sched_k = k;
  return MIVI_OK;
}

mivi_status_t mivi_set_target_funnel_constrained(mivi_ctx_t *c, double sigma_v) {
  mivi_status_t s = mivi_set_target_funnel(c, sigma_v);
  if (s == MIVI_OK) c->funnel_constrained = 1;
  return s;
}

mivi_status_t mivi_set_bijector_stacked(mivi_ctx_t *c, int32_t n_blocks, const int32_t *ranges, const int32_t *kinds) {
  if (!c || n_blocks < 0 || (n_blocks > 0 && (!ranges || !kinds))) return MIVI_ERR_BAD_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int d = c->cfg.d;
  std::vector<uint8_t> mask(d, 0), seen(d, 0);
  bool any = false;
  for (int b = 0; b < n_blocks; ++b) {
    const int lo = ranges[2 * b], hi = ranges[2 * b + 1];
    if (lo < 0 || hi > d || lo > hi) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: block range outside [0, d)");
    if (kinds[b] != 0 && kinds[b] != 1) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: kind must be 0 (identity) or 1 (exp)");
    for (int i = lo; i < hi; ++i) {
      if (seen[i]) return fail(c, MIVI_ERR_BAD_ARG, "stacked bijector: blocks overlap");
      seen[i] = 1;
      mask[i] = (uint8_t)kinds[b];
      any = any || kinds[b] == 1;
    }
  }
  invalidate_graph(c);
  HIPCHK(c, hipStreamSynchronize(c->stream));   // an estimate in flight may still read the old mask
  c->bij_ext = c->bij_ord = c->bij_tab = false;   // (the description the constrained rand / logpdf entries upload on first use: exp = lb 0)
  c->bij_code_h = mask;
  c->bij_bnd_h.assign(2 * (size_t)d, 0.0);
  if (!any) {   // all-identity (or no) bijector: nothing to apply
    c->bij_on = false;
    return MIVI_OK;
  }
  mivi_status_t s = ensure(c, c->bij_mask, (size_t)d, false);
  if (s) return s;
  HIPCHK(c, hipMemcpy(c->bij_mask.p, mask.data(), (size_t)d, hipMemcpyHostToDevice));
  c->bij_on = true;
  c->cap_M = 0;   // (re)allocate the work buffers incl. the per-column log-Jacobian sums
  return MIVI_OK;
}

mivi_status_t mivi_set_target_funnel(mivi_ctx_t *c, double sigma_v) {
  if (!c || !(sigma_v > 0.0) || c->cfg.d < 2) return MIVI_ERR_BAD_ARG;
  c->funnel_constrained = 0;
  c->funnel_sigma_v = sigma_v;
  c->t_const = -log(sigma_v) - 0.5 * kLog2Pi - 0.5 * (c->cfg.d - 1) * kLog2Pi;
  c->target = TGT_FUNNEL;
  invalidate_graph(c);
  return MIVI_OK;
}

mivi_status_t mivi_set_target_callback(mivi_ctx_t *c, mivi_logdensity_and_gradient_fn fg, mivi_logdensity_fn fv,
                                       void *user) {
  if (!c || !fg) return MIVI_ERR_BAD_ARG;
  c->cb_grad = fg;
  c->cb_value = fv;
  c->cb_user = user;
  c->t_const = 0.0;
  c->target = TGT_CALLBACK;
  invalidate_graph(c);
  return MIVI_OK;
}

int32_t mivi_fullrank_route(const mivi_ctx_t *c, int32_t n_samples) {
  if (!c || c->cfg.family != MIVI_FULLRANK) return 0;
  if (n_samples <= 0) n_samples = c->cfg.n_mc;
  if (!lds_path_shape_ok(c, n_samples) || (c->target != TGT_DIAG_GAUSS && c->target != TGT_DENSE_GAUSS)) return 0;
  return (lds_use_prod32(c, n_samples) ? 1 : 3) | 16;   // (bit 4: the bf16 matrix cores -- the only products this route has)
}

int32_t mivi_logreg_kernels(const mivi_ctx_t *c, int32_t n_samples) {
  if (!c) return 0;
  return logreg_kernel_bits(c, n_samples > 0 ? n_samples : c->cfg.n_mc);
}

mivi_status_t mivi_set_logreg_route(mivi_ctx_t *c, int32_t route) {
  if (!c || route < 0 || route > 2) return MIVI_ERR_BAD_ARG;
  c->lr_route = route;
  invalidate_graph(c);
  return MIVI_OK;
}

mivi_status_t mivi_set_index_source(mivi_ctx_t *c, const uint64_t *idx_dev) {
  if (!c) return MIVI_ERR_BAD_ARG;
  c->idx_src = idx_dev;
  invalidate_graph(c);
  return MIVI_OK;
}

mivi_status_t mivi_debug_timeline(mivi_ctx_t *c, void *buf) {
  if (!c) return MIVI_ERR_BAD_ARG;
#ifdef MIVI_DEV
  c->dbg = (long long *)buf;
  invalidate_graph(c);
  return MIVI_OK;
#else
  if (!buf) return MIVI_OK;
  return fail(c, MIVI_ERR_UNSUPPORTED, "timeline stamps are compiled out of the release library (build with `make DEV=1`)");
#endif
}

// ---------------------------------------------------------------------------------------------
// host-side RNG restatement
// ---------------------------------------------------------------------------------------------
void mivi_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4]) {
  u32x4 c{ctr[0], ctr[1], ctr[2], ctr[3]};
  const u32x4 r = philox4x32_10(c, key[0], key[1]);
  out[0] = r.x; out[1] = r.y; out[2] = r.z; out[3] = r.w;
}

void mivi_eps_bits_host(uint64_t seed, uint64_t idx, int32_t d, int64_t m, int32_t i0, int32_t count, uint32_t *out) {
  const uint64_t d4 = (uint64_t)((d + 3) / 4);
  for (int32_t t = 0; t < count; ++t) {
    const int32_t i = i0 + t;
    const u32x4 b = eps_block_bits(seed, idx, (uint64_t)m * d4 + (uint64_t)(i / 4));
    const uint32_t w[4] = {b.x, b.y, b.z, b.w};
    out[t] = w[i & 3];
  }
}

void mivi_eps_host(uint64_t seed, uint64_t idx, int32_t d, int64_t m, int32_t i0, int32_t count, int32_t dtype,
                   double *out) {
  const uint64_t d4 = (uint64_t)((d + 3) / 4);
  for (int32_t t = 0; t < count; ++t) {
    const int32_t i = i0 + t;
    const uint64_t q = (uint64_t)m * d4 + (uint64_t)(i / 4);
    if (dtype == MIVI_F32) {
      float e[4];
      eps_block<float>(seed, idx, q, e);
      out[t] = (double)e[i & 3];
    } else {
      double e[4];
      eps_block<double>(seed, idx, q, e);
      out[t] = e[i & 3];
    }
  }
}

