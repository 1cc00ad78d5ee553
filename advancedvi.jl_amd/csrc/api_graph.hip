// libmivi C ABI, part 8: the ONE owner of hipGraph capture, of the context's one-slot graph cache and of the replay protocol of the
// graph-batched estimates.  The routes (api_batch.hip, api_optimize.hip, api_dist.hip, api_profile.hip) say what their key is and what
// they record; nothing outside this file touches the capture stream or an intermediate hipGraph_t.
#include "api_common.h"

// ---- capture layer ------------------------------------------------------------------------------------------------------------------
// The null stream cannot be captured: record on an internal stream, replay on the context's stream.
// Whatever `body` and HIP return: on exit c->stream is the caller's stream, no capture is open on the internal stream and the intermediate
// hipGraph_t is destroyed.  Failures in the order the routes always reported them: the body's status, the end of the capture, the
// instantiation; the owner *exec stays empty on all of them.  The instantiated graph goes into it here (GraphExec, mivi_internal.h), and
// handle_destroy below is where the library destroys one.
mivi_status_t capture_graph_fn(mivi_ctx *c, GraphExec *exec, mivi_status_t (*body)(void *), void *arg) {
  exec->reset();
  mivi_status_t s;
  if (!c->cap_stream && (s = make_stream(c, c->cap_stream, false))) return s;
  HIPCHK(c, hipStreamSynchronize(c->stream));   // pending memsets / uploads on the launch stream
  HIPCHK(c, hipStreamBeginCapture(c->cap_stream.get(), hipStreamCaptureModeThreadLocal));
  {
    StreamScope on_capture(c, c->cap_stream.get());
    s = body(arg);
  }
  hipGraph_t graph = nullptr;
  hipError_t e = hipStreamEndCapture(c->cap_stream.get(), &graph);
  const char *what = "hipStreamEndCapture";
  if (s == MIVI_OK && e == hipSuccess) {
    hipGraphExec_t made = nullptr;
    e = hipGraphInstantiate(&made, graph, nullptr, nullptr, 0);
    what = "hipGraphInstantiate";
    if (e == hipSuccess) exec->adopt(made);
  }
  if (graph) (void)hipGraphDestroy(graph);
  if (s) return s;
  if (e != hipSuccess) {
    c->err = std::string(what) + ": " + hipGetErrorString(e);
    return MIVI_ERR_HIP;
  }
  return MIVI_OK;
}

// ---- cache layer --------------------------------------------------------------------------------------------------------------------
static bool same_loop(const mivi_loop_t &a, const mivi_loop_t &b) {   // everything baked into a captured loop
  return a.rule == b.rule && a.op == b.op && a.averager == b.averager && a.n_steps == b.n_steps && a.eta == b.eta &&
         a.beta1 == b.beta1 && a.beta2 == b.beta2 && a.adam_eps == b.adam_eps && a.clip_epsilon == b.clip_epsilon &&
         a.avg_eta == b.avg_eta && a.opt_state_dev == b.opt_state_dev && a.avg_params_dev == b.avg_params_dev;
}

namespace mivi {
bool GraphCache::matches(const GraphKey &k) const {
  return exec && key.kind == k.kind && key.count == k.count && key.params == k.params && key.value == k.value && key.grad == k.grad &&
         key.lanes == k.lanes && key.per_branch == k.per_branch && key.route == k.route && key.mode == k.mode &&
         (k.kind != GRAPH_LOOP || same_loop(key.loop, k.loop));
}
void GraphCache::drop() {
  exec.reset();
  key = GraphKey{};
}
void handle_destroy(hipGraphExec_t h) { (void)hipGraphExecDestroy(h); }
}  // namespace mivi

mivi_status_t graph_record_fn(mivi_ctx *c, const GraphKey &key, mivi_status_t (*body)(void *), void *arg) {
  c->graph.drop();   // (the routes call invalidate_graph before whatever they prepare for a capture: nothing is cached here)
  const mivi_status_t s = capture_graph_fn(c, &c->graph.exec, body, arg);
  if (s == MIVI_OK) {
    c->graph.key = key;
    ++c->graph_records;
  }
  return s;
}

// Replay of graph-batched estimates.  The recordings read their estimate indices from the device-side counter (d_idx[0]) and most of them
// leave it advanced (k_bump_u64 as their last node): a caller that walks the indices in order (an SGD-style driver does) needs no
// counter-setting launch in front of the next replay.
void graph_seek(mivi_ctx *c, uint64_t idx0) {
  if (!(c->d_idx_valid && c->d_idx_expect == idx0))
    hipLaunchKernelGGL(k_set_u64x2, dim3(1), dim3(1), 0, c->stream, (uint64_t *)c->d_idx.p, idx0, 0ull, 1);
}
mivi_status_t graph_launch(mivi_ctx *c, uint64_t idx0, uint64_t advance, bool advances) {
  HIPCHK(c, hipGraphLaunch(c->graph.exec.get(), c->stream));
  c->d_idx_valid = advances;
  c->d_idx_expect = idx0 + advance;
  return MIVI_OK;
}
