// rm_api_graph.hip — librm's hipGraph frame replay.
//
// Captures the frame once per render kernel (rm_ctx.hpp RenderKernel) / buffer
// set: the render kernel launch, and for one rank of an RCCL-gathered frame
// (rm_comm_init) the ncclGather and rank 0's assembly after it.  Each replay
// writes the frame's constants into the render node's by-value argument and
// launches the graph, so the graph path runs the same kernels as rm_dispatch at
// the same register budgets.  Counters and the wave-queue kernel are not
// available on this path.
#include <hip/hip_runtime.h>

#include "rm_ctx.hpp"

using namespace rm;

void rm::graph_release(rm_ctx* c) {
  rm_graph_slot& g = c->gs;
  if (g.exec || g.graph) (void)hipStreamSynchronize(c->stream);
  if (g.exec) (void)hipGraphExecDestroy(g.exec);
  if (g.graph) (void)hipGraphDestroy(g.graph);
  g = rm_graph_slot();
}

namespace {
int graph_capture(rm_ctx* c, const rmd::Frame& F, const RenderKernel& k) {
  graph_release(c);
  rm_graph_slot& g = c->gs;
  const bool comm = c->comm && !c->group_member;
  hipStream_t cs = nullptr;
  RM_HIP(c, hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
  hipStream_t keep = c->stream;
  int rc = RM_OK;
  hipError_t e = hipStreamBeginCapture(cs, hipStreamCaptureModeThreadLocal);
  if (e == hipSuccess) {
    e = launch(k, F, false, cs);
    // the render node: the one node the next captured operation would depend on
    hipStreamCaptureStatus st;
    const hipGraphNode_t* deps = nullptr;
    size_t ndeps = 0;
    if (e == hipSuccess) e = hipStreamGetCaptureInfo_v2(cs, &st, nullptr, nullptr, &deps, &ndeps);
    if (e == hipSuccess && ndeps == 1) g.render = deps[0];
    else if (e == hipSuccess) e = hipErrorInvalidValue;
    if (e == hipSuccess && comm) {
      c->stream = cs;  // the gather and the assembly, captured after the render
      rc = comm_gather(c);
      if (rc == RM_OK) rc = comm_assemble(c);
      c->stream = keep;
    }
    hipGraph_t gr = nullptr;
    const hipError_t e2 = hipStreamEndCapture(cs, &gr);
    g.graph = gr;
    if (e == hipSuccess) e = e2;
  }
  if (e == hipSuccess && rc == RM_OK) e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
  (void)hipStreamDestroy(cs);
  if (e != hipSuccess || rc != RM_OK) {
    if (rc == RM_OK) rc = hip_fail(c, e, "graph capture");
    graph_release(c);
    return rc;
  }
  g.kernel = k;
  g.send = render_dst(c);
  g.frame = image_rgba8(c);
  return RM_OK;
}
}  // namespace

int rm::graph_frame(rm_ctx* c) {
  if (c->comm_failed) return comm_dead(c);
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  rmd::Frame F = make_frame(c);
  const bool comm = c->comm && !c->group_member;
  if (comm && !c->comm_warm) {
    // RCCL sets a communicator's buffers up on its first operation, which must
    // not happen inside a capture: the first frame of a rank runs eagerly (every
    // rank takes the same branch, so the collective sequence matches)
    return rm_dispatch(c);
  }
  rm_graph_slot& g = c->gs;
  const RenderKernel k = pick_kernel(c, F);
  if ((!g.exec || !(k == g.kernel) || g.send != render_dst(c) || g.frame != image_rgba8(c)) &&
      (rc = graph_capture(c, F, k)) != RM_OK)
    return rc;
  // a table's render node is its batch kernel with one frame: its argument is a
  // FrameBatch (RenderKernel::takes_batch)
  static thread_local rmd::FrameBatch GB;
  void* args[] = {&F};
  if (k.takes_batch(false)) {
    GB.f[0] = F;
    args[0] = &GB;
  }
  hipKernelNodeParams kp;
  RM_HIP(c, hipGraphKernelNodeGetParams(g.render, &kp));
  kp.kernelParams = args;
  kp.extra = nullptr;
  RM_HIP(c, hipGraphExecKernelNodeSetParams(g.exec, g.render, &kp));
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  RM_HIP(c, hipGraphLaunch(g.exec, c->stream));
  if ((rc = t.end(c)) != RM_OK) return rc;
  c->dispatched = true;
  return RM_OK;
}

extern "C" {

int rm_graph_enable(rm_ctx* c, int enable) {
  if (!c) return RM_ERR_INVALID;
  for (rm_ctx* s : c->subs) {
    const int rc = rm_graph_enable(s, enable);
    if (rc != RM_OK) return fail(c, rc, s->err);
  }
  if (!c->subs.empty()) {
    c->graph_on = enable != 0;
    return RM_OK;
  }
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if (!enable) {
    graph_release(c);
    c->graph_on = false;
    return RM_OK;
  }
  if (c->cfg.counters) return fail(c, RM_ERR_STATE, "graph path does not collect counters");
  if (has_gbuf(c)) return fail(c, RM_ERR_STATE, "rm_graph_enable: not available on a G-buffer context (RM_OUT_GBUFFER)");
  c->graph_on = true;
  return RM_OK;
}

int rm_graph_dispatch(rm_ctx* c) {
  if (!c) return RM_ERR_INVALID;
  if (has_gbuf(c)) return fail(c, RM_ERR_STATE, "rm_graph_dispatch: not available on a G-buffer context (RM_OUT_GBUFFER)");
  if (!c->graph_on) return fail(c, RM_ERR_STATE, "rm_graph_enable(ctx, 1) first");
  if (!c->subs.empty()) return multi_frame(c, true);
  return graph_frame(c);
}

}  // extern "C"
