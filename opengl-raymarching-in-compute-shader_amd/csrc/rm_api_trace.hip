// rm_api_trace.hip — librm's C-ABI: ray queries (rm_trace_rays, rm_trace_rays_device,
// rm_pick; include/rm_api.h).  Caller-supplied rays against the context's scene
// with its current uniforms, by k_trace (the built-in scene, rm_trace.hip) or
// k_table_trace (a runtime scene table, rm_table_trace.hip).  DESIGN.md §4.9.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rm_ctx.hpp"

using namespace rm;

static_assert(sizeof(rm_ray_hit) == 48, "rm_ray_hit is three 16-byte words (rm_trace.hpp trace_store)");

namespace {

constexpr uint32_t kAllFlags = RM_TRACE_REFLECTED | RM_TRACE_NORMAL | RM_TRACE_SHADE | RM_TRACE_SHADOW;

// What every entry point refuses, before any device call.
int check_query(rm_ctx* c, const void* origins, const void* dirs, int64_t n, uint32_t flags, const void* hits) {
  if (!c->subs.empty()) return fail(c, RM_ERR_STATE, "ray queries: not available on a multi-device context (cfg.ngpus)");
  if (n < 0 || n > INT32_MAX) return fail(c, RM_ERR_INVALID, "ray queries: n must be in 0..2^31 - 1");
  if (flags & ~kAllFlags) return fail(c, RM_ERR_INVALID, "ray queries: unknown flag bits");
  if ((flags & RM_TRACE_SHADOW) && flags != RM_TRACE_SHADOW)
    return fail(c, RM_ERR_INVALID, "ray queries: RM_TRACE_SHADOW combines with no other flag");
  if ((flags & RM_TRACE_SHADE) && (flags & RM_TRACE_REFLECTED))
    return fail(c, RM_ERR_INVALID, "ray queries: RM_TRACE_SHADE renders RayMarch's hit, not RM_TRACE_REFLECTED's");
  if (n > 0 && (!origins || !dirs || !hits)) return fail(c, RM_ERR_INVALID, "ray queries: null pointer");
  return check_uniforms(c, c->u);
}

// The trace kernel for the context's scene on its stream, after whatever is
// queued there; n >= 1, device pointers.  The frame constants are a dispatch's
// but for the two facts that hold for a frame's primary rays only: step 0 at
// the camera (prepv) and |rd| = 1 (unit_rd).  The images and counters in F are
// not touched by the trace kernels.
int trace_launch(rm_ctx* c, const void* origins, const void* dirs, int64_t n, uint32_t flags, void* hits) {
  if (c->comm_failed) return comm_dead(c);
  rmd::Frame F = make_frame(c);
  std::memset(F.prepv, 0, sizeof F.prepv);
  F.unit_rd = 0;
  hipEvent_t e0, e1;
  int rc;
  if ((rc = timing_events(c, &e0, &e1)) != RM_OK) return rc;
  if (e0) RM_HIP(c, hipEventRecord(e0, c->stream));
  // built-in or table code, as pick_kernel chooses for frames; a table always
  // with the generic kernel (its specialised kernels render frames only)
  const hipError_t e = c->nprims ? launch_table_trace(F, origins, dirs, hits, n, flags, c->stream)
                                 : launch_trace(F, origins, dirs, hits, n, flags, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "trace kernel launch");
  if (e1) RM_HIP(c, hipEventRecord(e1, c->stream));
  return RM_OK;
}

int ensure_staging(rm_ctx* c, int64_t n) {
  if (n <= c->trace_cap) return RM_OK;
  // a buffer in use by an earlier query is free once the stream has passed it: the
  // host path is synchronous, so nothing of it is pending here
  if (c->d_trace_rays) (void)hipFree(c->d_trace_rays);
  if (c->d_trace_hits) (void)hipFree(c->d_trace_hits);
  c->d_trace_rays = nullptr;
  c->d_trace_hits = nullptr;
  c->trace_cap = 0;
  int64_t cap = 1024;
  while (cap < n) cap *= 2;
  if (hipMalloc(&c->d_trace_rays, (size_t)cap * 6 * sizeof(float)) != hipSuccess ||
      hipMalloc(&c->d_trace_hits, (size_t)cap * sizeof(rm_ray_hit)) != hipSuccess) {
    if (c->d_trace_rays) (void)hipFree(c->d_trace_rays);
    c->d_trace_rays = nullptr;
    c->d_trace_hits = nullptr;
    (void)hipGetLastError();
    return fail(c, RM_ERR_NOMEM, "ray queries: staging buffers for " + std::to_string(n) + " rays");
  }
  c->trace_cap = cap;
  return RM_OK;
}

}  // namespace

extern "C" {

int rm_trace_rays_device(rm_ctx* c, const void* origins_dev, const void* dirs_dev, int64_t n, uint32_t flags,
                         void* hits_dev) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_query(c, origins_dev, dirs_dev, n, flags, hits_dev);
  if (rc != RM_OK) return rc;
  if (n == 0) return RM_OK;
  if (reinterpret_cast<uintptr_t>(hits_dev) % 16 != 0)
    return fail(c, RM_ERR_INVALID, "rm_trace_rays_device: hits_dev must be 16-byte aligned");
  if ((rc = set_device(c)) != RM_OK) return rc;
  return trace_launch(c, origins_dev, dirs_dev, n, flags, hits_dev);
}

int rm_trace_rays(rm_ctx* c, const float* origins, const float* dirs, int64_t n, uint32_t flags, rm_ray_hit* hits) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_query(c, origins, dirs, n, flags, hits);
  if (rc != RM_OK) return rc;
  if (n == 0) return RM_OK;
  if ((rc = set_device(c)) != RM_OK) return rc;
  if ((rc = ensure_staging(c, n)) != RM_OK) return rc;
  float* d_o = c->d_trace_rays;
  float* d_d = c->d_trace_rays + 3 * c->trace_cap;
  const size_t rb = (size_t)n * 3 * sizeof(float);
  RM_HIP(c, hipMemcpyAsync(d_o, origins, rb, hipMemcpyHostToDevice, c->stream));
  RM_HIP(c, hipMemcpyAsync(d_d, dirs, rb, hipMemcpyHostToDevice, c->stream));
  if ((rc = trace_launch(c, d_o, d_d, n, flags, c->d_trace_hits)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(hits, c->d_trace_hits, (size_t)n * sizeof(rm_ray_hit), hipMemcpyDeviceToHost, c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return RM_OK;
}

int rm_pick(rm_ctx* c, int32_t px, int32_t py, rm_ray_hit* hit) {
  if (!c) return RM_ERR_INVALID;
  if (!hit) return fail(c, RM_ERR_INVALID, "rm_pick: null pointer");
  const int32_t W = c->cfg.width, H = c->cfg.height;
  if (px < 0 || py < 0 || px >= W || py >= H)
    return fail(c, RM_ERR_INVALID, "rm_pick: pixel outside the " + std::to_string(W) + " x " + std::to_string(H) + " frame");
  // main glsl:301-305 and castRay glsl:68-74 for this pixel, the IEEE float
  // operations in the shader's order (no contraction: Makefile), as the kernels'
  // cast_ray forms them per lane
  const rm_camera& cam = c->u.camera;
  const float uvx = (float)(px * 2 - W) / (float)W, uvy = (float)(py * 2 - H) / (float)H;
  const float persp = 45.0f * static_cast<float>(0.01745329251994329576923690768489);
  float v[4];
  for (int k = 0; k < 4; ++k) v[k] = (uvx * cam.xAxis[k] + uvy * cam.yAxis[k]) + cam.dir[k] * persp;
  const float dd = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3]);
  const float inv = 1.0f / __builtin_sqrtf(dd);
  const float ro[3] = {cam.pos[0], cam.pos[1], cam.pos[2]};
  const float rd[3] = {v[0] * inv, v[1] * inv, v[2] * inv};
  return rm_trace_rays(c, ro, rd, 1, RM_TRACE_HIT | RM_TRACE_NORMAL, hit);
}

}  // extern "C"
