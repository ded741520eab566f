// rm_api_trace.hip — librm's C-ABI: ray queries (rm_trace_rays, rm_trace_rays_device,
// rm_pick; include/rm_api.h).  Caller-supplied rays against the context's scene
// with its current uniforms, by k_trace (the built-in scene, rm_trace.hip) or
// k_table_trace (a runtime scene table, rm_table_trace.hip).  DESIGN.md §4.9.
#include <hip/hip_runtime.h>

#include <string>

#include "rm_ctx.hpp"

using namespace rm;

static_assert(sizeof(rm_ray_hit) == 48, "rm_ray_hit is three 16-byte words (rm_trace.hpp trace_store)");

namespace {

constexpr uint32_t kAllFlags = RM_TRACE_REFLECTED | RM_TRACE_NORMAL | RM_TRACE_SHADE | RM_TRACE_SHADOW;

// What every entry point refuses, before any device call.
int check_query(rm_ctx* c, const void* origins, const void* dirs, int64_t n, uint32_t flags, const void* hits) {
  const int rc = refuse_multi(c, "ray queries");
  if (rc != RM_OK) return rc;
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
// queued there; n >= 1, device pointers.
int trace_launch(rm_ctx* c, const void* origins, const void* dirs, int64_t n, uint32_t flags, void* hits) {
  if (c->comm_failed) return comm_dead(c);
  const rmd::Frame F = query_frame(c);
  Timed t;
  int rc;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  const hipError_t e = scene_kernels(c).trace(F, origins, dirs, hits, n, flags, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "trace kernel launch");
  return t.end(c);
}

constexpr const char* kStaging = "ray queries: a staging buffer";

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
  // the origins at the start of the shared input buffer, the dirs behind them at a 256-byte boundary
  const size_t rb = (size_t)n * 3 * sizeof(float), doff = (rb + 255) / 256 * 256, hb = (size_t)n * sizeof(rm_ray_hit);
  if ((rc = ensure(c, c->stage_in, doff + rb, kStaging)) != RM_OK) return rc;
  if ((rc = ensure(c, c->stage_out, hb, kStaging)) != RM_OK) return rc;
  void* const d_o = c->stage_in.p;
  void* const d_d = static_cast<char*>(d_o) + doff;
  RM_HIP(c, hipMemcpyAsync(d_o, origins, rb, hipMemcpyHostToDevice, c->stream));
  RM_HIP(c, hipMemcpyAsync(d_d, dirs, rb, hipMemcpyHostToDevice, c->stream));
  if ((rc = trace_launch(c, d_o, d_d, n, flags, c->stage_out.p)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(hits, c->stage_out.p, hb, hipMemcpyDeviceToHost, c->stream));
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
