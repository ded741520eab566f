// rm_api_sdf.hip — librm's C-ABI: SDF field queries (rm_sdf_points,
// rm_sdf_points_device, rm_sdf_grid, rm_sdf_grid_device; include/rm_api.h).
// sdf(p) and GetNormal(p) of the context's scene with its current uniforms, at
// caller-supplied points or on a regular grid, by k_sdf_points / k_sdf_grid (the
// built-in scene, rm_sdf.hip) or k_table_sdf_points / k_table_sdf_grid (a
// runtime scene table, rm_table_sdf.hip).  DESIGN.md §4.11.
#include <hip/hip_runtime.h>

#include <string>

#include "rm_ctx.hpp"

using namespace rm;

static_assert(sizeof(rm_ray_hit) == 48, "rm_ray_hit is three 16-byte words (rm_sdf.hpp sdf_store)");
static_assert(sizeof(rm_sdf_grid_desc) == 36, "rm_sdf_grid_desc: three floats, three floats, three int32");

namespace {

constexpr uint32_t kAllFlags = RM_SDF_NORMAL;

// What the entry points refuse, before any device call.
int check_points(rm_ctx* c, const void* points, int64_t n, uint32_t flags, const void* out) {
  int rc = refuse_multi(c, "sdf queries");
  if (rc != RM_OK) return rc;
  if (n < 0 || n > INT32_MAX) return fail(c, RM_ERR_INVALID, "sdf queries: n must be in 0..2^31 - 1");
  if (flags & ~kAllFlags) return fail(c, RM_ERR_INVALID, "sdf queries: unknown flag bits");
  if (n > 0 && (!points || !out)) return fail(c, RM_ERR_INVALID, "sdf queries: null pointer");
  return check_uniforms(c, c->u);
}

// *total: the grid's points.  0: nothing to do, and, as for n == 0 points, no
// pointer is looked at.
int check_grid(rm_ctx* c, const rm_sdf_grid_desc* g, const void* dist, const void* ids, int64_t* total) {
  int rc = refuse_multi(c, "sdf queries");
  if (rc != RM_OK) return rc;
  if (!g) return fail(c, RM_ERR_INVALID, "sdf grid: null descriptor");
  if ((rc = grid_points(c, "sdf grid", g, total)) != RM_OK) return rc;
  if (*total != 0 && !dist && !ids) return fail(c, RM_ERR_INVALID, "sdf grid: dist and ids are both null");
  return check_uniforms(c, c->u);
}

// One kernel on the context's stream, after whatever is queued there, bracketed
// by the timing events like a trace launch.
template <class Launch>
int sdf_launch(rm_ctx* c, Launch launch) {
  if (c->comm_failed) return comm_dead(c);
  const rmd::Frame F = query_frame(c);
  Timed t;
  int rc;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  const hipError_t e = launch(F);
  if (e != hipSuccess) return hip_fail(c, e, "sdf kernel launch");
  return t.end(c);
}

// n >= 1 points; device pointers.
int points_launch(rm_ctx* c, const void* points, int64_t n, uint32_t flags, void* out) {
  return sdf_launch(c, [&](const rmd::Frame& F) {
    return scene_kernels(c).sdf_points(F, points, out, n, flags, c->stream);
  });
}

// Every dim >= 1; device pointers, 4-byte aligned, one of them possibly null.
int grid_launch(rm_ctx* c, const rm_sdf_grid_desc* g, void* dist, void* ids) {
  const rmd::SdfGridArgs G = sdf_grid_args(g, dist, ids);
  return sdf_launch(c, [&](const rmd::Frame& F) { return scene_kernels(c).sdf_grid(F, G, c->stream); });
}

constexpr const char* kStaging = "sdf queries: a staging buffer";

}  // namespace

extern "C" {

int rm_sdf_points_device(rm_ctx* c, const void* points_dev, int64_t n, uint32_t flags, void* out_dev) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_points(c, points_dev, n, flags, out_dev);
  if (rc != RM_OK) return rc;
  if (n == 0) return RM_OK;
  if (reinterpret_cast<uintptr_t>(out_dev) % 16 != 0)
    return fail(c, RM_ERR_INVALID, "rm_sdf_points_device: out_dev must be 16-byte aligned");
  if ((rc = set_device(c)) != RM_OK) return rc;
  return points_launch(c, points_dev, n, flags, out_dev);
}

int rm_sdf_points(rm_ctx* c, const float* points, int64_t n, uint32_t flags, rm_ray_hit* out) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_points(c, points, n, flags, out);
  if (rc != RM_OK) return rc;
  if (n == 0) return RM_OK;
  if ((rc = set_device(c)) != RM_OK) return rc;
  const size_t pb = (size_t)n * 3 * sizeof(float), ob = (size_t)n * sizeof(rm_ray_hit);
  if ((rc = ensure(c, c->stage_in, pb, kStaging)) != RM_OK) return rc;
  if ((rc = ensure(c, c->stage_out, ob, kStaging)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(c->stage_in.p, points, pb, hipMemcpyHostToDevice, c->stream));
  if ((rc = points_launch(c, c->stage_in.p, n, flags, c->stage_out.p)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(out, c->stage_out.p, ob, hipMemcpyDeviceToHost, c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return RM_OK;
}

int rm_sdf_grid_device(rm_ctx* c, const rm_sdf_grid_desc* grid, void* dist_dev, void* ids_dev) {
  if (!c) return RM_ERR_INVALID;
  int64_t total = 0;
  int rc = check_grid(c, grid, dist_dev, ids_dev, &total);
  if (rc != RM_OK) return rc;
  if (total == 0) return RM_OK;
  if ((reinterpret_cast<uintptr_t>(dist_dev) | reinterpret_cast<uintptr_t>(ids_dev)) % 4 != 0)
    return fail(c, RM_ERR_INVALID, "rm_sdf_grid_device: dist_dev and ids_dev must be 4-byte aligned");
  if ((rc = set_device(c)) != RM_OK) return rc;
  return grid_launch(c, grid, dist_dev, ids_dev);
}

int rm_sdf_grid(rm_ctx* c, const rm_sdf_grid_desc* grid, float* dist, int32_t* ids) {
  if (!c) return RM_ERR_INVALID;
  int64_t total = 0;
  int rc = check_grid(c, grid, dist, ids, &total);
  if (rc != RM_OK) return rc;
  if (total == 0) return RM_OK;
  if ((rc = set_device(c)) != RM_OK) return rc;
  // the points' staging buffer holds the ids, the records' the distances
  const size_t b = (size_t)total * 4;
  if (ids && (rc = ensure(c, c->stage_in, b, kStaging)) != RM_OK) return rc;
  if (dist && (rc = ensure(c, c->stage_out, b, kStaging)) != RM_OK) return rc;
  if ((rc = grid_launch(c, grid, dist ? c->stage_out.p : nullptr, ids ? c->stage_in.p : nullptr)) != RM_OK) return rc;
  if (dist) RM_HIP(c, hipMemcpyAsync(dist, c->stage_out.p, b, hipMemcpyDeviceToHost, c->stream));
  if (ids) RM_HIP(c, hipMemcpyAsync(ids, c->stage_in.p, b, hipMemcpyDeviceToHost, c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return RM_OK;
}

}  // extern "C"
