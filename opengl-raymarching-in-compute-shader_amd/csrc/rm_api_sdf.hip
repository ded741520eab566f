// rm_api_sdf.hip — librm's C-ABI: SDF field queries (rm_sdf_points,
// rm_sdf_points_device, rm_sdf_grid, rm_sdf_grid_device; include/rm_api.h).
// sdf(p) and GetNormal(p) of the context's scene with its current uniforms, at
// caller-supplied points or on a regular grid, by k_sdf_points / k_sdf_grid (the
// built-in scene, rm_sdf.hip) or k_table_sdf_points / k_table_sdf_grid (a
// runtime scene table, rm_table_sdf.hip).  DESIGN.md §4.11.
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rm_ctx.hpp"

using namespace rm;

static_assert(sizeof(rm_ray_hit) == 48, "rm_ray_hit is three 16-byte words (rm_sdf.hpp sdf_store)");
static_assert(sizeof(rm_sdf_grid_desc) == 36, "rm_sdf_grid_desc: three floats, three floats, three int32");

namespace {

constexpr uint32_t kAllFlags = RM_SDF_NORMAL;
constexpr int32_t kMaxDim = 1 << 24;

// What every entry point refuses, before any device call.
int check_common(rm_ctx* c) {
  if (!c->subs.empty()) return fail(c, RM_ERR_STATE, "sdf queries: not available on a multi-device context (cfg.ngpus)");
  return RM_OK;
}

int check_points(rm_ctx* c, const void* points, int64_t n, uint32_t flags, const void* out) {
  int rc = check_common(c);
  if (rc != RM_OK) return rc;
  if (n < 0 || n > INT32_MAX) return fail(c, RM_ERR_INVALID, "sdf queries: n must be in 0..2^31 - 1");
  if (flags & ~kAllFlags) return fail(c, RM_ERR_INVALID, "sdf queries: unknown flag bits");
  if (n > 0 && (!points || !out)) return fail(c, RM_ERR_INVALID, "sdf queries: null pointer");
  return check_uniforms(c, c->u);
}

// *total: the grid's points.  0: nothing to do, and, as for n == 0 points, no
// pointer is looked at.
int check_grid(rm_ctx* c, const rm_sdf_grid_desc* g, const void* dist, const void* ids, int64_t* total) {
  int rc = check_common(c);
  if (rc != RM_OK) return rc;
  if (!g) return fail(c, RM_ERR_INVALID, "sdf grid: null descriptor");
  for (int a = 0; a < 3; ++a)
    if (g->dims[a] < 0 || g->dims[a] > kMaxDim) return fail(c, RM_ERR_INVALID, "sdf grid: every dim must be in 0..2^24");
  int64_t t = (int64_t)g->dims[0] * g->dims[1];  // <= 2^48
  if (t > INT32_MAX && g->dims[2] != 0) return fail(c, RM_ERR_INVALID, "sdf grid: more than 2^31 - 1 points");
  t = g->dims[2] == 0 ? 0 : t * g->dims[2];      // <= 2^55
  if (t > INT32_MAX) return fail(c, RM_ERR_INVALID, "sdf grid: more than 2^31 - 1 points");
  *total = t;
  if (t == 0) return check_uniforms(c, c->u);
  if (!dist && !ids) return fail(c, RM_ERR_INVALID, "sdf grid: dist and ids are both null");
  return check_uniforms(c, c->u);
}

// One kernel on the context's stream, after whatever is queued there, bracketed
// by the timing events like a trace launch.
template <class Launch>
int sdf_launch(rm_ctx* c, Launch launch) {
  if (c->comm_failed) return comm_dead(c);
  const rmd::Frame F = query_frame(c);
  hipEvent_t e0, e1;
  int rc;
  if ((rc = timing_events(c, &e0, &e1)) != RM_OK) return rc;
  if (e0) RM_HIP(c, hipEventRecord(e0, c->stream));
  const hipError_t e = launch(F);
  if (e != hipSuccess) return hip_fail(c, e, "sdf kernel launch");
  if (e1) RM_HIP(c, hipEventRecord(e1, c->stream));
  return RM_OK;
}

// n >= 1 points; device pointers.  Built-in or table code, as trace_launch chooses.
int points_launch(rm_ctx* c, const void* points, int64_t n, uint32_t flags, void* out) {
  return sdf_launch(c, [&](const rmd::Frame& F) {
    return c->nprims ? launch_table_sdf_points(F, points, out, n, flags, c->stream)
                     : launch_sdf_points(F, points, out, n, flags, c->stream);
  });
}

// Every dim >= 1; device pointers, 4-byte aligned, one of them possibly null.
int grid_launch(rm_ctx* c, const rm_sdf_grid_desc* g, void* dist, void* ids) {
  const rmd::SdfGridArgs G = sdf_grid_args(g, dist, ids);
  return sdf_launch(c, [&](const rmd::Frame& F) {
    return c->nprims ? launch_table_sdf_grid(F, G, c->stream) : launch_sdf_grid(F, G, c->stream);
  });
}

constexpr const char* kStaging = "sdf queries: a staging buffer";

}  // namespace

// The query's frame constants, built as trace_launch (rm_api_trace.hip) builds
// them: a dispatch's, without the two facts about a frame's primary rays.  The
// sdf kernels read blend / omblend and the scene table only.
rmd::Frame rm::query_frame(const rm_ctx* c) {
  rmd::Frame F = make_frame(c);
  std::memset(F.prepv, 0, sizeof F.prepv);
  F.unit_rd = 0;
  return F;
}

rmd::SdfGridArgs rm::sdf_grid_args(const rm_sdf_grid_desc* g, void* dist, void* ids) {
  rmd::SdfGridArgs G;
  for (int a = 0; a < 3; ++a) {
    G.origin[a] = g->origin[a];
    G.step[a] = g->step[a];
  }
  G.nx = g->dims[0];
  G.ny = g->dims[1];
  G.nz = g->dims[2];
  // 16-byte stores where every row of every output starts on a 16-byte boundary
  const uintptr_t da = reinterpret_cast<uintptr_t>(dist), ia = reinterpret_cast<uintptr_t>(ids);
  G.xpl = (G.nx % 4 == 0 && da % 16 == 0 && ia % 16 == 0) ? 4 : 1;
  const int per_wave = 64 * G.xpl;
  G.bpr = (uint32_t)((G.nx + per_wave - 1) / per_wave);
  G.nwg = G.bpr * (uint32_t)G.ny * (uint32_t)G.nz;  // <= nx ny nz <= 2^31 - 1
  G.dist = static_cast<float*>(dist);
  G.ids = static_cast<int32_t*>(ids);
  return G;
}

// The field queries' host paths are synchronous, and hipFree waits for the device:
// nothing of an earlier call is pending on a buffer that is replaced.
int rm::ensure_bytes(rm_ctx* c, void** buf, size_t* cap, size_t need, const char* what) {
  if (need <= *cap) return RM_OK;
  if (*buf) (void)hipFree(*buf);
  *buf = nullptr;
  *cap = 0;
  size_t n = 64 * 1024;
  while (n < need) n *= 2;
  if (hipMalloc(buf, n) != hipSuccess) {
    *buf = nullptr;
    (void)hipGetLastError();
    return fail(c, RM_ERR_NOMEM, std::string(what) + " of " + std::to_string(need) + " bytes");
  }
  *cap = n;
  return RM_OK;
}

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
  if ((rc = ensure_bytes(c, &c->d_sdf_in, &c->sdf_in_cap, pb, kStaging)) != RM_OK) return rc;
  if ((rc = ensure_bytes(c, &c->d_sdf_out, &c->sdf_out_cap, ob, kStaging)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(c->d_sdf_in, points, pb, hipMemcpyHostToDevice, c->stream));
  if ((rc = points_launch(c, c->d_sdf_in, n, flags, c->d_sdf_out)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(out, c->d_sdf_out, ob, hipMemcpyDeviceToHost, c->stream));
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
  if (ids && (rc = ensure_bytes(c, &c->d_sdf_in, &c->sdf_in_cap, b, kStaging)) != RM_OK) return rc;
  if (dist && (rc = ensure_bytes(c, &c->d_sdf_out, &c->sdf_out_cap, b, kStaging)) != RM_OK) return rc;
  if ((rc = grid_launch(c, grid, dist ? c->d_sdf_out : nullptr, ids ? c->d_sdf_in : nullptr)) != RM_OK) return rc;
  if (dist) RM_HIP(c, hipMemcpyAsync(dist, c->d_sdf_out, b, hipMemcpyDeviceToHost, c->stream));
  if (ids) RM_HIP(c, hipMemcpyAsync(ids, c->d_sdf_in, b, hipMemcpyDeviceToHost, c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return RM_OK;
}

}  // extern "C"
