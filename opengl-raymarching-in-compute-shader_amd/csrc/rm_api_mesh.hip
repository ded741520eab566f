// rm_api_mesh.hip — librm's C-ABI: SDF mesh extraction (rm_sdf_mesh,
// rm_sdf_mesh_device; include/rm_api.h).  A surface-nets mesh of the context's
// scene on a regular grid: the distance volume by the grid kernels of the field
// queries (k_sdf_grid / k_table_sdf_grid) into a buffer the context owns, the
// mesh by rm_mesh.hip's kernels, the attributes by the point kernels of the field
// queries (k_sdf_points / k_table_sdf_points) over the positions.  DESIGN.md §4.13.
#include <hip/hip_runtime.h>

#include <string>

#include "rm_ctx.hpp"

using namespace rm;

static_assert(sizeof(rm_sdf_mesh_counts) == 16, "rm_sdf_mesh_counts: two uint64 (rm_mesh_args.hpp counts)");
static_assert(RM_MESH_NORMAL == RM_SDF_NORMAL, "RM_MESH_NORMAL is the point kernels' flag");

namespace {

constexpr uint32_t kAllFlags = RM_MESH_TRIANGLES | RM_MESH_NORMAL;

// What both entry points refuse before any device call; the grid errors are
// rm_sdf_grid's (grid_points).  *cells: the grid's cells, 0 for a grid with a dim
// below 2.
int check_mesh(rm_ctx* c, const rm_sdf_grid_desc* g, uint32_t flags, const void* pos, int64_t vcap,
               const void* indices, int64_t qcap, const void* counts, int64_t* cells) {
  int rc = refuse_multi(c, "sdf mesh");
  if (rc != RM_OK) return rc;
  if (!g) return fail(c, RM_ERR_INVALID, "sdf mesh: null descriptor");
  if (!counts) return fail(c, RM_ERR_INVALID, "sdf mesh: null counts");
  if (flags & ~kAllFlags) return fail(c, RM_ERR_INVALID, "sdf mesh: unknown flag bits");
  if (vcap < 0 || qcap < 0) return fail(c, RM_ERR_INVALID, "sdf mesh: negative capacity");
  if ((vcap > 0 && !pos) || (qcap > 0 && !indices))
    return fail(c, RM_ERR_INVALID, "sdf mesh: null output with a capacity above 0");
  int64_t points;
  if ((rc = grid_points(c, "sdf mesh", g, &points)) != RM_OK) return rc;
  *cells = 0;
  if (g->dims[0] >= 2 && g->dims[1] >= 2 && g->dims[2] >= 2)
    *cells = (int64_t)(g->dims[0] - 1) * (g->dims[1] - 1) * (g->dims[2] - 1);
  return check_uniforms(c, c->u);
}

constexpr const char* kBuffer = "sdf mesh: a buffer";

// The grid's arguments (every dim >= 2) over the context's volume and per-wave
// arrays, both grown to it: the counts first, then the chunks' sums, then the
// per-wave arrays by falling alignment, each of whole scan chunks.
int mesh_args(rm_ctx* c, const rm_sdf_grid_desc* g, rmd::MeshArgs* M) {
  for (int a = 0; a < 3; ++a) {
    M->origin[a] = g->origin[a];
    M->step[a] = g->step[a];
  }
  M->nx = g->dims[0];
  M->ny = g->dims[1];
  M->nz = g->dims[2];
  M->bpr = (uint32_t)((M->nx + 63) / 64);
  M->nw = M->bpr * (uint32_t)M->ny * (uint32_t)M->nz;  // <= nx ny nz <= 2^31 - 1
  const size_t points = (size_t)M->nx * M->ny * M->nz;
  const size_t nwp = ((size_t)M->nw + rmd::kMeshScanChunk - 1) / rmd::kMeshScanChunk * rmd::kMeshScanChunk;
  int rc;
  if ((rc = ensure(c, c->mesh_vol, points * 4, kBuffer)) != RM_OK) return rc;
  const size_t wave_bytes = 16 + nwp / rmd::kMeshScanChunk * 16 + nwp * (32 + 8 + 4 + 4 + 1 + 1);
  if ((rc = ensure(c, c->mesh_waves, wave_bytes, kBuffer)) != RM_OK) return rc;
  M->vol = static_cast<const float*>(c->mesh_vol.p);
  uint8_t* p = static_cast<uint8_t*>(c->mesh_waves.p);
  M->counts = reinterpret_cast<unsigned long long*>(p);
  p += 16;
  M->chunks = reinterpret_cast<unsigned long long*>(p);
  p += nwp / rmd::kMeshScanChunk * 16;
  M->edges = reinterpret_cast<unsigned long long*>(p);
  p += nwp * 32;
  M->active = reinterpret_cast<unsigned long long*>(p);
  p += nwp * 8;
  M->qoff = reinterpret_cast<uint32_t*>(p);
  p += nwp * 4;
  M->voff = reinterpret_cast<uint32_t*>(p);
  p += nwp * 4;
  M->vcnt = p;
  p += nwp;
  M->qcnt = p;
  M->pos = nullptr;
  M->indices = nullptr;
  M->vcap = M->qcap = 0;
  M->triangles = 0;
  return RM_OK;
}

// The volume of the scene into the context's buffer, then the ballots, the scans
// and the counts: on the context's stream, by the field queries' grid kernel.
int mesh_count(rm_ctx* c, const rm_sdf_grid_desc* g, const rmd::Frame& F, const rmd::MeshArgs& M) {
  const rmd::SdfGridArgs G = sdf_grid_args(g, c->mesh_vol.p, nullptr);  // rm_sdf_grid_device's, dist only
  hipError_t e = scene_kernels(c).sdf_grid(F, G, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "sdf mesh: grid kernel launch");
  if ((e = launch_mesh_count(M, c->stream)) != hipSuccess) return hip_fail(c, e, "sdf mesh: count kernel launch");
  return RM_OK;
}

int points_launch(rm_ctx* c, const rmd::Frame& F, const void* points, int64_t n, uint32_t flags, void* out) {
  const hipError_t e = scene_kernels(c).sdf_points(F, points, out, n, flags & RM_MESH_NORMAL, c->stream);
  return e == hipSuccess ? RM_OK : hip_fail(c, e, "sdf mesh: point kernel launch");
}

size_t index_bytes(uint32_t flags) { return flags & RM_MESH_TRIANGLES ? 24 : 16; }

}  // namespace

extern "C" {

int rm_sdf_mesh_device(rm_ctx* c, const rm_sdf_grid_desc* grid, uint32_t flags, void* pos_dev, void* attr_dev,
                       int64_t vcap, void* indices_dev, int64_t qcap, void* counts_dev) {
  if (!c) return RM_ERR_INVALID;
  int64_t cells = 0;
  int rc = check_mesh(c, grid, flags, pos_dev, vcap, indices_dev, qcap, counts_dev, &cells);
  if (rc != RM_OK) return rc;
  const uintptr_t pa = reinterpret_cast<uintptr_t>(pos_dev), aa = reinterpret_cast<uintptr_t>(attr_dev),
                  ia = reinterpret_cast<uintptr_t>(indices_dev);
  if ((pa | aa | ia) % 16 != 0)
    return fail(c, RM_ERR_INVALID, "rm_sdf_mesh_device: pos_dev, attr_dev and indices_dev must be 16-byte aligned");
  if (reinterpret_cast<uintptr_t>(counts_dev) % 8 != 0)
    return fail(c, RM_ERR_INVALID, "rm_sdf_mesh_device: counts_dev must be 8-byte aligned");
  if (c->comm_failed) return comm_dead(c);
  if ((rc = set_device(c)) != RM_OK) return rc;
  if (cells == 0) {
    RM_HIP(c, hipMemsetAsync(counts_dev, 0, sizeof(rm_sdf_mesh_counts), c->stream));
    return RM_OK;
  }
  rmd::MeshArgs M;
  if ((rc = mesh_args(c, grid, &M)) != RM_OK) return rc;
  // the point kernel runs over the whole capacity (the host does not learn the count) into
  // a staging copy, of which the records below the count go to the caller's array
  const int64_t nattr = attr_dev ? (vcap < cells ? vcap : cells) : 0;
  const size_t attr_bytes = (size_t)nattr * sizeof(rm_ray_hit);
  if (nattr > 0 && (rc = ensure(c, c->mesh_attr, attr_bytes, kBuffer)) != RM_OK) return rc;
  const rmd::Frame F = query_frame(c);
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  if ((rc = mesh_count(c, grid, F, M)) != RM_OK) return rc;
  RM_HIP(c, hipMemcpyAsync(counts_dev, M.counts, sizeof(rm_sdf_mesh_counts), hipMemcpyDeviceToDevice, c->stream));
  M.pos = static_cast<float*>(pos_dev);
  M.indices = static_cast<uint32_t*>(indices_dev);
  M.vcap = vcap;
  M.qcap = qcap;
  M.triangles = flags & RM_MESH_TRIANGLES;
  hipError_t e = launch_mesh_emit(M, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "sdf mesh: emit kernel launch");
  if (nattr > 0) {
    if ((rc = points_launch(c, F, pos_dev, nattr, flags, c->mesh_attr.p)) != RM_OK) return rc;
    if ((e = launch_mesh_attr_copy(c->mesh_attr.p, attr_dev, M.counts, vcap, nattr, c->stream)) != hipSuccess)
      return hip_fail(c, e, "sdf mesh: attribute copy launch");
  }
  return t.end(c);
}

int rm_sdf_mesh(rm_ctx* c, const rm_sdf_grid_desc* grid, uint32_t flags, float* pos, rm_ray_hit* attr, int64_t vcap,
                uint32_t* indices, int64_t qcap, rm_sdf_mesh_counts* counts) {
  if (!c) return RM_ERR_INVALID;
  int64_t cells = 0;
  int rc = check_mesh(c, grid, flags, pos, vcap, indices, qcap, counts, &cells);
  if (rc != RM_OK) return rc;
  if (c->comm_failed) return comm_dead(c);
  if (cells == 0) {
    counts->vertices = counts->quads = 0;
    return RM_OK;
  }
  if ((rc = set_device(c)) != RM_OK) return rc;
  rmd::MeshArgs M;
  if ((rc = mesh_args(c, grid, &M)) != RM_OK) return rc;
  const rmd::Frame F = query_frame(c);
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  if ((rc = mesh_count(c, grid, F, M)) != RM_OK) return rc;
  // the call is synchronous: the host reads the counts and sizes the rest by them
  rm_sdf_mesh_counts n;
  RM_HIP(c, hipMemcpyAsync(&n, M.counts, sizeof n, hipMemcpyDeviceToHost, c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  const int64_t nv = (int64_t)n.vertices < vcap ? (int64_t)n.vertices : vcap;
  const int64_t nq = (int64_t)n.quads < qcap ? (int64_t)n.quads : qcap;
  const size_t pb = (size_t)nv * 3 * sizeof(float), ab = attr ? (size_t)nv * sizeof(rm_ray_hit) : 0,
               ib = (size_t)nq * index_bytes(flags);
  if ((rc = ensure(c, c->stage_in, pb, kBuffer)) != RM_OK) return rc;
  if ((rc = ensure(c, c->stage_out, ab, kBuffer)) != RM_OK) return rc;
  if ((rc = ensure(c, c->mesh_idx, ib, kBuffer)) != RM_OK) return rc;
  M.pos = static_cast<float*>(c->stage_in.p);
  M.indices = static_cast<uint32_t*>(c->mesh_idx.p);
  M.vcap = nv;
  M.qcap = nq;
  M.triangles = flags & RM_MESH_TRIANGLES;
  const hipError_t e = launch_mesh_emit(M, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "sdf mesh: emit kernel launch");
  if (ab && (rc = points_launch(c, F, c->stage_in.p, nv, flags, c->stage_out.p)) != RM_OK) return rc;
  if ((rc = t.end(c)) != RM_OK) return rc;
  if (pb) RM_HIP(c, hipMemcpyAsync(pos, c->stage_in.p, pb, hipMemcpyDeviceToHost, c->stream));
  if (ab) RM_HIP(c, hipMemcpyAsync(attr, c->stage_out.p, ab, hipMemcpyDeviceToHost, c->stream));
  if (ib) RM_HIP(c, hipMemcpyAsync(indices, c->mesh_idx.p, ib, hipMemcpyDeviceToHost, c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  *counts = n;
  return RM_OK;
}

}  // extern "C"
