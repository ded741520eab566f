// rm_table_sdf.hip — k_table_sdf_points / k_table_sdf_grid: SDF field queries
// against a runtime scene table (rm_sdf_points, rm_sdf_grid; include/rm_api.h;
// DESIGN.md §4.11).
//
// A translation unit of its own, as rm_table_trace.hip: rm_table.hip's device
// code without its kernels' launch wrappers, outside the hiprtc sources (a
// context with rm_scene_specialize on queries through this generic code).
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_sdf.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

// As k_sdf_points (rm_sdf.hip), over the table staged in LDS as k_table_trace
// stages it.  Table::dist is the table's sdf with per-point culling; tnormal's
// centre sample is that value at the same point, and its tnormalize is the IEEE
// v * (1 / sqrt(dot)) over the whole float range already.
__global__ __launch_bounds__(64) void k_table_sdf_points(Frame F, SdfPointArgs A) {
  extern __shared__ float lds[];
  const Table S = stage(F, lds);  // (barriers: before any lane leaves)
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const f3 p = trace_load3(A.points, i);
  const uint32_t flags = A.flags;
  const bool fast = sdf_fast_ok(p);
  TraceRec r = sdf_rec();
  if (fast) {
    TCnt c = {0, 0, 0, 0, 0, 0};
    int k;
    r.t = S.dist(p, k);
    r.id = S.id(k);
    r.material = S.material(k);
    r.albedo = S.color(k, p);
    if (flags & RM_SDF_NORMAL) r.normal = tnormal<false>(S, p, c, true, r.t);
  }
  if (!fast) r = lit_sdf(TableLit{S}, p, flags);
  sdf_store(A.out, i, r);
}

__global__ __launch_bounds__(64) void k_table_sdf_grid(Frame F, SdfGridArgs G) {
  extern __shared__ float lds[];
  const Table S = stage(F, lds);
  sdf_grid_body(G, [&](f3 p, float& d, int& id) {
    const bool fast = sdf_fast_ok(p);
    int k = 0;
    if (fast) d = S.dist(p, k);
    if (!fast) d = TableLit{S}.dist(p, k);
    id = S.id(k);
  });
}

// the table, then the lazy slots' balls (Table::sb), as the render kernels stage them
static size_t table_lds(const Frame& F) {
  return (((rm::scene_words(F.nprims) + 3) & ~(size_t)3) + 4 * (size_t)rm::EX_MAX_SLOTS) * sizeof(float);
}

}  // namespace rmd

namespace rm {

// n >= 1 points against the table F.scene; device pointers, out 16-byte aligned.
hipError_t launch_table_sdf_points(const rmd::Frame& F, const void* points, void* out, int64_t n, uint32_t flags,
                                   hipStream_t s) {
  const rmd::SdfPointArgs A{static_cast<const float*>(points), static_cast<float4*>(out), (int32_t)n, flags};
  hipLaunchKernelGGL(rmd::k_table_sdf_points, dim3((unsigned)((n + 63) / 64)), dim3(64), rmd::table_lds(F), s, F, A);
  return hipGetLastError();
}

hipError_t launch_table_sdf_grid(const rmd::Frame& F, const rmd::SdfGridArgs& G, hipStream_t s) {
  const unsigned blocks = G.nwg < rmd::kSdfGridMaxWg ? G.nwg : rmd::kSdfGridMaxWg;
  hipLaunchKernelGGL(rmd::k_table_sdf_grid, dim3(blocks), dim3(64), rmd::table_lds(F), s, F, G);
  return hipGetLastError();
}

}  // namespace rm
