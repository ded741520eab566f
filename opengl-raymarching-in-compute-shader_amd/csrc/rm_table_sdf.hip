// rm_table_sdf.hip — k_table_sdf_points / k_table_sdf_grid: SDF field queries
// against a runtime scene table (rm_sdf_points, rm_sdf_grid; include/rm_api.h;
// DESIGN.md §4.11).
//
// A translation unit of its own, as rm_table_trace.hip: rm_table.hip's device
// code without its kernels' launch wrappers, outside the hiprtc sources (a
// context with rm_scene_specialize on queries through this generic code).  The
// kernels' text is rm_sdf.hpp's bodies over TableFast / TableLit.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_sdf.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

// As k_sdf_points / k_sdf_grid (rm_sdf.hip), over the table staged in LDS as
// k_table_trace stages it (the grid's once per workgroup, before its loop).
__global__ __launch_bounds__(64) void k_table_sdf_points(Frame F, SdfPointArgs A) {
  extern __shared__ float lds[];
  const TableFast fast{F, stage(F, lds)};  // (barriers: before any lane leaves)
  sdf_points_body(A, fast, TableLit{fast.S});
}

__global__ __launch_bounds__(64) void k_table_sdf_grid(Frame F, SdfGridArgs G) {
  extern __shared__ float lds[];
  const TableFast fast{F, stage(F, lds)};
  sdf_grid_body(G, SdfGridEval(fast, TableLit{fast.S}));
}

}  // namespace rmd

namespace rm {

// Against the table F.scene.
hipError_t launch_table_sdf_points(const rmd::Frame& F, const void* points, void* out, int64_t n, uint32_t flags,
                                   hipStream_t s) {
  return rmd::launch_sdf_points_kernel(rmd::k_table_sdf_points, table_lds_bytes(F.nprims), F, points, out, n, flags, s);
}

hipError_t launch_table_sdf_grid(const rmd::Frame& F, const rmd::SdfGridArgs& G, hipStream_t s) {
  return rmd::launch_sdf_grid_kernel(rmd::k_table_sdf_grid, table_lds_bytes(F.nprims), F, G, s);
}

}  // namespace rm
