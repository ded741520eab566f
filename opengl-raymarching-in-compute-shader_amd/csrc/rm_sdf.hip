// rm_sdf.hip — k_sdf_points / k_sdf_grid: SDF field queries against the built-in
// scene (rm_sdf_points, rm_sdf_grid; include/rm_api.h).
//
// A translation unit of its own, as rm_trace.hip: rm_kernels.hip's device code
// with both of its *_ONLY switches set, so that no existing object changes.  The
// kernels' text is rm_sdf.hpp's bodies over BuiltinFast / BuiltinLit.
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_builtin_fast.hpp"
#include "rm_sdf.hpp"

namespace rmd {

// Of the query Frame only blend / omblend are read.
__global__ __launch_bounds__(64) void k_sdf_points(Frame F, SdfPointArgs A) {
  sdf_points_body(A, BuiltinFast{F}, BuiltinLit{F.blend, F.omblend});
}

// The grid: the coordinates come from the lane's indices, no input array.
__global__ __launch_bounds__(64) void k_sdf_grid(Frame F, SdfGridArgs G) {
  sdf_grid_body(G, SdfGridEval(BuiltinFast{F}, BuiltinLit{F.blend, F.omblend}));
}

}  // namespace rmd

namespace rm {

hipError_t launch_sdf_points(const rmd::Frame& F, const void* points, void* out, int64_t n, uint32_t flags,
                             hipStream_t s) {
  return rmd::launch_sdf_points_kernel(rmd::k_sdf_points, 0, F, points, out, n, flags, s);
}

hipError_t launch_sdf_grid(const rmd::Frame& F, const rmd::SdfGridArgs& G, hipStream_t s) {
  return rmd::launch_sdf_grid_kernel(rmd::k_sdf_grid, 0, F, G, s);
}

}  // namespace rm
