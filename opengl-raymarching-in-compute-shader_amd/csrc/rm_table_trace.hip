// rm_table_trace.hip — k_table_trace: ray queries against a runtime scene table
// (rm_trace_rays, include/rm_api.h).
//
// A translation unit of its own, so that rm_table.o's kernels are what they were
// without it, and outside the hiprtc sources: a context with rm_scene_specialize
// on traces through this generic, LDS-staged code too.  The device code is
// rm_table.hip's (tmarch / tnormal / tshadow / trender over the staged Table),
// included without its kernels' launch wrappers.  The kernel's text is trace_body
// (rm_trace.hpp) over TableFast / TableLit.  RM_QUERY_GAMMA: rm_scene.hpp gamma_pow.
#define RM_QUERY_GAMMA
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_table_lit.hpp"

namespace rmd {

// As k_trace (rm_trace.hip), over the staged table.
__global__ __launch_bounds__(64) void k_table_trace(Frame F, TraceArgs A) {
  extern __shared__ float lds[];
  const TableFast fast{F, stage(F, lds)};  // (barriers: before any lane leaves)
  trace_body(F, A, fast, TableLit{fast.S});
}

}  // namespace rmd

namespace rm {

// Against the table F.scene.
hipError_t launch_table_trace(const rmd::Frame& F, const void* origins, const void* dirs, void* hits,
                              int64_t n, uint32_t flags, hipStream_t s) {
  return rmd::launch_trace_kernel(rmd::k_table_trace, table_lds_bytes(F.nprims), F, origins, dirs, hits, n, flags, s);
}

}  // namespace rm
