// rm_trace.hip — k_trace: ray queries against the built-in scene (rm_trace_rays,
// include/rm_api.h).
//
// A translation unit of its own, so that the render kernels' code objects
// (rm_kernels.o, rm_kernels_aa.o) are what they were without it.  The device
// code is rm_kernels.hip's, included with both of its *_ONLY switches set: that
// leaves its templates (march, get_normal, softshadow, render) and drops every
// kernel and launch wrapper of its own.  The kernel's text is trace_body
// (rm_trace.hpp) over BuiltinFast / BuiltinLit.  RM_QUERY_GAMMA: rm_scene.hpp gamma_pow.
#define RM_QUERY_GAMMA
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_builtin_fast.hpp"

namespace rmd {

// 64 VGPRs, 8 waves per SIMD, as the render kernels: no scratch (2 spilled SGPRs),
// and against the 71 registers / 7 waves of an unbounded build -4 % per SHADE trace
// and -6 % per HIT trace of the cfg 2 frame's rays (profiles/r07_ab_trace_waves.txt).
__global__ __launch_bounds__(64, 8) void k_trace(Frame F, TraceArgs A) {
  trace_body(F, A, BuiltinFast{F}, BuiltinLit{F.blend, F.omblend});
}

}  // namespace rmd

namespace rm {

hipError_t launch_trace(const rmd::Frame& F, const void* origins, const void* dirs, void* hits, int64_t n,
                        uint32_t flags, hipStream_t s) {
  return rmd::launch_trace_kernel(rmd::k_trace, 0, F, origins, dirs, hits, n, flags, s);
}

}  // namespace rm
