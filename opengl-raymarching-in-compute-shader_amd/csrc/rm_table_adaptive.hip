// rm_table_adaptive.hip — k_table_adapt_refine: the refinement of adaptive
// supersampling for a runtime scene table (rm_dispatch_adaptive /
// rm_dispatch_refine, include/rm_api.h).
//
// A translation unit of its own, so that rm_table.o's kernels are what they were
// without it, and outside the hiprtc sources: a context with rm_scene_specialize
// on refines through this generic, LDS-staged code too (the values are the same).
// The device code is rm_table.hip's, included without its kernels' launch
// wrappers.  The flags, the scan and the list are rm_adaptive.hip's kernels.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_adaptive_args.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

// The loop is rm_adaptive.hip's k_adapt_refine over table_sample_body's pixel
// (adapt_refine_round over TableFast): the table staged once per wave.
__global__ __launch_bounds__(64) void k_table_adapt_refine(Frame F, AdaptArgs A) {
  extern __shared__ float lds[];
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 15ull) >> 4;
  if (blockIdx.x >= ngroups) return;  // (uniform: before stage's barriers)
  const TableFast fast{F, stage(F, lds)};
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) adapt_refine_round(F, A, total, g, fast);
}

}  // namespace rmd

namespace rm {

// The listed pixels of frame F of the table F.scene, on `waves` one-wave workgroups.
hipError_t launch_table_adapt_refine(const rmd::Frame& F, const rmd::AdaptArgs& A, int waves, hipStream_t s) {
  hipLaunchKernelGGL(rmd::k_table_adapt_refine, dim3((unsigned)waves), dim3(64), table_lds_bytes(F.nprims), s, F, A);
  return hipGetLastError();
}

}  // namespace rm
