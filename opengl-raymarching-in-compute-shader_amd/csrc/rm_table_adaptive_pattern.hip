// rm_table_adaptive_pattern.hip — k_table_adapt_refine_pattern: the refinement of
// adaptive supersampling at the offsets of a caller's sample pattern, for a runtime
// scene table (rm_dispatch_adaptive_pattern / rm_dispatch_refine_pattern,
// include/rm_api.h RM_HAS_ADAPTIVE_PATTERN).
//
// A translation unit of its own, so that every other code object is what it was
// without it, and outside the hiprtc sources: a context with rm_scene_specialize on
// refines through this generic, LDS-staged code too (the values are the same).  The
// device code is rm_table.hip's, included without its kernels' launch wrappers.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_adaptive_pattern.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

// k_adapt_refine_pattern's loops (rm_adaptive_pattern.hip) over TableFast: the table
// staged once per wave.
__global__ __launch_bounds__(64) void k_table_adapt_refine_pattern(Frame F, AdaptArgs A, PatternArgs P) {
  extern __shared__ float lds[];
  __shared__ __attribute__((aligned(16))) float acc[kPatternAcc];
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 15ull) >> 4;
  if (blockIdx.x >= ngroups) return;  // (uniform: before stage's barriers)
  const TableFast fast{F, stage(F, lds)};
  const int rounds = (P.n + 3) >> 2;
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x)
    for (int r = 0; r < rounds; ++r) adapt_pattern_round(F, A, P, total, g, r, acc, fast);
}

// A pattern of one sample: groups of 64 entries, one lane per entry.
__global__ __launch_bounds__(64) void k_table_adapt_refine_pattern_one(Frame F, AdaptArgs A, PatternArgs P) {
  extern __shared__ float lds[];
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 63ull) >> 6;
  if (blockIdx.x >= ngroups) return;  // (uniform: before stage's barriers)
  const TableFast fast{F, stage(F, lds)};
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) adapt_pattern_pixel(F, A, P, total, g, fast);
}

}  // namespace rmd

namespace rm {

// The listed pixels of frame F of the table F.scene at pattern P, on `waves` one-wave
// workgroups.
hipError_t launch_table_adapt_refine_pattern(const rmd::Frame& F, const rmd::AdaptArgs& A, const rmd::PatternArgs& P,
                                             int waves, hipStream_t s) {
  if (P.n == 1)
    hipLaunchKernelGGL(rmd::k_table_adapt_refine_pattern_one, dim3((unsigned)waves), dim3(64),
                       table_lds_bytes(F.nprims), s, F, A, P);
  else
    hipLaunchKernelGGL(rmd::k_table_adapt_refine_pattern, dim3((unsigned)waves), dim3(64), table_lds_bytes(F.nprims),
                       s, F, A, P);
  return hipGetLastError();
}

}  // namespace rm
