// rm_adaptive_pattern.hip — k_adapt_refine_pattern: the refinement of adaptive
// supersampling at the offsets of a caller's sample pattern, for the built-in scene
// (rm_dispatch_adaptive_pattern / rm_dispatch_refine_pattern, include/rm_api.h
// RM_HAS_ADAPTIVE_PATTERN).
//
// A translation unit of its own, so that every other code object (rm_adaptive.o and
// rm_pattern.o among them) is what it was without it.  The device code is
// rm_kernels.hip's, included with both of its *_ONLY switches set, as rm_adaptive.hip
// includes it.  Pass 1, the flags, the scan and the list are the adaptive calls'
// kernels (rm_adaptive.hip, rm_adaptive_edges.hip) and the uv table is
// rm_dispatch_pattern's; only the refinement is new.
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_adaptive_pattern.hpp"
#include "rm_builtin_fast.hpp"

namespace rmd {

// The frame constants as k_adapt_refine takes them (rm_adaptive.hip AdaptFrame): a
// round reads the fields it needs from the kernel arguments at an index the compiler
// cannot see through, scalar loads where they are used, instead of the whole Frame
// live in SGPRs around the loops.
struct AdaptPatternFrame {
  Frame f[1];
};

// k_adapt_refine's wave over pattern_round's rounds: every wave reads the count (the
// host does not know it) and strides over the groups of 16 entries by the grid,
// ceil(n / 4) rounds a group.  Waves per SIMD the register allocation must allow:
// k_sample's.
__global__ __launch_bounds__(64, 8) void k_adapt_refine_pattern(AdaptPatternFrame B, AdaptArgs A, PatternArgs P) {
  __shared__ __attribute__((aligned(16))) float acc[kPatternAcc];
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 15ull) >> 4;
  const int rounds = (P.n + 3) >> 2;
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    for (int r = 0; r < rounds; ++r) {
      int slot = 0;
      asm volatile("" : "+s"(slot));
      const Frame& F = B.f[slot];
      adapt_pattern_round(F, A, P, total, g, r, acc, BuiltinFast{F});
    }
  }
}

// A pattern of one sample: groups of 64 entries, one lane per entry, rendered as
// k_pattern_one renders a pixel.
__global__ __launch_bounds__(64, 8) void k_adapt_refine_pattern_one(AdaptPatternFrame B, AdaptArgs A, PatternArgs P) {
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 63ull) >> 6;
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    int slot = 0;
    asm volatile("" : "+s"(slot));
    const Frame& F = B.f[slot];
    adapt_pattern_pixel(F, A, P, total, g, BuiltinPrimary{F});
  }
}

}  // namespace rmd

namespace rm {

// The listed pixels of frame F of the built-in scene at pattern P, on `waves` one-wave
// workgroups: groups of 16 entries, or of 64 for a pattern of one sample.
hipError_t launch_adapt_refine_pattern(const rmd::Frame& F, const rmd::AdaptArgs& A, const rmd::PatternArgs& P,
                                       int waves, hipStream_t s) {
  rmd::AdaptPatternFrame B;
  B.f[0] = F;
  if (P.n == 1)
    hipLaunchKernelGGL(rmd::k_adapt_refine_pattern_one, dim3((unsigned)waves), dim3(64), 0, s, B, A, P);
  else
    hipLaunchKernelGGL(rmd::k_adapt_refine_pattern, dim3((unsigned)waves), dim3(64), 0, s, B, A, P);
  return hipGetLastError();
}

}  // namespace rm
