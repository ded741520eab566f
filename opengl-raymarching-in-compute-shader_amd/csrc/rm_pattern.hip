// rm_pattern.hip — k_pattern: a frame of the built-in scene supersampled at the
// offsets of a caller's sample pattern (rm_dispatch_pattern, include/rm_api.h
// RM_HAS_SAMPLE_PATTERN).
//
// A translation unit of its own, so that the render kernels' code objects
// (rm_kernels.o, rm_kernels_aa.o) are what they were without it.  The device
// code is rm_kernels.hip's, included with both of its *_ONLY switches set, as
// rm_adaptive.hip includes it.
//
// The wave is k_sample's: a one-wave workgroup on a 4x4 pixel tile x 4 sample
// lanes, in tile_row / tile_col order; it takes ceil(n / 4) rounds over the
// pattern's samples, reading a sample's uv from the pattern's table
// (rm_pattern_args.hpp pattern_round).
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_builtin_fast.hpp"
#include "rm_pattern_args.hpp"

namespace rmd {

// The frame constants as k_adapt_refine takes them (rm_adaptive.hip AdaptFrame): a
// round reads the fields it needs from the kernel arguments at an index the
// compiler cannot see through, scalar loads where they are used, instead of the
// whole Frame live in SGPRs around the loop.
struct PatternFrame {
  Frame f[1];
};

// Waves per SIMD the register allocation must allow: k_sample's.
__global__ __launch_bounds__(64, 8) void k_pattern(PatternFrame B, PatternArgs P) {
  __shared__ __attribute__((aligned(16))) float acc[kPatternAcc];
  const int rounds = (P.n + 3) >> 2;
  for (int r = 0; r < rounds; ++r) {
    int slot = 0;
    asm volatile("" : "+s"(slot));
    const Frame& F = B.f[slot];
    const int by = tile_row(blockIdx.y, F.grid_y);
    const int bx = tile_col(blockIdx.x, F.grid_x, 128 / (kSampleTileW * 4));
    pattern_round(F, P, r, bx, by, acc, BuiltinFast{F});
  }
}

// A pattern of one sample (temporal jitter): k_pixel's wave, an 8x8 pixel tile, with
// the uv from the pattern's table.
__global__ __launch_bounds__(64, 8) void k_pattern_one(Frame F, PatternArgs P) {
  const int by = tile_row(blockIdx.y, F.grid_y);
  const int bx = tile_col(blockIdx.x, F.grid_x, 128 / (kTileW * 4));
  pattern_pixel(F, P, bx, by, BuiltinPrimary{F});
}

}  // namespace rmd

namespace rm {

// Frame F of the built-in scene at pattern P.  F.grid_x / grid_y are the sample
// kernels' 4x4 tiles' (pixel_grid with aa set), or for a pattern of one sample the
// pixel kernels' 8x8 tiles'.
hipError_t launch_pattern(const rmd::Frame& F, const rmd::PatternArgs& P, hipStream_t s) {
  if (P.n == 1) {
    hipLaunchKernelGGL(rmd::k_pattern_one, dim3(F.grid_x, F.grid_y), dim3(64), 0, s, F, P);
    return hipGetLastError();
  }
  rmd::PatternFrame B;
  B.f[0] = F;
  hipLaunchKernelGGL(rmd::k_pattern, dim3(F.grid_x, F.grid_y), dim3(64), 0, s, B, P);
  return hipGetLastError();
}

}  // namespace rm
