// rm_table_pattern.hip — k_table_pattern: a frame of a runtime scene table
// supersampled at the offsets of a caller's sample pattern (rm_dispatch_pattern,
// include/rm_api.h RM_HAS_SAMPLE_PATTERN).
//
// A translation unit of its own, so that rm_table.o's kernels are what they were
// without it, and outside the hiprtc sources: a context with rm_scene_specialize
// on renders a pattern frame through this generic, LDS-staged code too (the
// values are the same).  The device code is rm_table.hip's, included without its
// kernels' launch wrappers.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_pattern_args.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

// table_sample_body's wave (4x4 pixels x 4 sample lanes, tile_row / tile_col
// order) over the pattern's rounds (pattern_round over TableFast): the table
// staged once per wave.
__global__ __launch_bounds__(64) void k_table_pattern(Frame F, PatternArgs P) {
  extern __shared__ float lds[];
  __shared__ __attribute__((aligned(16))) float acc[kPatternAcc];
  const TableFast fast{F, stage(F, lds)};
  const int by = tile_row(blockIdx.y, gridDim.y);
  const int bx = tile_col(blockIdx.x, gridDim.x, 8);
  const int rounds = (P.n + 3) >> 2;
  for (int r = 0; r < rounds; ++r) pattern_round(F, P, r, bx, by, acc, fast);
}

// A pattern of one sample: table_pixel_body's wave, an 8x8 pixel tile.
__global__ __launch_bounds__(64) void k_table_pattern_one(Frame F, PatternArgs P) {
  extern __shared__ float lds[];
  const TableFast fast{F, stage(F, lds)};
  const int by = tile_row(blockIdx.y, gridDim.y);
  const int bx = tile_col(blockIdx.x, gridDim.x, 4);
  pattern_pixel(F, P, bx, by, fast);
}

}  // namespace rmd

namespace rm {

// Frame F of the table F.scene at pattern P, one wave per 4x4 pixel tile, or per
// 8x8 pixel tile for a pattern of one sample.
hipError_t launch_table_pattern(const rmd::Frame& F, const rmd::PatternArgs& P, hipStream_t s) {
  if (P.n == 1) {
    const dim3 grid1((unsigned)((F.width + 7) / 8), (unsigned)((F.rows + 7) / 8));
    hipLaunchKernelGGL(rmd::k_table_pattern_one, grid1, dim3(64), table_lds_bytes(F.nprims), s, F, P);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)((F.width + 3) / 4), (unsigned)((F.rows + 3) / 4));
  hipLaunchKernelGGL(rmd::k_table_pattern, grid, dim3(64), table_lds_bytes(F.nprims), s, F, P);
  return hipGetLastError();
}

}  // namespace rm
