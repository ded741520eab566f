// rm_table_accum.hip — k_table_accum: a frame of a runtime scene table supersampled
// at the offsets of a caller's sample pattern and added onto the context's sum image
// (rm_dispatch_accumulate, include/rm_api.h RM_HAS_ACCUMULATION).
//
// A translation unit of its own and outside the hiprtc sources, as
// rm_table_pattern.hip is: a context with rm_scene_specialize on accumulates through
// this generic, LDS-staged code (the values are the same).  The waves are
// rm_table_pattern.hip's, with the accumulating tail (rm_accum_args.hpp).
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_accum_args.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

__global__ __launch_bounds__(64) void k_table_accum(Frame F, PatternArgs P, AccumArgs A) {
  extern __shared__ float lds[];
  __shared__ __attribute__((aligned(16))) float acc[kPatternAcc];
  const TableFast fast{F, stage(F, lds)};
  const int by = tile_row(blockIdx.y, gridDim.y);
  const int bx = tile_col(blockIdx.x, gridDim.x, 8);
  const int rounds = (P.n + 3) >> 2;
  for (int r = 0; r < rounds; ++r) accum_round(F, P, A, r, bx, by, acc, fast);
}

// A pattern of one sample: an 8x8 pixel tile.
__global__ __launch_bounds__(64) void k_table_accum_one(Frame F, PatternArgs P, AccumArgs A) {
  extern __shared__ float lds[];
  const TableFast fast{F, stage(F, lds)};
  const int by = tile_row(blockIdx.y, gridDim.y);
  const int bx = tile_col(blockIdx.x, gridDim.x, 4);
  accum_pixel(F, P, A, bx, by, fast);
}

}  // namespace rmd

namespace rm {

// Frame F of the table F.scene at pattern P, accumulated by A: launch_table_pattern's grids.
hipError_t launch_table_accum(const rmd::Frame& F, const rmd::PatternArgs& P, const rmd::AccumArgs& A,
                              hipStream_t s) {
  if (P.n == 1) {
    const dim3 grid1((unsigned)((F.width + 7) / 8), (unsigned)((F.rows + 7) / 8));
    hipLaunchKernelGGL(rmd::k_table_accum_one, grid1, dim3(64), table_lds_bytes(F.nprims), s, F, P, A);
    return hipGetLastError();
  }
  const dim3 grid((unsigned)((F.width + 3) / 4), (unsigned)((F.rows + 3) / 4));
  hipLaunchKernelGGL(rmd::k_table_accum, grid, dim3(64), table_lds_bytes(F.nprims), s, F, P, A);
  return hipGetLastError();
}

}  // namespace rm
