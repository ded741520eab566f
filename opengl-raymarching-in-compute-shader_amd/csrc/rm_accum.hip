// rm_accum.hip — k_accum: a frame of the built-in scene supersampled at the offsets
// of a caller's sample pattern and added onto the context's sum image
// (rm_dispatch_accumulate, include/rm_api.h RM_HAS_ACCUMULATION).
//
// A translation unit of its own, so that every other code object (rm_pattern.o among
// them) is what it was without it.  The device code is rm_kernels.hip's, included
// with both of its *_ONLY switches set, as rm_pattern.hip includes it.
//
// The waves are rm_pattern.hip's, with the accumulating tail (rm_accum_args.hpp
// accum_round, accum_pixel).
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_accum_args.hpp"
#include "rm_builtin_fast.hpp"

namespace rmd {

// The frame constants as k_pattern takes them (rm_pattern.hip PatternFrame), and the
// sum's arguments beside them: read from the kernel arguments at an index the compiler
// cannot see through, scalar loads in the round's tail, where they are used.  As plain
// kernel arguments the four words stayed in SGPRs around the render, and k_accum spilled
// 8 B per lane to scratch.
struct AccumFrame {
  Frame f[1];
  AccumArgs a[1];
};

// Waves per SIMD the register allocation must allow: k_sample's.
__global__ __launch_bounds__(64, 8) void k_accum(AccumFrame B, PatternArgs P) {
  __shared__ __attribute__((aligned(16))) float acc[kPatternAcc];
  const int rounds = (P.n + 3) >> 2;
  for (int r = 0; r < rounds; ++r) {
    int slot = 0;
    asm volatile("" : "+s"(slot));
    const Frame& F = B.f[slot];
    const int by = tile_row(blockIdx.y, F.grid_y);
    const int bx = tile_col(blockIdx.x, F.grid_x, 128 / (kSampleTileW * 4));
    accum_round(F, P, B.a[slot], r, bx, by, acc, BuiltinFast{F});
  }
}

// A pattern of one sample: k_pattern_one's wave, an 8x8 pixel tile.
__global__ __launch_bounds__(64, 8) void k_accum_one(Frame F, PatternArgs P, AccumArgs A) {
  const int by = tile_row(blockIdx.y, F.grid_y);
  const int bx = tile_col(blockIdx.x, F.grid_x, 128 / (kTileW * 4));
  accum_pixel(F, P, A, bx, by, BuiltinPrimary{F});
}

}  // namespace rmd

namespace rm {

// Frame F of the built-in scene at pattern P, accumulated by A.  F.grid_x / grid_y as
// launch_pattern takes them.
hipError_t launch_accum(const rmd::Frame& F, const rmd::PatternArgs& P, const rmd::AccumArgs& A, hipStream_t s) {
  if (P.n == 1) {
    hipLaunchKernelGGL(rmd::k_accum_one, dim3(F.grid_x, F.grid_y), dim3(64), 0, s, F, P, A);
    return hipGetLastError();
  }
  rmd::AccumFrame B;
  B.f[0] = F;
  B.a[0] = A;
  hipLaunchKernelGGL(rmd::k_accum, dim3(F.grid_x, F.grid_y), dim3(64), 0, s, B, P);
  return hipGetLastError();
}

}  // namespace rm
