// rm_sdf_args.hpp — the SDF field-query kernels' arguments beside the Frame
// (rm_sdf.hpp), plain structs: what the host layer (rm_ctx.hpp, rm_api_sdf.hip)
// needs of those kernels, without their device code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rmd {

// Kernel arguments beside the Frame: points.
struct SdfPointArgs {
  const float* points;  // [n][3]
  float4* out;          // [n] rm_ray_hit, 3 x 16 B each
  int32_t n;
  uint32_t flags;       // RM_SDF_*, wave-uniform
};

// Kernel arguments beside the Frame: a grid.  Its nwg = bpr ny nz (row, x-block)
// pairs (<= nx ny nz <= 2^31 - 1) are numbered b = row bpr + x-block, row =
// iz ny + iy, and taken by the workgroups of a 1-D launch with a grid stride:
// rows and slices are not grid dimensions, whose 65,535 cap a dim of 2^24
// passes, and the launch holds at most kSdfGridMaxWg workgroups.  A lane takes xpl
// consecutive x: 1 (64 x per wave, 4-byte stores: any nx, any 4-byte aligned
// pointer) or 4 (256 x per wave, one 16-byte store per output: nx % 4 == 0 and
// 16-byte aligned pointers, so that every row starts on a 16-byte boundary).
struct SdfGridArgs {
  float origin[3], step[3];
  int32_t nx, ny, nz;
  uint32_t bpr;   // x-blocks per row: ceil(nx / (64 xpl))
  uint32_t nwg;   // bpr * ny * nz
  int32_t xpl;    // x per lane: 1 or 4
  float* dist;    // [nz][ny][nx] or null
  int32_t* ids;   // [nz][ny][nx] or null
};

// Workgroups of a grid launch at most: 2^24 one-wave workgroups are 2^30
// work-items, inside the 32-bit work-item count of a dispatch, and far more than
// the device holds at once.
constexpr uint32_t kSdfGridMaxWg = 1u << 24;

}  // namespace rmd
