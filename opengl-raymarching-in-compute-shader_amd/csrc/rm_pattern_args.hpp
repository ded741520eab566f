// rm_pattern_args.hpp — the kernel arguments of a sample-pattern frame
// (rm_dispatch_pattern, include/rm_api.h RM_HAS_SAMPLE_PATTERN),
// shared by the kernels (rm_pattern.hip, rm_table_pattern.hip) and the host
// (rm_api_pattern.hip), the kernels' round over Fast (pattern_round) and a round's tail (pattern_accumulate).
#pragma once

#include <cstddef>
#include <cstdint>

#include "rm_adaptive_args.hpp"
#include "rm_scene.hpp"

namespace rmd {

struct PatternArgs {
  const float* uvx;  // [width][n]: the uv of column px, sample s at px * n + s (rm::pattern_uv)
  const float* uvy;  // [height][n]
  int32_t n;         // samples per pixel, 1..RM_MAX_SAMPLES
  float nf;          // (float)n, the divisor of the sum
};

// The running sums of a wave's 16 pixels between rounds, in LDS: floats
// [channel][pixel].  Registers would have to stay live across the render, which
// has none to spare at 8 waves per SIMD.
constexpr int kPatternAcc = 3 * 16;

// The tail of a round for lane s == 0 of pixel q of the wave's 16: the round's samples
// added onto the pixel's running sum in sample order, samples past n taking no part;
// a round that is not the last keeps the sum in acc, the last divides by n and stores
// at idx() (a functor: the index is formed, a list entry re-read, on the store path only).
template <class Idx>
__device__ __forceinline__ void pattern_accumulate(const Frame& F, const PatternArgs& P, int r, int q, f3 col,
                                                   const Quad& nb, float* acc, const Idx& idx) {
  float a0 = col.x, a1 = col.y, a2 = col.z;
  if (r > 0) {
    a0 = acc[q] + col.x;
    a1 = acc[16 + q] + col.y;
    a2 = acc[32 + q] + col.z;
  }
  const int left = P.n - 4 * r;  // the pattern's samples from this round on (uniform), >= 1
  if (left > 1) {
    a0 += nb.c1.x;
    a1 += nb.c1.y;
    a2 += nb.c1.z;
  }
  if (left > 2) {
    a0 += nb.c2.x;
    a1 += nb.c2.y;
    a2 += nb.c2.z;
  }
  if (left > 3) {
    a0 += nb.c3.x;
    a1 += nb.c3.y;
    a2 += nb.c3.z;
  }
  if (left > 4) {
    acc[q] = a0;
    acc[16 + q] = a1;
    acc[32 + q] = a2;
  } else {
    store_pixel(F, idx(), a0 / P.nf, a1 / P.nf, a2 / P.nf, 1.0f);
  }
}

// Round r of a pattern frame's wave: the 4x4 pixel tile (bx, by) x 4 sample lanes of
// the AA kernels' sample bodies, lane l on pixel l >> 2 and sample 4 r + (l & 3) of
// the pattern, over the fast-path scene sc (Fast, rm_trace.hpp).  Lane s == 0 of a
// pixel adds the round's samples onto the pixel's running sum in sample order
// (sum = c_0, then sum + c_s one by one: for n = 4 the AA kernels' ((c0 + c1) + c2) + c3),
// samples past n take no part, and the last round divides by n and stores.  The
// sum is touched by that one lane only, so the rounds need no barrier.
template <class Fast>
__device__ __forceinline__ void pattern_round(const Frame& F, const PatternArgs& P, int r, int bx, int by, float* acc,
                                              const Fast& sc) {
  f3 col = mk(0.0f, 0.0f, 0.0f);
  {
    const int lane = threadIdx.x & 63;
    const int q = lane >> 2, s = 4 * r + (lane & 3);
    const int px = bx * 4 + (q & 3), py = by * 4 + (q >> 2);
    if (px < F.width && py < F.rows && s < P.n) {
      f3 ro, rd;
      cast_ray(F, P.uvx[px * P.n + s], P.uvy[py * P.n + s], ro, rd);  // (below 2^16 * 16)
      col = sc.render(ro, rd);
    }
  }
  // the lane id re-formed, as the refinement does: nothing of the pixel stays live across the render
  const int ol = out_lane();
  const Quad nb = quad_neighbours(col, ol);
  const int q = ol >> 2;
  const int px = bx * 4 + (q & 3), py = by * 4 + (q >> 2);
  if ((ol & 3) != 0 || px >= F.width || py >= F.rows) return;
  // (px, py captured by value: by reference k_pattern's code changed in size)
  pattern_accumulate(F, P, r, q, col, nb, acc, [&, px, py] { return (size_t)py * (size_t)F.width + (size_t)px; });
}

// A pattern of one sample: the frame kernels' pixel tile instead, one lane per pixel
// of the 8x8 tile (bx, by), so no lane of the wave idles.  The pixel is its sample:
// the sum is c_0 and c_0 / 1.0f is c_0.  sc.render is the scene's render of a
// primary ray.
template <class Primary>
__device__ __forceinline__ void pattern_pixel(const Frame& F, const PatternArgs& P, int bx, int by, const Primary& sc) {
  f3 col = mk(0.0f, 0.0f, 0.0f);
  {
    const int lane = threadIdx.x & 63;
    const int px = bx * 8 + (lane & 7), py = by * 8 + (lane >> 3);
    if (px >= F.width || py >= F.rows) return;
    f3 ro, rd;
    cast_ray(F, P.uvx[px], P.uvy[py], ro, rd);
    col = sc.render(ro, rd);
  }
  const int ol = out_lane();
  const size_t idx = (size_t)(by * 8 + (ol >> 3)) * (size_t)F.width + (size_t)(bx * 8 + (ol & 7));
  store_pixel(F, idx, col.x, col.y, col.z, 1.0f);
}

}  // namespace rmd
