// rm_accum_args.hpp — the kernel arguments of an accumulating pattern frame
// (rm_dispatch_accumulate, include/rm_api.h RM_HAS_ACCUMULATION),
// shared by the kernels (rm_accum.hip, rm_table_accum.hip) and the host
// (rm_api_accum.hip), and the pattern kernels' round and pixel (rm_pattern_args.hpp
// pattern_round, pattern_pixel) with the accumulating tail: the context's sum image
// read, added onto in sample order and written back, and the frame stored from it.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rm_pattern_args.hpp"

namespace rmd {

struct AccumArgs {
  float4* sum;   // the sum image, [height][width]: (S.r, S.g, S.b, (float)N)
  float nf;      // (float)(N + n) of the host's int64 count after this call: the divisor, and the new w
  int32_t seed;  // N > 0 before the call: the samples are added onto the stored sum
};

// The sum of pixel i written back with its count, and the frame's pixel from it.
__device__ __forceinline__ void accum_store(const Frame& F, const AccumArgs& A, size_t i, float a0, float a1,
                                            float a2) {
  A.sum[i] = make_float4(a0, a1, a2, A.nf);
  store_pixel(F, i, a0 / A.nf, a1 / A.nf, a2 / A.nf, 1.0f);
}

// pattern_accumulate with the sum image at both ends: round 0 starts from the stored sum
// (one 16-byte load, after the round's render: nothing of it is live across the render;
// loaded before the render into the pixel's LDS slots it measured slower)
// when the call continues one, from c_0 itself when it does not, and the sum image is not
// read then; the last round stores the sum and the frame's pixel.  Lane s == 0 of a pixel
// inside the frame only (accum_round returns the others before this).
template <class Idx>
__device__ __forceinline__ void accum_accumulate(const Frame& F, const PatternArgs& P, const AccumArgs& A, int r,
                                                 int q, f3 col, const Quad& nb, float* acc, const Idx& idx) {
  float a0 = col.x, a1 = col.y, a2 = col.z;
  if (r > 0) {
    a0 = acc[q] + col.x;
    a1 = acc[16 + q] + col.y;
    a2 = acc[32 + q] + col.z;
  } else if (A.seed) {  // (uniform)
    const float4 s = A.sum[idx()];
    a0 = s.x + col.x;
    a1 = s.y + col.y;
    a2 = s.z + col.z;
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
    accum_store(F, A, idx(), a0, a1, a2);
  }
}

// pattern_round with that tail.  A lane whose pixel is outside the frame (a ragged tile)
// returns before the pixel's index is formed: it neither loads nor stores the sum.
template <class Fast>
__device__ __forceinline__ void accum_round(const Frame& F, const PatternArgs& P, const AccumArgs& A, int r, int bx,
                                            int by, float* acc, const Fast& sc) {
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
  // the lane id re-formed, as pattern_round does: nothing of the pixel stays live across the render
  const int ol = out_lane();
  const Quad nb = quad_neighbours(col, ol);
  const int q = ol >> 2;
  const int px = bx * 4 + (q & 3), py = by * 4 + (q >> 2);
  if ((ol & 3) != 0 || px >= F.width || py >= F.rows) return;
  accum_accumulate(F, P, A, r, q, col, nb, acc, [&, px, py] { return (size_t)py * (size_t)F.width + (size_t)px; });
}

// pattern_pixel with the sum image: one lane per pixel of the 8x8 tile (bx, by), the
// pixel's one sample added onto its stored sum, or the sum itself.  A lane outside the
// frame returns before the render, so before the index.
template <class Primary>
__device__ __forceinline__ void accum_pixel(const Frame& F, const PatternArgs& P, const AccumArgs& A, int bx, int by,
                                            const Primary& sc) {
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
  float a0 = col.x, a1 = col.y, a2 = col.z;
  if (A.seed) {  // (uniform)
    const float4 s = A.sum[idx];
    a0 = s.x + col.x;
    a1 = s.y + col.y;
    a2 = s.z + col.z;
  }
  accum_store(F, A, idx, a0, a1, a2);
}

}  // namespace rmd
