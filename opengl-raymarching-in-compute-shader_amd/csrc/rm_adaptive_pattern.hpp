// rm_adaptive_pattern.hpp — the rounds of pattern refinement in the adaptive calls
// (rm_dispatch_adaptive_pattern / rm_dispatch_refine_pattern, include/rm_api.h
// RM_HAS_ADAPTIVE_PATTERN) over the fast-path scene interface (Fast,
// rm_trace.hpp), shared by the kernels of the built-in scene (rm_adaptive_pattern.hip)
// and of a scene table (rm_table_adaptive_pattern.hip).  The arguments are the adaptive
// calls' list (AdaptArgs) and the pattern's table (PatternArgs) as they are.
#pragma once

#include <cstddef>
#include <cstdint>

#include "rm_adaptive_args.hpp"
#include "rm_pattern_args.hpp"

namespace rmd {

// Round r of group g of a pattern refinement's wave: adapt_refine_round's 16 list
// entries x 4 sample lanes crossed with pattern_round's rounds.  Lane l is on entry
// l >> 2 of the group and sample 4 r + (l & 3) of the pattern, with the uv from the
// pattern's table at the entry's px | py << 16; the lanes of entries past the list's
// end and of samples past n idle, a pixel's four together.  Lane s == 0 of an entry
// adds the round's samples onto the entry's running sum in sample order (sum = c_0,
// then sum + c_s one by one, a missing sample no + 0), and the last round divides by
// n and stores at the entry's index.  acc is pattern_round's: touched by that one
// lane only and never read in round 0, so neither the rounds nor consecutive groups
// of a striding wave need a barrier.
template <class Fast>
__device__ __forceinline__ void adapt_pattern_round(const Frame& F, const AdaptArgs& A, const PatternArgs& P,
                                                    unsigned long long total, unsigned long long g, int r,
                                                    float* acc, const Fast& sc) {
  // the group's entries: 16, or what is left of the list (indices below 2^32)
  const uint32_t* __restrict__ ent = A.list + g * 16ull;
  const unsigned long long rest = total - g * 16ull;
  const int ne = rest < 16ull ? (int)rest : 16;
  f3 col = mk(0.0f, 0.0f, 0.0f);
  {
    // the lane id formed here too, not from threadIdx.x: what the compiler derives from
    // that (the entry's number, its address in the group, the sample lane) is invariant
    // in one or both loops and was kept live across the render, 8 VGPRs spilled
    const int lane = out_lane();
    const int s = 4 * r + (lane & 3);
    if ((lane >> 2) < ne && s < P.n) {
      const uint32_t e = ent[lane >> 2];
      f3 ro, rd;
      // (px, py <= 65535 and n <= 16: below 2^16 * 16)
      cast_ray(F, P.uvx[(int)(e & 0xffffu) * P.n + s], P.uvy[(int)(e >> 16) * P.n + s], ro, rd);
      col = sc.render(ro, rd);
    }
  }
  // the lane id re-formed, as the refinement does: nothing of the entry stays live across the render
  const int ol = out_lane();
  const Quad nb = quad_neighbours(col, ol);
  const int q = ol >> 2;
  if ((ol & 3) != 0 || q >= ne) return;
  pattern_accumulate(F, P, r, q, col, nb, acc, [&] {
    const uint32_t e = ent[q];
    return (size_t)(e >> 16) * (size_t)F.width + (size_t)(e & 0xffffu);
  });
}

// A pattern of one sample: group g of 64 list entries, one lane per entry, so no lane
// of a full group idles.  The pixel is its sample (pattern_pixel): the colour itself is
// stored.  sc.render is the scene's render of a primary ray.
template <class Primary>
__device__ __forceinline__ void adapt_pattern_pixel(const Frame& F, const AdaptArgs& A, const PatternArgs& P,
                                                    unsigned long long total, unsigned long long g,
                                                    const Primary& sc) {
  const uint32_t* __restrict__ ent = A.list + g * 64ull;
  const unsigned long long rest = total - g * 64ull;
  const int ne = rest < 64ull ? (int)rest : 64;
  f3 col = mk(0.0f, 0.0f, 0.0f);
  {
    const int lane = threadIdx.x & 63;
    if (lane < ne) {
      const uint32_t e = ent[lane];
      f3 ro, rd;
      cast_ray(F, P.uvx[e & 0xffffu], P.uvy[e >> 16], ro, rd);
      col = sc.render(ro, rd);
    }
  }
  const int ol = out_lane();
  if (ol >= ne) return;
  const uint32_t e = ent[ol];
  const size_t idx = (size_t)(e >> 16) * (size_t)F.width + (size_t)(e & 0xffffu);
  store_pixel(F, idx, col.x, col.y, col.z, 1.0f);
}

}  // namespace rmd
