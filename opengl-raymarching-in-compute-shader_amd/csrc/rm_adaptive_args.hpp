// rm_adaptive_args.hpp — the kernel arguments of adaptive supersampling
// (rm_dispatch_adaptive / rm_dispatch_adaptive_edges / rm_dispatch_refine, DESIGN.md
// §4.12), shared by the kernels (rm_adaptive.hip, rm_adaptive_edges.hip,
// rm_table_adaptive.hip) and the host (rm_api_adaptive.hip), the refine kernels'
// round over Fast (adapt_refine_round).
#pragma once

#include <cstddef>
#include <cstdint>

#include "rm_scene.hpp"

namespace rmd {

// Tiles are 8x8 pixels, one wave each, numbered row-major: tile = ty * tiles_x + tx.
constexpr int kAdaptTile = 8;
// k_adapt_scan takes the tile counts in chunks of this many (1024 lanes x 16
// counts); the counts and offsets are allocated, and the counts zeroed, up to a
// whole number of chunks, so the scan needs no bounds.
constexpr int kAdaptScanLanes = 1024, kAdaptScanPer = 16;
constexpr size_t kAdaptScanChunk = (size_t)kAdaptScanLanes * kAdaptScanPer;

struct AdaptArgs {
  uint8_t* mask;              // [height][width], 0 / 1: the context's copy
  uint8_t* counts;            // [tiles] flagged pixels of a tile, 0..64
  uint32_t* offsets;          // [tiles] exclusive scan of counts
  unsigned long long* total;  // [1] all flagged pixels (up to 2^32: one more than a word holds)
  uint32_t* list;             // [total] px | py << 16, tile by tile, a tile's in lane order
  int32_t width, height, tiles_x;
};

// What k_adapt_classify_edges classifies (rm_dispatch_adaptive_edges): pass 1's
// images and the caller's criteria, checked by the host.
struct EdgeArgs {
  const void* gbuf;      // [height][width] rm_gbuffer_px, 16-byte aligned; read under a geometry bit
  const void* rgba8;     // pass 1's RGBA8 image, or null: rgba32f, quantised; read under COLOR
  const void* rgba32f;
  uint32_t edges;        // RM_AA_EDGE_* mask
  int32_t color_threshold;
  float depth_rel, normal_cos;
};

// One round of a refine kernel: group g of 16 list entries x 4 samples on one
// wave, over the fast-path scene sc (Fast, rm_trace.hpp): cast_ray, render, the
// three-shuffle sum and store_pixel of the AA kernels' sample bodies in the same
// order, so a refined pixel is the AA-on frame's bit for bit.  k_table_adapt_refine
// calls it over TableFast; k_adapt_refine (rm_adaptive.hip) holds the same round in
// its own text for now (see there).
template <class Fast>
__device__ __forceinline__ void adapt_refine_round(const Frame& F, const AdaptArgs& A, unsigned long long total,
                                                   unsigned long long g, const Fast& sc) {
  // the group's entries: 16, or what is left of the list (indices below 2^32)
  const uint32_t* __restrict__ ent = A.list + g * 16ull;
  const unsigned long long left = total - g * 16ull;
  const int n = left < 16ull ? (int)left : 16;
  // entry q = lane >> 2 of the group, sample s = lane & 3: as sample_body's lanes.
  // The spare lanes of a partial last group stay idle (all 4 of a pixel together).
  f3 col = mk(0.0f, 0.0f, 0.0f);
  {
    const int lane = threadIdx.x & 63;
    if ((lane >> 2) < n) {
      const uint32_t e = ent[lane >> 2];
      f3 ro, rd;
      cast_ray(F, lane_uv(F, 0, (int)(e & 0xffffu), lane & 3), lane_uv(F, 1, (int)(e >> 16), lane & 3), ro, rd);
      col = sc.render(ro, rd);
    }
  }
  const int ol = out_lane();
  // (the list entry is read again from the re-formed lane id: px, py do not stay live across the render)
  const Quad nb = quad_neighbours(col, ol);
  if ((ol & 3) == 0 && (ol >> 2) < n) {
    const uint32_t e = ent[ol >> 2];
    const size_t idx = (size_t)(e >> 16) * (size_t)F.width + (size_t)(e & 0xffffu);
    const f3 o = quad_sum(col, nb);
    store_pixel(F, idx, o.x / 4.0f, o.y / 4.0f, o.z / 4.0f, 1.0f);
  }
}

}  // namespace rmd
