// rm_adaptive_args.hpp — the kernel arguments of adaptive supersampling
// (rm_dispatch_adaptive / rm_dispatch_adaptive_edges / rm_dispatch_refine, DESIGN.md
// §4.12), shared by the kernels (rm_adaptive.hip, rm_adaptive_edges.hip,
// rm_table_adaptive.hip) and the host (rm_api_adaptive.hip).
#pragma once

#include <cstddef>
#include <cstdint>

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

}  // namespace rmd
