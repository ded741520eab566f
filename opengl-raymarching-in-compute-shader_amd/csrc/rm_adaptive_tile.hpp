// rm_adaptive_tile.hpp — the tile bookkeeping the flagging kernels of adaptive
// supersampling share (rm_adaptive.hip: k_adapt_classify, k_adapt_mask,
// k_adapt_scatter; rm_adaptive_edges.hip: k_adapt_classify_edges):
// which pixel a lane has, how its flag reaches the mask and the tile's count, and
// pass 1's pixel as an RGBA8 word.  Device code only.
#pragma once

#include "rm_adaptive_args.hpp"
#include "rm_scene.hpp"

namespace rmd {

// One wave per 8x8 tile, four tiles of a tile row per workgroup: a grid of 4K's
// 130 k one-wave workgroups costs such short kernels more to launch than to run.
constexpr int kAdaptWaves = 4;

// The wave's tile column (the tile row is blockIdx.y); the last workgroup of a row
// may hold waves past tiles_x, whose lanes are all outside the frame.
__device__ __forceinline__ int adapt_tx() { return blockIdx.x * kAdaptWaves + (int)(threadIdx.x >> 6); }

// The lane's pixel of its wave's tile; false outside the frame.
__device__ __forceinline__ bool adapt_pixel(const AdaptArgs& A, int& px, int& py) {
  const int lane = threadIdx.x & 63;
  px = adapt_tx() * kAdaptTile + (lane & 7);
  py = blockIdx.y * kAdaptTile + (lane >> 3);
  return px < A.width && py < A.height;
}

// The flag into the context's mask, the tile's count into counts (every lane of
// the wave calls it: the ballot is over the whole tile).
__device__ __forceinline__ void adapt_flag(const AdaptArgs& A, bool in, int px, int py, bool flag) {
  if (in) A.mask[(size_t)py * (size_t)A.width + (size_t)px] = flag ? 1 : 0;
  const unsigned long long m = __ballot(in && flag);
  if ((threadIdx.x & 63) == 0 && adapt_tx() < A.tiles_x)
    A.counts[(size_t)blockIdx.y * (size_t)A.tiles_x + adapt_tx()] = (uint8_t)__popcll(m);
}

// max over R, G, B of |p_c - q_c| > thr on RGBA8 words (alpha takes no part)
__device__ __forceinline__ bool adapt_differs(uint32_t p, uint32_t q, int thr) {
  bool f = false;
#pragma unroll
  for (int sh = 0; sh < 24; sh += 8) {
    const int d = (int)((p >> sh) & 255u) - (int)((q >> sh) & 255u);
    f = f | ((d < 0 ? -d : d) > thr);
  }
  return f;
}

// Pass 1's pixel as its RGBA8 word: the RGBA8 image's, or the RGBA32F image's
// floats quantised as store_pixel quantises them.
__device__ __forceinline__ uint32_t adapt_word(const uint32_t* rgba8, const float4* rgba32f, size_t i) {
  if (rgba8) return rgba8[i];
  const float4 v = rgba32f[i];
  return quantize(v.x) | (quantize(v.y) << 8) | (quantize(v.z) << 16);
}

}  // namespace rmd
