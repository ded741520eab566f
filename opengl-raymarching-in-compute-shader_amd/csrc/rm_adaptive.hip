// rm_adaptive.hip — adaptive supersampling for the built-in scene, and its
// bookkeeping for every scene (rm_dispatch_adaptive / rm_dispatch_refine,
// include/rm_api.h).
//
// A translation unit of its own, so that the render kernels' code objects
// (rm_kernels.o, rm_kernels_aa.o) are what they were without it.  The device
// code is rm_kernels.hip's, included with both of its *_ONLY switches set, as
// rm_gbuffer.hip includes it.
//
// The frame is k_pixel's (one centre ray per pixel, launched by the host as
// pass 1) with the flagged pixels rendered again as k_sample renders them.  Four
// kernels join the two:
//   k_adapt_classify / k_adapt_mask
//                      one wave per 8x8 tile (four per workgroup): the pixel's flag
//                      (colour contrast against its 4-neighbours, or the caller's mask)
//                      into the context's 0/1 mask, the tile's count by ballot + popcount;
//   k_adapt_scan       exclusive scan of the tile counts, and their total;
//   k_adapt_scatter    the flagged pixels' coordinates into a list, a tile's at its
//                      offset in lane order (v_mbcnt): deterministic, an edge's pixels
//                      adjacent, and no atomic anywhere;
//   k_adapt_refine     16 list entries x 4 samples per wave and round: cast_ray,
//                      render<>, the three-shuffle sum and store_pixel of k_sample's
//                      sample_body, the same instantiations in the same order, so a
//                      refined pixel is the AA-on frame's bit for bit.
// The tile bookkeeping is rm_adaptive_tile.hpp's, shared with the geometry-edge
// classifier (rm_adaptive_edges.hip), whose flags take the same scan, scatter and
// refinement (launch_adapt_list below).
// This version: whole-frame, one-device contexts; no counting build.
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_adaptive_tile.hpp"

namespace rmd {

__global__ __launch_bounds__(64 * kAdaptWaves) void k_adapt_classify(AdaptArgs A, const uint32_t* __restrict__ rgba8,
                                                       const float4* __restrict__ rgba32f, int thr) {
  int px, py;
  const bool in = adapt_pixel(A, px, py);
  bool flag = false;
  if (in) {
    const size_t w = (size_t)A.width, i = (size_t)py * w + (size_t)px;
    const uint32_t p = adapt_word(rgba8, rgba32f, i);
    if (px > 0) flag |= adapt_differs(p, adapt_word(rgba8, rgba32f, i - 1), thr);
    if (px + 1 < A.width) flag |= adapt_differs(p, adapt_word(rgba8, rgba32f, i + 1), thr);
    if (py > 0) flag |= adapt_differs(p, adapt_word(rgba8, rgba32f, i - w), thr);
    if (py + 1 < A.height) flag |= adapt_differs(p, adapt_word(rgba8, rgba32f, i + w), thr);
  }
  adapt_flag(A, in, px, py, flag);
}

// The caller's mask, rows `pitch` bytes apart: any non-zero byte flags its pixel.
// src may be A.mask itself (pitch == width): a lane reads its byte before it writes it.
__global__ __launch_bounds__(64 * kAdaptWaves) void k_adapt_mask(AdaptArgs A, const uint8_t* src, size_t pitch) {
  int px, py;
  const bool in = adapt_pixel(A, px, py);
  const bool flag = in && src[(size_t)py * pitch + (size_t)px] != 0;
  adapt_flag(A, in, px, py, flag);
}

// Exclusive scan of counts[0 .. nchunks * kAdaptScanChunk) into offsets, the sum
// into *total: one workgroup, a chunk per round, 16 adjacent counts (one 16-byte
// load) per lane.  The tail of the last chunk holds zeros (rm_adaptive_args.hpp).
// Offsets are words: an exclusive offset is below width * height <= 2^32 for
// every real tile; the total, which may be 2^32, is kept in 64 bits.
__global__ __launch_bounds__(kAdaptScanLanes) void k_adapt_scan(const uint8_t* __restrict__ counts,
                                                                uint32_t* __restrict__ offsets,
                                                                unsigned long long* __restrict__ total,
                                                                uint32_t nchunks) {
  constexpr int kWaves = kAdaptScanLanes / 64;
  __shared__ uint32_t wsum[kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned long long base = 0;  // everything before this chunk (uniform)
  for (uint32_t ch = 0; ch < nchunks; ++ch) {
    const size_t i0 = ((size_t)ch * kAdaptScanLanes + (size_t)t) * kAdaptScanPer;
    const uint4 v = *reinterpret_cast<const uint4*>(counts + i0);
    const uint32_t words[4] = {v.x, v.y, v.z, v.w};
    uint32_t c[kAdaptScanPer], sum = 0;
#pragma unroll
    for (int j = 0; j < kAdaptScanPer; ++j) {
      c[j] = (words[j >> 2] >> (8 * (j & 3))) & 255u;
      sum += c[j];
    }
    uint32_t inc = sum;  // inclusive scan over the wave
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
      const uint32_t o = __shfl_up(inc, d);
      if (lane >= d) inc += o;
    }
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    uint32_t before = 0, all = 0;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const uint32_t s = wsum[k];
      before += k < w ? s : 0u;
      all += s;
    }
    __syncthreads();  // wsum is rewritten next round
    uint32_t run = (uint32_t)base + before + (inc - sum);
    uint32_t o[kAdaptScanPer];
#pragma unroll
    for (int j = 0; j < kAdaptScanPer; ++j) {
      o[j] = run;
      run += c[j];
    }
    uint4* dst = reinterpret_cast<uint4*>(offsets + i0);
#pragma unroll
    for (int j = 0; j < kAdaptScanPer / 4; ++j) dst[j] = make_uint4(o[4 * j], o[4 * j + 1], o[4 * j + 2], o[4 * j + 3]);
    base += all;
  }
  if (t == 0) *total = base;
}

__global__ __launch_bounds__(64 * kAdaptWaves) void k_adapt_scatter(AdaptArgs A) {
  int px, py;
  const bool in = adapt_pixel(A, px, py);
  const bool flag = in && A.mask[(size_t)py * (size_t)A.width + (size_t)px] != 0;
  const unsigned long long m = __ballot(flag);
  if (!flag) return;
  // (a flagged lane is inside the frame: its wave's tile is a real one)
  const size_t at = (size_t)A.offsets[(size_t)blockIdx.y * (size_t)A.tiles_x + adapt_tx()] + lane_rank(m);
  A.list[at] = (uint32_t)px | ((uint32_t)py << 16);  // both <= 65535
}

// The frame constants as k_sample_frames takes them (a batch of one): a round
// reads the fields it needs from the kernel arguments at an index the compiler
// cannot see through, as that kernel reads its frame's, so they are scalar loads
// where they are used instead of some 80 SGPRs live around the whole loop (which
// spilled: 52 SGPRs and 13 VGPRs, 56 B of scratch per lane).
struct AdaptFrame {
  Frame f[1];
};

// Waves per SIMD the register allocation must allow: k_sample's.
__global__ __launch_bounds__(64, 8) void k_adapt_refine(AdaptFrame B, AdaptArgs A) {
  // the host does not know the count: every wave reads it (a uniform load) and
  // strides over the groups of 16 entries by the grid
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 15ull) >> 4;
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    int slot = 0;
    asm volatile("" : "+s"(slot));
    const Frame& F = B.f[slot];
    // The round in this kernel's own text, not adapt_refine_round over BuiltinFast
    // (rm_adaptive_args.hpp, k_table_adapt_refine's): that form's code object differed
    // from this one's in the operand order of two integer adds, and the A/B of the two
    // (profiles/fast_scene_ab.txt) had one figure above this one's spread in most runs.
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
        Cnt c = {0, 0, 0, 0, 0, 0};
        f3 ro, rd;
        cast_ray(F, lane_uv(F, 0, (int)(e & 0xffffu), lane & 3), lane_uv(F, 1, (int)(e >> 16), lane & 3), ro, rd);
        col = render<false>(F, ro, rd, c);
      }
    }
    const int ol = out_lane();
    const Quad nb = quad_neighbours(col, ol);
    if ((ol & 3) == 0 && (ol >> 2) < n) {
      const uint32_t e = ent[ol >> 2];
      const size_t idx = (size_t)(e >> 16) * (size_t)F.width + (size_t)(e & 0xffffu);
      const f3 o = quad_sum(col, nb);
      store_pixel(F, idx, o.x / 4.0f, o.y / 4.0f, o.z / 4.0f, 1.0f);
    }
  }
}

}  // namespace rmd

namespace rm {

// The scan of the tile counts a flagging kernel has written, and the scatter of the
// flagged pixels into the list.  A's counts and offsets hold whole scan chunks
// (rm_adaptive_args.hpp).
hipError_t launch_adapt_list(const rmd::AdaptArgs& A, hipStream_t s) {
  const unsigned tiles_y = (unsigned)((A.height + rmd::kAdaptTile - 1) / rmd::kAdaptTile);
  const dim3 tiles((unsigned)((A.tiles_x + rmd::kAdaptWaves - 1) / rmd::kAdaptWaves), tiles_y), wg(64 * rmd::kAdaptWaves);
  const size_t ntiles = (size_t)A.tiles_x * tiles_y;
  const uint32_t nchunks = (uint32_t)((ntiles + rmd::kAdaptScanChunk - 1) / rmd::kAdaptScanChunk);
  hipLaunchKernelGGL(rmd::k_adapt_scan, dim3(1), dim3(rmd::kAdaptScanLanes), 0, s, A.counts, A.offsets, A.total, nchunks);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(rmd::k_adapt_scatter, tiles, wg, 0, s, A);
  return hipGetLastError();
}

// mask_src: the caller's device mask at mask_pitch (k_adapt_mask), or null: colour
// contrast above `threshold` on pass 1's image, F.rgba8 or else F.rgba32f
// (k_adapt_classify).  Then the scan and the scatter.
hipError_t launch_adapt_flags(const rmd::Frame& F, const rmd::AdaptArgs& A, const void* mask_src, size_t mask_pitch,
                              int threshold, hipStream_t s) {
  const unsigned tiles_y = (unsigned)((A.height + rmd::kAdaptTile - 1) / rmd::kAdaptTile);
  const dim3 tiles((unsigned)((A.tiles_x + rmd::kAdaptWaves - 1) / rmd::kAdaptWaves), tiles_y), wg(64 * rmd::kAdaptWaves);
  if (mask_src)
    hipLaunchKernelGGL(rmd::k_adapt_mask, tiles, wg, 0, s, A, static_cast<const uint8_t*>(mask_src), mask_pitch);
  else
    hipLaunchKernelGGL(rmd::k_adapt_classify, tiles, wg, 0, s, A, reinterpret_cast<const uint32_t*>(F.rgba8),
                       reinterpret_cast<const float4*>(F.rgba32f), threshold);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  return launch_adapt_list(A, s);
}

// The listed pixels of frame F of the built-in scene, on `waves` one-wave workgroups.
hipError_t launch_adapt_refine(const rmd::Frame& F, const rmd::AdaptArgs& A, int waves, hipStream_t s) {
  rmd::AdaptFrame B;
  B.f[0] = F;
  hipLaunchKernelGGL(rmd::k_adapt_refine, dim3((unsigned)waves), dim3(64), 0, s, B, A);
  return hipGetLastError();
}

}  // namespace rm
