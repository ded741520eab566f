// rm_adaptive_edges.hip — k_adapt_classify_edges: the flags of
// rm_dispatch_adaptive_edges (include/rm_api.h), the union of the
// caller's edge criteria on pass 1's own G-buffer records and / or RGBA8 image.
//
// A translation unit of its own: rm_adaptive.o's kernels, and every render
// object, are what they were without it.  It renders nothing and is scene
// independent; the scan, the list and the refinement after it are
// rm_adaptive.hip's and rm_table_adaptive.hip's, unchanged.
//
// One wave per 8x8 tile as k_adapt_classify (rm_adaptive_tile.hpp): the 0/1 mask
// byte, the tile's count by ballot + popcount.  A record is two 16-byte loads; the
// colour word is read only under RM_AA_EDGE_COLOR, the record only under a
// geometry bit (the criteria are kernel arguments: scalar branches).
//
// Every pair test is symmetric, so by default a lane evaluates two pairs, not
// four: (p, right) and (p, above).  The wave's two ballots of those results hold
// (left, p) at bit lane - 1 and (below, p) at bit lane - 8 for every lane whose
// left / lower neighbour is in the tile; only the tile's left column and bottom
// row evaluate a pair whose partner is another wave's pixel.  EXCHANGE = false is
// the plain form, own record and four neighbours, kept for the measurement
// (RM_AA_EDGES_NAIVE): the same mask.
#include "rm_adaptive_tile.hpp"

#include "../../include/rm_api.h"

namespace rmd {

constexpr uint32_t kEdgeGeometry = RM_AA_EDGE_ID | RM_AA_EDGE_DEPTH | RM_AA_EDGE_NORMAL | RM_AA_EDGE_ALBEDO;

// rm_gbuffer_px as gbuf_store writes it: a = {t, id, normal[0], normal[1]},
// b = {normal[2], albedo[0..2]}; w is pass 1's RGBA8 word.
struct EdgePx {
  float4 a, b;
  uint32_t w;
};

__device__ __forceinline__ EdgePx edge_load(const EdgeArgs& E, size_t i) {
  EdgePx p;
  p.a = p.b = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
  p.w = 0u;
  if (E.edges & kEdgeGeometry) {
    const float4* __restrict__ rec = static_cast<const float4*>(E.gbuf) + 2 * i;
    p.a = rec[0];
    p.b = rec[1];
  }
  if (E.edges & RM_AA_EDGE_COLOR)
    p.w = adapt_word(static_cast<const uint32_t*>(E.rgba8), static_cast<const float4*>(E.rgba32f), i);
  return p;
}

// The rule of include/rm_api.h for the pair (p, q), operation for operation
// (this file is compiled with -ffp-contract=off: no FMA).
__device__ __forceinline__ bool edge_pair(const EdgeArgs& E, const EdgePx& p, const EdgePx& q) {
  bool f = false;
  if (E.edges & RM_AA_EDGE_ID) f |= __float_as_int(p.a.y) != __float_as_int(q.a.y);
  if (E.edges & (RM_AA_EDGE_DEPTH | RM_AA_EDGE_NORMAL)) {
    const bool hit = p.a.x != -1.0f && q.a.x != -1.0f;
    if (E.edges & RM_AA_EDGE_DEPTH) f |= hit && fabsf(p.a.x - q.a.x) > E.depth_rel * fminf(p.a.x, q.a.x);
    if (E.edges & RM_AA_EDGE_NORMAL) f |= hit && (p.a.z * q.a.z + p.a.w * q.a.w) + p.b.x * q.b.x < E.normal_cos;
  }
  if (E.edges & RM_AA_EDGE_ALBEDO) f |= (p.b.y != q.b.y) | (p.b.z != q.b.z) | (p.b.w != q.b.w);
  if (E.edges & RM_AA_EDGE_COLOR) f |= adapt_differs(p.w, q.w, E.color_threshold);
  return f;
}

template <bool EXCHANGE>
__global__ __launch_bounds__(64 * kAdaptWaves) void k_adapt_classify_edges(AdaptArgs A, EdgeArgs E) {
  int px, py;
  const bool in = adapt_pixel(A, px, py);
  const int lane = threadIdx.x & 63;
  // the pairs with the right, upper, left and lower neighbour
  bool fr = false, fu = false, fl = false, fd = false;
  if (in) {
    const size_t w = (size_t)A.width, i = (size_t)py * w + (size_t)px;
    const EdgePx p = edge_load(E, i);
    if (px + 1 < A.width) fr = edge_pair(E, p, edge_load(E, i + 1));
    if (py + 1 < A.height) fu = edge_pair(E, p, edge_load(E, i + w));
    // (EXCHANGE: the neighbour is another tile's pixel, only in the left column / bottom row)
    if (px > 0 && (!EXCHANGE || (lane & 7) == 0)) fl = edge_pair(E, p, edge_load(E, i - 1));
    if (py > 0 && (!EXCHANGE || lane < 8)) fd = edge_pair(E, p, edge_load(E, i - w));
  }
  if constexpr (EXCHANGE) {
    // lane - 1 holds the pixel to the left and has tested (left, p) as its (p, right);
    // lane - 8 the pixel below.  A lane inside the frame has both inside it too.
    const unsigned long long r = __ballot(fr), u = __ballot(fu);
    if (lane & 7) fl = ((r >> ((lane - 1) & 63)) & 1ull) != 0;
    if (lane >= 8) fd = ((u >> ((lane - 8) & 63)) & 1ull) != 0;
  }
  adapt_flag(A, in, px, py, fr | fu | fl | fd);
}

}  // namespace rmd

namespace rm {

// The flags of E's criteria into A's mask and tile counts; launch_adapt_list
// (rm_adaptive.hip) follows.  exchange: the two-pair form (the default).
hipError_t launch_adapt_edges(const rmd::AdaptArgs& A, const rmd::EdgeArgs& E, bool exchange, hipStream_t s) {
  const unsigned tiles_y = (unsigned)((A.height + rmd::kAdaptTile - 1) / rmd::kAdaptTile);
  const dim3 tiles((unsigned)((A.tiles_x + rmd::kAdaptWaves - 1) / rmd::kAdaptWaves), tiles_y), wg(64 * rmd::kAdaptWaves);
  if (exchange)
    hipLaunchKernelGGL(rmd::k_adapt_classify_edges<true>, tiles, wg, 0, s, A, E);
  else
    hipLaunchKernelGGL(rmd::k_adapt_classify_edges<false>, tiles, wg, 0, s, A, E);
  return hipGetLastError();
}

}  // namespace rm
