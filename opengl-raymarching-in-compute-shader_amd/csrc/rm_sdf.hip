// rm_sdf.hip — k_sdf_points / k_sdf_grid: SDF field queries against the built-in
// scene (rm_sdf_points, rm_sdf_grid; include/rm_api.h).
//
// A translation unit of its own, as rm_trace.hip: rm_kernels.hip's device code
// with both of its *_ONLY switches set, so that no existing object changes.
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_sdf.hpp"

namespace rmd {

// sdf(p) of a fast lane: value and opU id with bounding-ball culling.
__device__ __forceinline__ void sdf_fast(const Frame& F, f3 p, float& d, int& id) {
  d = scene_cull<true>(p, F.blend, F.omblend, id);
}

// GetNormal(p) of a fast lane: get_normal<false, false>'s two steps, the samples
// with shared culling and the normalisation, taken apart for the gradient
// between them.  normalize()'s rcp_of_sqrt equals the IEEE 1 / sqrt for roots in
// [2^-74.5, 2^64], the roots of positive finite sums.  A point of a field query
// is no march hit: far from the origin the 0.001 offsets vanish and the
// gradient is exactly 0 (the oracle's normal: 0 * inf = NaN), and a gradient
// whose squares underflow has a zero sum under non-zero components (the
// oracle's: +-inf and NaN).  Such sums take the IEEE operations.
__device__ __forceinline__ f3 sdf_fast_normal(const Frame& F, f3 p) {
  float c0, vx, vy, vz;
  normal_samples<false>(p, F.blend, F.omblend, c0, vx, vy, vz);
  const f3 g = subs(mk(vx, vy, vz), c0);
  const float dd = dot(g, g);
  if ((dd > 0.0f) & (dd < __builtin_huge_valf())) return normalize(g);
  return lit_normalize(g);
}

// One point per lane, 64 consecutive points per one-wave workgroup; the flags
// are uniform.  Of the query Frame only blend / omblend are read.
__global__ __launch_bounds__(64) void k_sdf_points(Frame F, SdfPointArgs A) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const f3 p = trace_load3(A.points, i);
  const uint32_t flags = A.flags;
  const bool fast = sdf_fast_ok(p);
  TraceRec r = sdf_rec();
  if (fast) {
    sdf_fast(F, p, r.t, r.id);
    r.material = r.id == 7 ? 0.0f : 1.0f;  // MATTE: the floor alone
    r.albedo = hit_color(r.id, p);
    if (flags & RM_SDF_NORMAL) r.normal = sdf_fast_normal(F, p);
  }
  // the lanes outside the predicate, after the fast ones
  if (!fast) r = lit_sdf(BuiltinLit{F.blend, F.omblend}, p, flags);
  sdf_store(A.out, i, r);
}

// The grid: the coordinates come from the lane's indices, no input array.
__global__ __launch_bounds__(64) void k_sdf_grid(Frame F, SdfGridArgs G) {
  sdf_grid_body(G, [&](f3 p, float& d, int& id) {
    const bool fast = sdf_fast_ok(p);
    if (fast) sdf_fast(F, p, d, id);
    if (!fast) d = BuiltinLit{F.blend, F.omblend}.dist(p, id);  // (its opU winner is the id)
  });
}

}  // namespace rmd

namespace rm {

// n >= 1 points; device pointers, out 16-byte aligned.
hipError_t launch_sdf_points(const rmd::Frame& F, const void* points, void* out, int64_t n, uint32_t flags,
                             hipStream_t s) {
  const rmd::SdfPointArgs A{static_cast<const float*>(points), static_cast<float4*>(out), (int32_t)n, flags};
  hipLaunchKernelGGL(rmd::k_sdf_points, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, F, A);
  return hipGetLastError();
}

// Every dim >= 1; min(G.nwg, kSdfGridMaxWg) workgroups, each taking its pairs with a grid stride.
hipError_t launch_sdf_grid(const rmd::Frame& F, const rmd::SdfGridArgs& G, hipStream_t s) {
  const unsigned blocks = G.nwg < rmd::kSdfGridMaxWg ? G.nwg : rmd::kSdfGridMaxWg;
  hipLaunchKernelGGL(rmd::k_sdf_grid, dim3(blocks), dim3(64), 0, s, F, G);
  return hipGetLastError();
}

}  // namespace rm
