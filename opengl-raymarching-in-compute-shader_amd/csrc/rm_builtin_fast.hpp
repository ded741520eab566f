// rm_builtin_fast.hpp — BuiltinFast: the built-in scene as the query kernels'
// fast-path scene (Fast, rm_trace.hpp), shared by k_trace (rm_trace.hip) and the
// sdf kernels (rm_sdf.hip).  Include it after rm_kernels.hip, whose march /
// get_normal / softshadow / render it calls.
#pragma once

#include "rm_trace.hpp"

namespace rmd {

struct BuiltinFast {
  const Frame& F;
  __device__ __forceinline__ FastHit march(f3 ro, f3 rd, bool reflected) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    FastHit h;
    h.d = 0.0f;
    h.t = rmd::march<false, false, false>(F, ro, rd, reflected, h.id, h.color, c, h.d);
    h.material = (h.t != -1.0f && h.id == 7) ? 0.0f : 1.0f;
    return h;
  }
  __device__ __forceinline__ f3 normal(f3 pos, float d) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return get_normal<false, true>(F, pos, c, d);
  }
  __device__ __forceinline__ float shadow(f3 ro, f3 rd) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return softshadow<false>(F, ro, rd, ray_rdl(rd), c);
  }
  __device__ __forceinline__ f3 render(f3 ro, f3 rd) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return rmd::render<false>(F, ro, rd, c);
  }
  // trace_fast_ok is the whole predicate: the floor bounds a shadow march's steps
  // (DESIGN.md §4.9 item 3).
  __device__ __forceinline__ bool shadow_ok(f3, f3) const { return true; }
  // sdf(p): value and opU id with bounding-ball culling.
  __device__ __forceinline__ float dist(f3 p, int& k) const { return scene_cull<true>(p, F.blend, F.omblend, k); }
  __device__ __forceinline__ void attrs(int k, f3 p, int& id, float& material, f3& color) const {
    BuiltinLit{F.blend, F.omblend}.attrs(k, p, id, material, color);
  }
  // GetNormal(p): get_normal<false, false>'s two steps, the samples with shared
  // culling and the normalisation, taken apart for the gradient between them.
  // normalize()'s rcp_of_sqrt equals the IEEE 1 / sqrt for roots in
  // [2^-74.5, 2^64], the roots of positive finite sums.  A point of a field query
  // is no march hit: far from the origin the 0.001 offsets vanish and the
  // gradient is exactly 0 (the oracle's normal: 0 * inf = NaN), and a gradient
  // whose squares underflow has a zero sum under non-zero components (the
  // oracle's: +-inf and NaN).  Such sums take the IEEE operations.
  __device__ __forceinline__ f3 field_normal(f3 p, float) const {
    float c0, vx, vy, vz;
    normal_samples<false>(p, F.blend, F.omblend, c0, vx, vy, vz);
    const f3 g = subs(mk(vx, vy, vz), c0);
    const float dd = dot(g, g);
    if ((dd > 0.0f) & (dd < __builtin_huge_valf())) return normalize(g);
    return lit_normalize(g);
  }
};

// k_pixel's render of a primary ray (the projection bound of the miss exit too,
// rm_kernels.hip march): what the one-sample pattern kernels render with
// (rm_pattern.hip, rm_adaptive_pattern.hip).
struct BuiltinPrimary {
  const Frame& F;
  __device__ __forceinline__ f3 render(f3 ro, f3 rd) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return rmd::render<false, true>(F, ro, rd, c);
  }
};

}  // namespace rmd
