// rm_table_lit.hpp — TableLit and TableFast: a runtime scene table as the literal
// path's Scene and as the fast path's Fast (rm_trace.hpp), shared by k_table_trace
// (rm_table_trace.hip), the table sdf kernels (rm_table_sdf.hip) and
// k_table_adapt_refine (rm_table_adaptive.hip).  Include it after rm_table.hip,
// whose Table it reads.
#pragma once

#include "rm_trace.hpp"

namespace rmd {

// The table for the literal path: every entry at every point, opU in table
// order (Table::dist_mask over all entries; prim_dist's full-range form is the
// GLSL's operations over the whole float range already).
struct TableLit {
  const Table& S;
  __device__ __forceinline__ float dist(f3 p, int& k) const {
    return S.dist_mask(p, S.n >= 32 ? 0xffffffffu : (1u << S.n) - 1u, k);
  }
  __device__ __forceinline__ int id(int k) const { return S.id(k); }
  __device__ __forceinline__ void attrs(int k, f3 p, int& id, float& material, f3& color) const {
    id = S.id(k);
    material = S.material(k);
    color = S.color(k, p);
  }
};

// The staged table for the fast path.  One instance serves every table:
// EX_MAX_SLOTS lazy slots hold any table's, and TLazy is the march every table
// can take (the reference-shaped and plane-bounded shapes are frame
// optimisations; all three compute the same values).
// It holds the Table itself (the kernel stages into it: TableFast{F, stage(F, lds)}),
// not a reference: tmarch / tnormal / tshadow / trender are plain __device__
// functions here, inlined on cost, and the inliner credits their reads of S only
// when it can trace S to a local of the kernel.  Behind a reference member they
// stay calls that take the Table through scratch memory (432 B per lane).
struct TableFast {
  static constexpr int KL = rm::EX_MAX_SLOTS;
  const Frame& F;
  const Table S;
  __device__ __forceinline__ FastHit march(f3 ro, f3 rd, bool reflected) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    const THit h = tmarch<false, KL, 0>(S, ro, rd, reflected, c);
    return FastHit{h.t, h.id, h.material, h.color, h.d};
  }
  __device__ __forceinline__ f3 normal(f3 pos, float d) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return tnormal<false>(S, pos, c, true, d);
  }
  __device__ __forceinline__ float shadow(f3 ro, f3 rd) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return tshadow<false, KL>(F, S, ro, rd, c);
  }
  __device__ __forceinline__ f3 render(f3 ro, f3 rd) const {
    Cnt c = {0, 0, 0, 0, 0, 0};
    return trender<false, KL, 0>(F, S, ro, rd, c);
  }
  // The table term of the predicate for RM_TRACE_SHADOW.
  // softshadow has no escape test, and a table need not have the built-in floor
  // that bounds its steps: along a ray that leaves every entry behind t grows
  // geometrically, p(t) overflows within the 16 steps, and the GLSL's answer is
  // then what inf and NaN distances make of it (a plane with a negative
  // coefficient on the axis that overflows first: -inf, 0.05), where tshadow has
  // left through table_exit_T with res.  Every entry's value is at most
  // L (|p|_1 + 2 S) (L = EX_LIP >= 1, S = EX_S >= |c|_1 + the sum of the entry's
  // |parameters|: a bounded entry is below |q| + S, a capsule |q - a| + |ba|, a plane
  // |n| |q| + |w|), so a step is at most b + (g - 1) t with b = L (|ro|_1 + 2 S),
  // g = 1 + L |rd|_1, t <= 16 b g^15 after 16 steps and |p|_1 <= 17 b g^16 / L.
  // b g^17 <= 2^56 keeps |p|_1 below 2^61 (the float error of the values, 2^-12
  // relative, is inside 17 < 32) and every square in an sdf finite, which is what
  // the bounds of tshadow assume; past it the lane marches literally, 16 steps over
  // every entry.  An overflow of the product is +inf and fails; a table without
  // valid bounds fails too.
  __device__ __forceinline__ bool shadow_ok(f3 ro, f3 rd) const {
    const float* ex = S.exits();
    if (ex[rm::EX_VALID] == 0.0f) return false;
    const float ro1 = (fabsf(ro.x) + fabsf(ro.y)) + fabsf(ro.z);
    const float rd1 = (fabsf(rd.x) + fabsf(rd.y)) + fabsf(rd.z);
    const float g = 1.0f + ex[rm::EX_LIP] * rd1, b = ex[rm::EX_LIP] * (ro1 + 2.0f * ex[rm::EX_S]);
    const float g2 = g * g, g4 = g2 * g2, g8 = g4 * g4;
    return (g8 * g8) * g * b <= 0x1p56f;
  }
  // Table::dist is the table's sdf with per-point culling; tnormal's centre
  // sample is that value at the same point, and its tnormalize is the IEEE
  // v * (1 / sqrt(dot)) over the whole float range already.
  __device__ __forceinline__ float dist(f3 p, int& k) const { return S.dist(p, k); }
  __device__ __forceinline__ void attrs(int k, f3 p, int& id, float& material, f3& color) const {
    TableLit{S}.attrs(k, p, id, material, color);
  }
  __device__ __forceinline__ f3 field_normal(f3 p, float d) const { return normal(p, d); }
};

}  // namespace rmd
