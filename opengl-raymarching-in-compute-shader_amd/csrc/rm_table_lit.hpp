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
    TCnt c = {0, 0, 0, 0, 0, 0};
    const THit h = tmarch<false, KL, 0>(S, ro, rd, reflected, c);
    return FastHit{h.t, h.id, h.material, h.color, h.d};
  }
  __device__ __forceinline__ f3 normal(f3 pos, float d) const {
    TCnt c = {0, 0, 0, 0, 0, 0};
    return tnormal<false>(S, pos, c, true, d);
  }
  __device__ __forceinline__ float shadow(f3 ro, f3 rd) const {
    TCnt c = {0, 0, 0, 0, 0, 0};
    return tshadow<false, KL>(F, S, ro, rd, c);
  }
  __device__ __forceinline__ f3 render(f3 ro, f3 rd) const {
    TCnt c = {0, 0, 0, 0, 0, 0};
    return trender<false, KL, 0>(F, S, ro, rd, c);
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
