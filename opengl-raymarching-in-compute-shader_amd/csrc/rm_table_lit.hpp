// rm_table_lit.hpp — TableLit: a runtime scene table as the literal path's Scene
// (rm_trace.hpp), shared by k_table_trace (rm_table_trace.hip) and the table sdf
// kernels (rm_table_sdf.hip).  Include it after rm_table.hip, whose Table it reads.
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
  __device__ __forceinline__ void attrs(int k, f3 p, int& id, float& material, f3& color) const {
    id = S.id(k);
    material = S.material(k);
    color = S.color(k, p);
  }
};

}  // namespace rmd
