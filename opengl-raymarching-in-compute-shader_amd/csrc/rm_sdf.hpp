// rm_sdf.hpp — SDF field queries (rm_sdf_points, rm_sdf_grid; include/rm_api.h):
// the four kernels' bodies, written once over Fast and Scene (rm_trace.hpp).
// k_sdf_points / k_sdf_grid (rm_sdf.hip, the built-in scene) and
// k_table_sdf_points / k_table_sdf_grid (rm_table_sdf.hip, runtime scene tables)
// evaluate sdf(p) (glsl:107-123) and GetNormal(p) (glsl:278-288) at
// caller-supplied points or on a regular grid, one point per lane in one-wave
// workgroups, with the render kernels' exact evaluations (Fast's dist / attrs /
// field_normal: scene_cull / normal_samples, Table::dist / tnormal).
//
// Those evaluations cull with bounds stated for finite points whose squares stay
// far from overflow.  sdf_fast_ok() is the predicate under which they hold
// (DESIGN.md §4.11); a lane that fails it runs the literal evaluation of
// rm_trace.hpp (BuiltinLit / TableLit, lit_normal) instead, in the same kernel
// after the fast lanes, so inf, NaN and huge points get the oracle's answer.
#pragma once

#include "rm_sdf_args.hpp"
#include "rm_trace.hpp"

namespace rmd {

// The fast lanes: finite points with |p|_1 <= 2^20.  A NaN
// fails the compare; an infinite component makes the sum infinite.
__device__ __forceinline__ bool sdf_fast_ok(f3 p) {
  return (fabsf(p.x) + fabsf(p.y)) + fabsf(p.z) <= 0x1p20f;
}

// Grid coordinate idx of one axis: one IEEE multiply, then one IEEE add (no
// contraction: Makefile).  idx <= 2^24, so (float)idx is exact.
__device__ __forceinline__ float sdf_grid_coord(float origin, float step, int idx) {
  const float m = (float)idx * step;
  return origin + m;
}

// A point's record before its fields are set: there is no miss, color is always 0.
__device__ __forceinline__ TraceRec sdf_rec() {
  const f3 z = mk(0.0f, 0.0f, 0.0f);
  return TraceRec{0.0f, 0, 0.0f, z, z, z};
}
// The record's store is a ray hit's: three 16-byte stores (trace_store).
__device__ __forceinline__ void sdf_store(float4* out, int64_t i, const TraceRec& r) { trace_store(out, i, r); }

// One point of a lane outside sdf_fast_ok: sdf(p) as the GLSL writes it, every
// entry, opU in order (a NaN distance loses every <, so the last entry wins).
template <class Scene>
__device__ __forceinline__ TraceRec lit_sdf(const Scene& sc, f3 p, uint32_t flags) {
  TraceRec r = sdf_rec();
  int k;
  r.t = sc.dist(p, k);
  sc.attrs(k, p, r.id, r.material, r.albedo);
  if (flags & RM_SDF_NORMAL) r.normal = lit_normal(sc, p);
  return r;
}

// The point kernels' body: one point per lane, 64 consecutive points per
// one-wave workgroup; the flags are uniform.
template <class Fast, class Lit>
__device__ __forceinline__ void sdf_points_body(const SdfPointArgs& A, const Fast& fast, const Lit& lit) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const f3 p = trace_load3(A.points, i);
  const uint32_t flags = A.flags;
  const bool ok = sdf_fast_ok(p);
  TraceRec r = sdf_rec();
  if (ok) {
    int k;
    r.t = fast.dist(p, k);
    fast.attrs(k, p, r.id, r.material, r.albedo);
    if (flags & RM_SDF_NORMAL) r.normal = fast.field_normal(p, r.t);
  }
  // the lanes outside the predicate, after the fast ones
  if (!ok) r = lit_sdf(lit, p, flags);
  sdf_store(A.out, i, r);
}

// The grid kernels' evaluation of one point: the distance, and the id of its opU winner.
template <class Fast, class Lit>
struct SdfGridEval {
  Fast fast;
  Lit lit;
  __device__ __forceinline__ SdfGridEval(const Fast& f, const Lit& l) : fast(f), lit(l) {}
  __device__ __forceinline__ void operator()(f3 p, float& d, int& id) const {
    const bool ok = sdf_fast_ok(p);
    int k = 0;
    if (ok) d = fast.dist(p, k);
    if (!ok) d = lit.dist(p, k);
    id = lit.id(k);
  }
};

// The grid kernels' body around one evaluation `eval(p, d, id)`: the wave's
// (row, x-block) pairs, G.nwg of them taken with a grid stride (the launch holds
// at most kSdfGridMaxWg workgroups: a dispatch counts work-items in 32 bits, so
// 64-lane workgroups stop at 2^26 - 1 while rows alone may reach 2^31 - 1); per
// pair the lane's points, their values kept by selects (no indexed array, no
// scratch), and the stores.  Lanes past the row's end sit the pair out.
template <class Eval>
__device__ __forceinline__ void sdf_grid_body(const SdfGridArgs& G, Eval eval) {
  for (uint32_t b = blockIdx.x; b < G.nwg; b += gridDim.x) {
    const uint32_t row = b / G.bpr, xb = b - row * G.bpr;
    const int iz = (int)(row / (uint32_t)G.ny), iy = (int)(row - (uint32_t)iz * (uint32_t)G.ny);
    const int x0 = (int)(xb * 64u + threadIdx.x) * G.xpl;
    if (x0 < G.nx) {
      const float py = sdf_grid_coord(G.origin[1], G.step[1], iy);
      const float pz = sdf_grid_coord(G.origin[2], G.step[2], iz);
      float d0 = 0.0f, d1 = 0.0f, d2 = 0.0f, d3 = 0.0f;
      int k0 = 0, k1 = 0, k2 = 0, k3 = 0;
#pragma unroll 1
      for (int j = 0; j < G.xpl; ++j) {
        float d;
        int id;
        eval(mk(sdf_grid_coord(G.origin[0], G.step[0], x0 + j), py, pz), d, id);
        d0 = j == 0 ? d : d0;
        d1 = j == 1 ? d : d1;
        d2 = j == 2 ? d : d2;
        d3 = j == 3 ? d : d3;
        k0 = j == 0 ? id : k0;
        k1 = j == 1 ? id : k1;
        k2 = j == 2 ? id : k2;
        k3 = j == 3 ? id : k3;
      }
      const size_t at = (size_t)row * (size_t)G.nx + (size_t)x0;  // < 2^31
      if (G.xpl == 4) {
        if (G.dist) *reinterpret_cast<float4*>(G.dist + at) = make_float4(d0, d1, d2, d3);
        if (G.ids) *reinterpret_cast<int4*>(G.ids + at) = make_int4(k0, k1, k2, k3);
      } else {
        if (G.dist) G.dist[at] = d0;
        if (G.ids) G.ids[at] = k0;
      }
    }
  }
}

// The launch wrappers' packing; lds is the kernel's dynamic LDS bytes.
// n >= 1 points; device pointers, out 16-byte aligned.
inline hipError_t launch_sdf_points_kernel(void (*kernel)(Frame, SdfPointArgs), size_t lds, const Frame& F,
                                           const void* points, void* out, int64_t n, uint32_t flags, hipStream_t s) {
  const SdfPointArgs A{static_cast<const float*>(points), static_cast<float4*>(out), (int32_t)n, flags};
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, F, A);
  return hipGetLastError();
}
// Every dim >= 1; min(G.nwg, kSdfGridMaxWg) workgroups, each taking its pairs with a grid stride.
inline hipError_t launch_sdf_grid_kernel(void (*kernel)(Frame, SdfGridArgs), size_t lds, const Frame& F,
                                         const SdfGridArgs& G, hipStream_t s) {
  const unsigned blocks = G.nwg < kSdfGridMaxWg ? G.nwg : kSdfGridMaxWg;
  hipLaunchKernelGGL(kernel, dim3(blocks), dim3(64), lds, s, F, G);
  return hipGetLastError();
}

}  // namespace rmd
