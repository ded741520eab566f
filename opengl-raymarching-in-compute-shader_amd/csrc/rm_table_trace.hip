// rm_table_trace.hip — k_table_trace: ray queries against a runtime scene table
// (rm_trace_rays, include/rm_api.h).
//
// A translation unit of its own, so that rm_table.o's kernels are what they were
// without it, and outside the hiprtc sources: a context with rm_scene_specialize
// on traces through this generic, LDS-staged code too.  The device code is
// rm_table.hip's (tmarch / tnormal / tshadow / trender over the staged Table),
// included without its kernels' launch wrappers.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_trace.hpp"
#include "rm_table_lit.hpp"

namespace rmd {

// As k_trace (rm_trace.hip), over the staged table.  One instance serves every
// table: EX_MAX_SLOTS lazy slots hold any table's, and TLazy is the march every
// table can take (the reference-shaped and plane-bounded shapes are frame
// optimisations; all three compute the same values).
constexpr int kTraceKL = rm::EX_MAX_SLOTS;
__global__ __launch_bounds__(64) void k_table_trace(Frame F, TraceArgs A) {
  extern __shared__ float lds[];
  const Table S = stage(F, lds);  // (barriers: before any lane leaves)
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const f3 ro = trace_load3(A.origins, i), rd = trace_load3(A.dirs, i);
  const uint32_t flags = A.flags;
  const bool fast = trace_fast_ok(ro, rd);
  TraceRec r = trace_miss();
  if (fast) {
    TCnt c = {0, 0, 0, 0, 0, 0};
    if (flags & RM_TRACE_SHADOW) {
      r.t = tshadow<false, kTraceKL>(F, S, ro, rd, c);
      r.id = 0;
      r.material = 0.0f;
    } else {
      const THit h = tmarch<false, kTraceKL, 0>(S, ro, rd, (flags & RM_TRACE_REFLECTED) != 0, c);
      r.t = h.t;
      r.id = h.id;
      r.material = h.material;
      r.albedo = h.color;
      if ((flags & RM_TRACE_NORMAL) && h.t != -1.0f)
        r.normal = tnormal<false>(S, add(ro, muls(rd, h.t)), c, true, h.d);
      if (flags & RM_TRACE_SHADE) r.color = trender<false, kTraceKL, 0>(F, S, ro, rd, c);
    }
  }
  if (!fast) r = lit_trace(F, TableLit{S}, ro, rd, flags);
  trace_store(A.hits, i, r);
}

}  // namespace rmd

namespace rm {

// n >= 1 rays against the table F.scene; device pointers, hits 16-byte aligned.
hipError_t launch_table_trace(const rmd::Frame& F, const void* origins, const void* dirs, void* hits,
                              int64_t n, uint32_t flags, hipStream_t s) {
  const rmd::TraceArgs A{static_cast<const float*>(origins), static_cast<const float*>(dirs),
                         static_cast<float4*>(hits), (int32_t)n, flags};
  // the table, then the lazy slots' balls (Table::sb), as the render kernels stage them
  const size_t lds = (((rm::scene_words(F.nprims) + 3) & ~(size_t)3) + 4 * (size_t)rm::EX_MAX_SLOTS) * sizeof(float);
  hipLaunchKernelGGL(rmd::k_table_trace, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, F, A);
  return hipGetLastError();
}

}  // namespace rm
