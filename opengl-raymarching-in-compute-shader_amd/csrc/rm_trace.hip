// rm_trace.hip — k_trace: ray queries against the built-in scene (rm_trace_rays,
// include/rm_api.h).
//
// A translation unit of its own, so that the render kernels' code objects
// (rm_kernels.o, rm_kernels_aa.o) are what they were without it.  The device
// code is rm_kernels.hip's, included with both of its *_ONLY switches set: that
// leaves its templates (march, get_normal, softshadow, render) and drops every
// kernel and launch wrapper of its own.
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

#include "rm_trace.hpp"

namespace rmd {

// (BuiltinLit, the built-in scene of the literal path: rm_trace.hpp)

// One ray per lane, 64 consecutive rays per one-wave workgroup; the flags are
// uniform.  The query Frame has prepv[PREP_VALID] = 0 and unit_rd = 0
// (rm_api_trace.hip): step 0 at the camera and |rd| = 1 are facts about a
// frame's primary rays only.
// 64 VGPRs, 8 waves per SIMD, as the render kernels: no scratch (2 spilled SGPRs),
// and against the 71 registers / 7 waves of an unbounded build -4 % per SHADE trace
// and -6 % per HIT trace of the cfg 2 frame's rays (profiles/r07_ab_trace_waves.txt).
__global__ __launch_bounds__(64, 8) void k_trace(Frame F, TraceArgs A) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const f3 ro = trace_load3(A.origins, i), rd = trace_load3(A.dirs, i);
  const uint32_t flags = A.flags;
  const bool fast = trace_fast_ok(ro, rd);
  TraceRec r = trace_miss();
  if (fast) {
    Cnt c = {0, 0, 0, 0, 0, 0};
    if (flags & RM_TRACE_SHADOW) {
      r.t = softshadow<false>(F, ro, rd, ray_rdl(rd), c);
      r.id = 0;
      r.material = 0.0f;
    } else {
      float dl = 0.0f;
      r.t = march<false, false, false>(F, ro, rd, (flags & RM_TRACE_REFLECTED) != 0, r.id, r.albedo, c, dl);
      r.material = (r.t != -1.0f && r.id == 7) ? 0.0f : 1.0f;
      // (the centre sample of the normal is the march's last distance: the same point)
      if ((flags & RM_TRACE_NORMAL) && r.t != -1.0f)
        r.normal = get_normal<false, true>(F, add(ro, muls(rd, r.t)), c, dl);
      if (flags & RM_TRACE_SHADE) r.color = render<false>(F, ro, rd, c);
    }
  }
  // the lanes outside the predicate, after the fast ones (no vote of theirs is shared)
  if (!fast) r = lit_trace(F, BuiltinLit{F.blend, F.omblend}, ro, rd, flags);
  trace_store(A.hits, i, r);
}

}  // namespace rmd

namespace rm {

// n >= 1 rays; origins / dirs / hits are device pointers, hits 16-byte aligned.
hipError_t launch_trace(const rmd::Frame& F, const void* origins, const void* dirs, void* hits, int64_t n,
                        uint32_t flags, hipStream_t s) {
  const rmd::TraceArgs A{static_cast<const float*>(origins), static_cast<const float*>(dirs),
                         static_cast<float4*>(hits), (int32_t)n, flags};
  hipLaunchKernelGGL(rmd::k_trace, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, F, A);
  return hipGetLastError();
}

}  // namespace rm
