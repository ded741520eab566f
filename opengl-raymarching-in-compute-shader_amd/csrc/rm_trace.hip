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

// The built-in scene (glsl:107-123) for the literal path: every primitive, every
// operation as the GLSL writes it.  scene_exact (rm_scene.hpp) is the same sdf for
// finite points only: its v_min / v_max drop a NaN operand, its plane is p.y + 5.5
// (the dot product's x * 0 and z * 0 are NaN for an infinite p) and sqrt_core
// takes finite sums.
struct BuiltinLit {
  float blend, omblend;
  __device__ __forceinline__ float dist(f3 p, int& id) const {
    auto opu = [&](float d, float v, int k) {  // opU glsl:105: (d1 < d2) ? d1 : d2
      const bool keep = d < v;
      id = keep ? id : k;
      return keep ? d : v;
    };
    id = 0;
    float d = lit_len(sub(p, mk(15.0f, 0.0f, -10.0f))) - 3.0f;                    // glsl:111
    d = opu(d, lit_len(sub(p, mk(-25.0f, 0.0f, -10.0f))) - 3.0f, 1);              // glsl:112
    {                                                                              // glsl:115-117
      const f3 q = sub(p, mk(-5.0f, 0.0f, -10.0f));
      const f3 e = mk(fabsf(q.x) - 3.0f, fabsf(q.y) - 2.5f, fabsf(q.z) - 2.5f);
      const float box = gmin(gmax(e.x, gmax(e.y, e.z)), 0.0f) +
                        lit_len(mk(gmax(e.x, 0.0f), gmax(e.y, 0.0f), gmax(e.z, 0.0f)));
      const float sph = lit_len(q) - 3.0f;
      d = opu(d, box * omblend + sph * blend, 4);
    }
    {                                                                              // glsl:119
      const f3 q = sub(p, mk(-5.0f, 0.0f, 10.0f));  // sdTorus(q.xzy, (2.5, 0.5))
      const float l = lit_sqrt(q.x * q.x + q.y * q.y) - 2.5f;
      d = opu(d, lit_sqrt(l * l + q.z * q.z) - 0.5f, 5);
    }
    {                                                                              // glsl:120
      const f3 pa = sub(sub(p, mk(-5.0f, -2.0f, -30.0f)), mk(CAP_AX, CAP_AY, CAP_AZ));
      const f3 ba = mk(CAP_BAX, CAP_BAY, CAP_BAZ);
      const float h = gmin(gmax(dot(pa, ba) / dot(ba, ba), 0.0f), 1.0f);
      d = opu(d, lit_len(sub(pa, muls(ba, h))) - 1.0f, 6);
    }
    return opu(d, dot(p, mk(0.0f, 1.0f, 0.0f)) + 5.5f, 7);                         // glsl:85,121
  }
  __device__ __forceinline__ void attrs(int k, f3 p, int& id, float& material, f3& color) const {
    id = k;
    material = k == 7 ? 0.0f : 1.0f;  // MATTE: the floor alone
    color = hit_color(k, p);
  }
};

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
