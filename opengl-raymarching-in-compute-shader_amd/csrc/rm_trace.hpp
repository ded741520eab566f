// rm_trace.hpp — ray queries (rm_trace_rays, include/rm_api.h): the two trace
// kernels' body, written once over two scene interfaces.  k_trace (rm_trace.hip,
// the built-in scene) and k_table_trace (rm_table_trace.hip, runtime scene
// tables) march caller-supplied rays, one ray per lane in one-wave workgroups,
// with the render kernels' device code: march / get_normal / softshadow / render
// and their table forms, behind the fast-path interface (Fast, below).
//
// That code cuts work with proofs (lazy culling, the provable-miss, step-cap and
// shadow exits: rm_scene.hpp, rm_table.hip) whose margins are stated for the
// rays a frame casts.  A query ray is any six floats.  trace_fast_ok() is the
// predicate under which every one of those bounds holds (DESIGN.md §4.9 derives
// it); a lane that fails it runs the lit_* functions below instead, in the same
// kernel after the fast lanes: a literal transcription of the GLSL over an exact
// evaluation of the scene, every operation the IEEE one over the whole float
// range (GLSL min / max, IEEE sqrt and division, the plane's full dot product),
// with no culling and no early exit.  It is the oracle's code (oracle/rm_oracle.c)
// line by line, so inf, NaN, zero and huge rays get the reference's answer.
#pragma once

#include "rm_internal.hpp"
#include "rm_scene.hpp"

namespace rmd {

// Kernel arguments beside the Frame.
struct TraceArgs {
  const float* origins;  // [n][3]
  const float* dirs;     // [n][3]
  float4* hits;          // [n] rm_ray_hit, 3 x 16 B each
  int32_t n;
  uint32_t flags;        // RM_TRACE_*, wave-uniform
};

// One rm_ray_hit in registers.
struct TraceRec {
  float t;
  int id;
  float material;
  f3 albedo, normal, color;
};
// The GLSL's dummy RayHit {-1, 0, -1, 1.0} (glsl:128), the other fields 0.
__device__ __forceinline__ TraceRec trace_miss() {
  const f3 z = mk(0.0f, 0.0f, 0.0f);
  return TraceRec{-1.0f, -1, 1.0f, z, z, z};
}

// The fast lanes: finite rays with |ro|_1 <= 2^20 and
// 2^-12 <= |rd| <= 2^12.  A NaN fails every compare; an infinite component makes
// its sum infinite.
__device__ __forceinline__ bool trace_fast_ok(f3 ro, f3 rd) {
  const float ro1 = (fabsf(ro.x) + fabsf(ro.y)) + fabsf(ro.z);
  const float dd = dot(rd, rd);
  return (ro1 <= 0x1p20f) & (dd >= 0x1p-24f) & (dd <= 0x1p24f);
}

__device__ __forceinline__ f3 trace_load3(const float* p, int64_t i) {
  return mk(p[3 * i], p[3 * i + 1], p[3 * i + 2]);
}
// Three 16-byte stores: a wave's 64 records are 3 KiB of contiguous memory.
__device__ __forceinline__ void trace_store(float4* hits, int64_t i, const TraceRec& r) {
  float4* o = hits + 3 * i;
  o[0] = make_float4(r.t, __int_as_float(r.id), r.material, r.albedo.x);
  o[1] = make_float4(r.albedo.y, r.albedo.z, r.normal.x, r.normal.y);
  o[2] = make_float4(r.normal.z, r.color.x, r.color.y, r.color.z);
}

// ---- the fast path ---------------------------------------------------------------------
// What a query family calls on a lane inside its predicate: the render kernels'
// device code, proofs and all, in the instantiations the adapters name.  Every
// call holds its own work counter (Cnt / Cnt: no counting build).
// Fast: FastHit march(f3 ro, f3 rd, bool reflected) const
//       f3 normal(f3 pos, float d) const    GetNormal at a march's hit, d its last distance (the centre sample),
//       float shadow(f3 ro, f3 rd) const    softshadow,
//       bool shadow_ok(f3 ro, f3 rd) const  what the scene adds to trace_fast_ok for a RM_TRACE_SHADOW lane,
//       f3 render(f3 ro, f3 rd) const       a primary ray's colour,
//       float dist(f3 p, int& k) const, void attrs(int k, f3 p, int&, float&, f3&) const
//                                           as Scene's below, for the points of sdf_fast_ok (rm_sdf.hpp),
//       f3 field_normal(f3 p, float d) const   GetNormal at such a point, d = dist(p).
// BuiltinFast (rm_builtin_fast.hpp, over rm_kernels.hip) and TableFast
// (rm_table_lit.hpp, over rm_table.hip) implement it.  A new family writes its
// body once over Fast and Scene in its header, and per scene a kernel that calls
// the body and a launch wrapper.
struct FastHit {
  float t;  // -1: no hit
  int id;
  float material;
  f3 color;
  float d;  // a hit's last distance: sdf at the hit point itself
};

// ---- the literal path ------------------------------------------------------------------
// Scene: float dist(f3 p, int& k) const   sdf(p).hitpoint and its opU winner k,
//        int id(int k) const   the winner's id,
//        void attrs(int k, f3 p, int&, float&, f3&) const   the winner's id, material, colour.
struct LitHit {
  float t;
  int id;
  float material;
  f3 color;
};
__device__ __forceinline__ float lit_sqrt(float x) { return __builtin_sqrtf(x); }  // IEEE (Makefile)
__device__ __forceinline__ float lit_len(f3 a) { return lit_sqrt(dot(a, a)); }
__device__ __forceinline__ f3 lit_normalize(f3 a) { return muls(a, 1.0f / lit_sqrt(dot(a, a))); }

// The built-in scene (glsl:107-123) for the literal path: every primitive, every
// operation as the GLSL writes it.  scene_exact (rm_scene.hpp) is the same sdf for
// finite points only: its v_min / v_max drop a NaN operand, its plane is p.y + 5.5
// (the dot product's x * 0 and z * 0 are NaN for an infinite p) and sqrt_core
// takes finite sums.  (k_trace's, rm_trace.hip, and the sdf kernels', rm_sdf.hip.)
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
  __device__ __forceinline__ int id(int k) const { return k; }
  __device__ __forceinline__ void attrs(int k, f3 p, int& id, float& material, f3& color) const {
    id = k;
    material = k == 7 ? 0.0f : 1.0f;  // MATTE: the floor alone
    color = hit_color(k, p);
  }
};

// RayMarch glsl:125-142 / reflectedRay glsl:144-161
template <class Scene>
__device__ __forceinline__ LitHit lit_march(const Scene& sc, f3 ro, f3 rd, bool reflected) {
  const float tmax = reflected ? 200.0f : 400.0f;
  const int nmax = reflected ? 256 : 512;
  float t = 0.0f;
  for (int i = 0; i < nmax; ++i) {
    const f3 p = add(ro, muls(rd, t));
    int k;
    const float d = sc.dist(p, k);
    if (d < 0.000001f * t) {
      LitHit h;
      h.t = t;
      sc.attrs(k, p, h.id, h.material, h.color);
      return h;
    }
    if (d > tmax) break;
    t += d;
  }
  return LitHit{-1.0f, -1, 1.0f, mk(0.0f, 0.0f, 0.0f)};
}

// GetNormal glsl:278-288.  The four samples in one rolled loop (one copy of the
// scene's code), each value kept by a select: no indexed array, no scratch.
template <class Scene>
__device__ __forceinline__ f3 lit_normal(const Scene& sc, f3 pos) {
  float c = 0.0f, vx = 0.0f, vy = 0.0f, vz = 0.0f;
#pragma unroll 1
  for (int j = 0; j < 4; ++j) {
    int k;
    // j = 0: pos itself (pos + 0 would turn a -0 component into +0)
    const f3 q = j == 0 ? pos : add(pos, mk(j == 1 ? 0.001f : 0.0f, j == 2 ? 0.001f : 0.0f, j == 3 ? 0.001f : 0.0f));
    const float d = sc.dist(q, k);
    c = j == 0 ? d : c;
    vx = j == 1 ? d : vx;
    vy = j == 2 ? d : vy;
    vz = j == 3 ? d : vz;
  }
  return lit_normalize(subs(mk(vx, vy, vz), c));
}

// softshadow glsl:201-216
template <class Scene>
__device__ __forceinline__ float lit_shadow(const Scene& sc, f3 ro, f3 rd, float k) {
  float res = 1.0f, t = 0.0f;
  for (int i = 0; i < 16; ++i) {
    int w;
    const float h = sc.dist(add(ro, muls(rd, t)), w);
    if (h < 0.001f) return 0.05f;
    res = gmin(res, k * h / t);
    t += h;
  }
  return res;
}

// getPointLight glsl:253-276 (pow as the kernels evaluate it: gpow, rm_scene.hpp)
__device__ __forceinline__ f3 lit_point_light(const Frame& F, f3 color, f3 normal, f3 pos) {
  const f3 lpos = mk(F.lpos[0], F.lpos[1], F.lpos[2]);
  f3 ambient = mk(F.lamb[0], F.lamb[1], F.lamb[2]);
  const f3 viewDir = lit_normalize(sub(pos, mk(F.cam_pos[0], F.cam_pos[1], F.cam_pos[2])));
  const f3 lightDir = lit_normalize(sub(lpos, pos));
  const float NtoL = gmax(dot(normal, lightDir), 0.0f);
  f3 diffuse = muls(mk(F.ldif[0], F.ldif[1], F.ldif[2]), NtoL);
  const f3 reflectDir = reflect(lightDir, normal);
  const float spec = gpow(gmax(dot(viewDir, reflectDir), 0.0f), 32.0f);
  f3 specular = muls(mk(F.lspec[0], F.lspec[1], F.lspec[2]), spec);
  const float distance = lit_len(sub(lpos, pos));
  const float attenuation = 1.0f / ((F.lconst + F.llin * distance) + F.lquad * (distance * distance));
  diffuse = muls(diffuse, attenuation);
  ambient = muls(ambient, attenuation);
  specular = muls(specular, attenuation);
  return mul(color, add(add(diffuse, ambient), specular));
}

// bounce glsl:163-199.  After a MATTE prevObject every iteration leaves the colour
// as it is (glsl:181, 189-190), so the loop ends there.
template <class Scene>
__device__ __forceinline__ f3 lit_bounce(const Frame& F, const Scene& sc, f3 rayDir, f3 pos, f3 normal, f3 color,
                         const LitHit& primary) {
  float prevMat = primary.material;
  f3 prevColor = primary.color;
  const f3 lpos = mk(F.lpos[0], F.lpos[1], F.lpos[2]);
  for (int i = 1; i <= F.bounces; ++i) {
    if (prevMat == 0.0f) break;
    rayDir = reflect(rayDir, normal);
    LitHit h = lit_march(sc, add(pos, muls(normal, 0.001f)), rayDir, true);
    pos = add(pos, muls(rayDir, h.t));
    normal = lit_normal(sc, pos);
    if (h.t == -1.0f) h.color = subs(mk(0.36f, 0.36f, 0.60f), rayDir.y * 0.2f);
    else h.color = lit_point_light(F, h.color, normal, pos);
    if (h.id == 7 && i < 3) {
      const float sh = lit_shadow(sc, add(pos, muls(normal, 0.02f)), sub(lpos, pos), F.k);
      color = muls(color, sh / (float)i);
    }
    color = add(color, divs(mul(h.color, prevColor), (float)i));
    prevColor = h.color;
    prevMat = h.material;
  }
  return color;
}

// render glsl:218-251; the primary hit comes back in `prim`.
template <class Scene>
__device__ __forceinline__ f3 lit_render(const Frame& F, const Scene& sc, f3 ro, f3 rd, const LitHit& prim) {
  f3 color = subs(mk(0.30f, 0.36f, 0.60f), rd.y * 0.2f);
  if (prim.t != -1.0f) {
    const f3 pos = add(ro, muls(rd, prim.t));
    const f3 normal = lit_normal(sc, pos);
    color = lit_point_light(F, prim.color, normal, pos);
    if (prim.id == 7) {
      const f3 lpos = mk(F.lpos[0], F.lpos[1], F.lpos[2]);
      const float sh = lit_shadow(sc, add(pos, muls(normal, 0.02f)), sub(lpos, pos), F.k);
      return gamma(muls(color, sh));
    }
    if (F.bounces > 0) color = lit_bounce(F, sc, rd, pos, normal, color, prim);
  }
  return gamma(color);
}

// One query of a lane outside trace_fast_ok, by the flags' meaning (rm_api.h).
template <class Scene>
__device__ __forceinline__ TraceRec lit_trace(const Frame& F, const Scene& sc, f3 ro, f3 rd, uint32_t flags) {
  TraceRec r = trace_miss();
  if (flags & RM_TRACE_SHADOW) {
    r.t = lit_shadow(sc, ro, rd, F.k);
    r.id = 0;
    r.material = 0.0f;
    return r;
  }
  const LitHit h = lit_march(sc, ro, rd, (flags & RM_TRACE_REFLECTED) != 0);
  r.t = h.t;
  r.id = h.id;
  r.material = h.material;
  r.albedo = h.color;
  if ((flags & RM_TRACE_NORMAL) && h.t != -1.0f) r.normal = lit_normal(sc, add(ro, muls(rd, h.t)));
  if (flags & RM_TRACE_SHADE) r.color = lit_render(F, sc, ro, rd, h);
  return r;
}

// ---- the kernels' body and launch --------------------------------------------------------
// One ray per lane, 64 consecutive rays per one-wave workgroup; the flags are
// uniform.  The query Frame has prepv[PREP_VALID] = 0 and unit_rd = 0
// (rm_api_trace.hip): step 0 at the camera and |rd| = 1 are facts about a
// frame's primary rays only.
template <class Fast, class Lit>
__device__ __forceinline__ void trace_body(const Frame& F, const TraceArgs& A, const Fast& fast, const Lit& lit) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= A.n) return;
  const f3 ro = trace_load3(A.origins, i), rd = trace_load3(A.dirs, i);
  const uint32_t flags = A.flags;
  // (shadow_ok: the scene's own term for a shadow query, whose march has no escape test)
  const bool ok = trace_fast_ok(ro, rd) && (!(flags & RM_TRACE_SHADOW) || fast.shadow_ok(ro, rd));
  TraceRec r = trace_miss();
  if (ok) {
    if (flags & RM_TRACE_SHADOW) {
      r.t = fast.shadow(ro, rd);
      r.id = 0;
      r.material = 0.0f;
    } else {
      const FastHit h = fast.march(ro, rd, (flags & RM_TRACE_REFLECTED) != 0);
      r.t = h.t;
      r.id = h.id;
      r.material = h.material;
      r.albedo = h.color;
      // (the centre sample of the normal is the march's last distance: the same point)
      if ((flags & RM_TRACE_NORMAL) && h.t != -1.0f) r.normal = fast.normal(add(ro, muls(rd, h.t)), h.d);
      if (flags & RM_TRACE_SHADE) r.color = fast.render(ro, rd);
    }
  }
  // the lanes outside the predicate, after the fast ones (no vote of theirs is shared)
  if (!ok) r = lit_trace(F, lit, ro, rd, flags);
  trace_store(A.hits, i, r);
}

// The launch wrappers' packing: n >= 1 rays; origins / dirs / hits are device
// pointers, hits 16-byte aligned; lds the kernel's dynamic LDS bytes.
inline hipError_t launch_trace_kernel(void (*kernel)(Frame, TraceArgs), size_t lds, const Frame& F,
                                      const void* origins, const void* dirs, void* hits, int64_t n, uint32_t flags,
                                      hipStream_t s) {
  const TraceArgs A{static_cast<const float*>(origins), static_cast<const float*>(dirs), static_cast<float4*>(hits),
                    (int32_t)n, flags};
  hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), lds, s, F, A);
  return hipGetLastError();
}

}  // namespace rmd
