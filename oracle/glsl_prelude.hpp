/*
 * glsl_prelude.hpp — TEST INFRASTRUCTURE ONLY.
 *
 * Gives the GLSL *language* its C++ meaning, so that compute-shader text
 * rewritten by oracle/glsl_rewrite.py compiles as C++20 against GLM (the
 * library the reference vendors to give C++ the GLSL vocabulary).  Nothing in
 * this file knows the scene, the uniforms or any constant of a shader: it holds
 * storage qualifiers, the image and work-group built-ins, the two conversions
 * GLSL performs implicitly and C++ templates cannot deduce, and the built-ins
 * DESIGN.md §2 defines otherwise than GLM does.
 *
 * -DGLSL_REF_PURE_GLM leaves every built-in to GLM (oracle/_ref/glsl_ref_glm).
 *
 * Include it at file scope, then open `namespace glslref`, include the
 * rewritten text there, and `#include "glsl_prelude.hpp"` again with
 * GLSL_PRELUDE_END defined to take the qualifier macros away.  The namespace
 * keeps the shader's main() and its uniforms from colliding with C's names.
 */
#ifndef GLSL_PRELUDE_END
#ifndef GLSL_PRELUDE_HPP
#define GLSL_PRELUDE_HPP

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define GLM_FORCE_SWIZZLE /* .xyz() members */
#define GLM_FORCE_PURE    /* scalar code only: one IEEE operation per GLSL operation */
#include <glm/glm.hpp>

namespace glslref {
using namespace glm;

/* ---- storage and layout qualifiers: plain globals in C++ ------------------- */
#define uniform
#define layout(...)
#define in

/* ---- image load/store (GLSL 4.50 §8.12), one bound RGBA32F image ----------- */
struct image2D {
  int width = 0, height = 0;
  float *texels = nullptr;          /* [height][width][4] */
  ivec2 expect = ivec2(-1, -1);     /* the pixel this invocation owns (the dispatcher sets it) */
  long stores = 0;
};
inline ivec2 imageSize(const image2D &img) { return ivec2(img.width, img.height); }
inline void imageStore(image2D &img, ivec2 p, vec4 v) {
  if (p != img.expect) {
    std::fprintf(stderr, "glsl_ref: imageStore at (%d,%d), dispatched pixel (%d,%d)\n", p.x, p.y,
                 img.expect.x, img.expect.y);
    std::exit(3);
  }
  if (p.x < 0 || p.y < 0 || p.x >= img.width || p.y >= img.height) return; /* GL drops it */
  float *t = img.texels + (static_cast<size_t>(p.y) * img.width + p.x) * 4;
  t[0] = v.x, t[1] = v.y, t[2] = v.z, t[3] = v.w;
  img.stores++;
}

/* ---- compute-shader built-in variables (GLSL 4.50 §7.1) ------------------- */
inline uvec3 gl_WorkGroupID(0), gl_LocalInvocationID(0);

/* ---- implicit int -> float conversions (GLSL 4.50 §4.1.10) that C++ template
 *      deduction does not perform ------------------------------------------- */
inline float radians(int degrees) { return glm::radians(static_cast<float>(degrees)); }
inline vec3 operator/(const vec3 &v, int s) { return v / static_cast<float>(s); }

/* ---- built-ins DESIGN.md §2 defines otherwise than GLM 0.9.8.5 -------------
 * GLSL_REF_GLM_MIX / GLSL_REF_GLM_MINMAX hand one family back to GLM
 * (tools/ref_builtin_diff.py measures what each choice changes). */
#ifdef GLSL_REF_PURE_GLM
#define GLSL_REF_GLM_MIX
#define GLSL_REF_GLM_MINMAX
#endif
#ifndef GLSL_REF_GLM_MIX
#define GLSL_REF_OVERRIDES_MIX "mix", /* list heads: they keep their commas */
/* §2 "reflect / mix": mix(x,y,a) = x·(1−a) + y·a   (GLM: x + a·(y−x)) */
inline float mix(float x, float y, float a) { return x * (1.0f - a) + y * a; }
#else
#define GLSL_REF_OVERRIDES_MIX
#endif
#ifndef GLSL_REF_GLM_MINMAX
#define GLSL_REF_OVERRIDES_MINMAX "min", "max", "clamp",
/* §2 "min / max": min(x,y) = y<x ? y : x   (GLSL spec; GLM: x<y ? x : y) */
inline float min(float x, float y) { return y < x ? y : x; }
/* §2 "min / max": max(x,y) = x<y ? y : x   (GLSL spec; GLM: x>y ? x : y) */
inline float max(float x, float y) { return x < y ? y : x; }
/* §2 "min / max": the same max per component, vector against scalar */
inline vec3 max(const vec3 &v, float s) { return vec3(max(v.x, s), max(v.y, s), max(v.z, s)); }
/* §2 "min / max": clamp = min(max()) */
inline float clamp(float x, float lo, float hi) { return min(max(x, lo), hi); }
#else
#define GLSL_REF_OVERRIDES_MINMAX
#endif
/* §2 "int()": truncation; a value outside the int range saturates and NaN gives 0
 * (GLSL: undefined value; the C++ cast: undefined behaviour, whichever build) */
inline int glsl_int(float x) {
  return !(x == x) ? 0 : x >= 2147483648.0f ? 2147483647 : x < -2147483648.0f ? -2147483647 - 1 : static_cast<int>(x);
}
template <typename T> inline int glsl_int(T x) { return static_cast<int>(x); } /* int(uint), int(bool), ... */
#define GLSL_REF_OVERRIDES GLSL_REF_OVERRIDES_MIX GLSL_REF_OVERRIDES_MINMAX "int",

}  // namespace glslref
#endif /* GLSL_PRELUDE_HPP */
#else  /* GLSL_PRELUDE_END */
#undef uniform
#undef layout
#undef in
#endif
