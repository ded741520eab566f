/*
 * glsl_ref_main.cpp — TEST INFRASTRUCTURE ONLY.
 *
 * Runs the reference's own compute shader on the CPU: its text, rewritten by
 * oracle/glsl_rewrite.py (token rules only) and compiled as C++20 against the
 * reference's vendored GLM through oracle/glsl_prelude.hpp, is included below
 * from oracle/_ref/ (-DGLSL_REF_SHADER=<path>; never committed).  This driver
 * plays the part of the GL host: it sets the uniforms from an rm_uniforms
 * blob and dispatches main() once per pixel.
 *
 *   glsl_ref frame W H uniforms.bin [workgroups]  > frame.f32
 *       uniforms.bin: the 168 bytes of rm_uniforms (shadow_mode must be 0: the
 *       hard shadow is librm's extension, the shader has none).  Output: raw
 *       RGBA32F, [H][W][4], row 0 = pixel row 0.  workgroups (default 8) is the
 *       shader's tile edge: pixel = gl_WorkGroupID * workgroups +
 *       gl_LocalInvocationID, as glDispatchCompute would number them.
 *   glsl_ref probe uniforms.bin  < records > results
 *       records of {int32 function; float args[9]} in, one {float/int32 v[8]}
 *       per record out (see probe_one).
 *   glsl_ref info
 *       one JSON line: GLM version, the prelude's overrides.
 *
 * Built with -ffp-contract=off: every float operation is one IEEE operation
 * in the shader's source order.
 */
#include <cstring>
#include <vector>

#include "../include/rm_api.h"

#include "glsl_prelude.hpp" /* last: its qualifier macros are live until the shader text ends */

#ifndef GLSL_REF_SHADER
#error "build with -DGLSL_REF_SHADER='\"oracle/_ref/<rewritten shader>\"' (make oracle/_ref/glsl_ref)"
#endif

/* The shader initialises namespace-scope constants from the launch-geometry
 * uniform, which GLSL evaluates per invocation and C++ once, before main().  So
 * the uniform must hold its value by then: glibc hands argv to constructors,
 * and one that runs before every C++ initialiser picks the argument up. */
static unsigned g_workgroups_arg = 8;
__attribute__((constructor(101))) static void early_args(int argc, char **argv, char **) {
  if (argc > 5 && argv && !std::strcmp(argv[1], "frame")) {
    long v = std::strtol(argv[5], nullptr, 10);
    if (v > 0 && v <= 65536) g_workgroups_arg = static_cast<unsigned>(v);
  }
}

namespace glslref {

extern uint workgroups; /* the shader defines it; set here, ahead of its initialisers */
[[maybe_unused]] static const bool workgroups_set = (workgroups = g_workgroups_arg, true);

#include GLSL_REF_SHADER
#define GLSL_PRELUDE_END
#include "glsl_prelude.hpp"

static int fail(const char *what) {
  std::fprintf(stderr, "glsl_ref: %s\n", what);
  return 2;
}

static bool read_all(FILE *f, std::vector<unsigned char> &out) {
  if (!f) return false;
  unsigned char buf[4096];
  size_t n;
  while ((n = std::fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  return !std::ferror(f);
}

static bool read_file(const char *path, std::vector<unsigned char> &out) {
  FILE *f = std::fopen(path, "rb");
  bool ok = read_all(f, out);
  if (f) std::fclose(f);
  return ok;
}

static bool write_stdout(const void *p, size_t n) {
  return std::fwrite(p, 1, n, stdout) == n && std::fflush(stdout) == 0;
}

static vec3 v3(const float *p) { return vec3(p[0], p[1], p[2]); }
static vec4 v4(const float *p) { return vec4(p[0], p[1], p[2], p[3]); }

/* What main.cpp's setBool/setInt/setFloat/setVec* calls do, from the blob. */
static int set_uniforms(const char *path) {
  static_assert(sizeof(rm_uniforms) == 168, "rm_uniforms layout");
  std::vector<unsigned char> b;
  if (!read_file(path, b)) return fail("cannot read the uniforms file");
  if (b.size() != sizeof(rm_uniforms)) return fail("uniforms file is not sizeof(rm_uniforms) = 168 bytes");
  rm_uniforms u;
  std::memcpy(&u, b.data(), sizeof u);
  if (u.shadow_mode != RM_SHADOW_SOFT)
    return fail("shadow_mode != 0: the hard shadow is librm's extension, the shader has none");
  camera.pos = v4(u.camera.pos);
  camera.dir = v4(u.camera.dir);
  camera.yAxis = v4(u.camera.yAxis);
  camera.xAxis = v4(u.camera.xAxis);
  light.position = v3(u.light.position);
  light.ambient = v3(u.light.ambient);
  light.diffuse = v3(u.light.diffuse);
  light.specular = v3(u.light.specular);
  light.constant = u.light.constant;
  light.linear = u.light.linear;
  light.quadratic = u.light.quadratic;
  iTime = u.iTime;
  bounceVar = u.bounceVar;
  AA = u.AA != 0;
  drand48 = u.drand48;
  mouse = v3(u.mouse);
  iMouse = vec2(u.iMouse[0], u.iMouse[1]);
  return 0;
}

static int frame(int argc, char **argv) {
  if (argc < 5 || argc > 6) return fail("usage: glsl_ref frame W H uniforms.bin [workgroups]");
  int W = std::atoi(argv[2]), H = std::atoi(argv[3]);
  if (W <= 0 || H <= 0 || W > 65536 || H > 65536) return fail("bad W or H");
  if (argc > 5 && std::strtol(argv[5], nullptr, 10) != static_cast<long>(workgroups))
    return fail("bad workgroups (1..65536)");
  if (int rc = set_uniforms(argv[4])) return rc;
  std::vector<float> texels(static_cast<size_t>(W) * H * 4, 0.0f);
  img_output.width = W;
  img_output.height = H;
  img_output.texels = texels.data();
  const unsigned wg = workgroups;
  /* glDispatchCompute(ceil(W / wg), ceil(H / wg), 1), each group wg x wg invocations */
  for (unsigned gy = 0; gy * wg < static_cast<unsigned>(H); gy++)
    for (unsigned gx = 0; gx * wg < static_cast<unsigned>(W); gx++)
      for (unsigned ly = 0; ly < wg; ly++)
        for (unsigned lx = 0; lx < wg; lx++) {
          int px = static_cast<int>(gx * wg + lx), py = static_cast<int>(gy * wg + ly);
          if (px >= W || py >= H) continue; /* imageStore would drop it */
          gl_WorkGroupID = uvec3(gx, gy, 0);
          gl_LocalInvocationID = uvec3(lx, ly, 0);
          img_output.expect = ivec2(px, py);
          main();
        }
  if (img_output.stores != static_cast<long>(W) * H) return fail("the shader did not store every pixel");
  if (!write_stdout(texels.data(), texels.size() * sizeof(float))) return fail("cannot write the frame");
  return 0;
}

/* ---- probe: single shader functions ---------------------------------------- */
enum { P_SDF = 0, P_RAYMARCH, P_REFLECTED, P_NORMAL, P_SOFTSHADOW, P_POINTLIGHT, P_CASTRAY, P_RENDER, P_COUNT };
struct probe_rec {
  int32_t fn;
  float a[9];
};
union probe_val {
  float f;
  int32_t i;
};
struct probe_out {
  probe_val v[8];
};

static void put(probe_out &o, const RayHit &h) { /* hitpoint, colour, id (int32), material */
  o.v[0].f = h.hitpoint, o.v[1].f = h.color.x, o.v[2].f = h.color.y, o.v[3].f = h.color.z;
  o.v[4].i = h.id, o.v[5].f = h.material;
}
static void put(probe_out &o, const vec3 &v, int at = 0) { o.v[at].f = v.x, o.v[at + 1].f = v.y, o.v[at + 2].f = v.z; }

static bool probe_one(const probe_rec &r, probe_out &o) {
  const float *a = r.a;
  vec3 p(a[0], a[1], a[2]), q(a[3], a[4], a[5]), s(a[6], a[7], a[8]);
  std::memset(&o, 0, sizeof o);
  switch (r.fn) {
    case P_SDF: put(o, sdf(p)); break;                      /* pos */
    case P_RAYMARCH: put(o, RayMarch(p, q)); break;         /* origin, dir */
    case P_REFLECTED: put(o, reflectedRay(p, q)); break;    /* origin, dir */
    case P_NORMAL: put(o, GetNormal(p)); break;             /* pos */
    case P_SOFTSHADOW: o.v[0].f = softshadow(p, q, a[6]); break; /* ro, rd, k */
    case P_POINTLIGHT: put(o, getPointLight(p, q, s)); break;    /* colour, normal, pos */
    case P_CASTRAY: {                                       /* uv */
      Ray ray = castRay(vec2(a[0], a[1]));
      put(o, ray.origin, 0), put(o, ray.dir, 3);
      break;
    }
    case P_RENDER: put(o, render(p, q)); break;             /* origin, dir */
    default: return false;
  }
  return true;
}

static int probe(int argc, char **argv) {
  if (argc != 3) return fail("usage: glsl_ref probe uniforms.bin < records > results");
  if (int rc = set_uniforms(argv[2])) return rc;
  std::vector<unsigned char> b;
  if (!read_all(stdin, b)) return fail("cannot read the records");
  if (b.size() % sizeof(probe_rec)) return fail("records are not a whole number of 40-byte records");
  size_t n = b.size() / sizeof(probe_rec);
  std::vector<probe_out> out(n);
  for (size_t i = 0; i < n; i++) {
    probe_rec r;
    std::memcpy(&r, b.data() + i * sizeof r, sizeof r);
    if (!probe_one(r, out[i])) return fail("unknown probe function");
  }
  if (!write_stdout(out.data(), n * sizeof(probe_out))) return fail("cannot write the results");
  return 0;
}

static int info() {
  const char *ov[] = {GLSL_REF_OVERRIDES nullptr};
  std::printf("{\"glm_version\": \"%d.%d.%d.%d\", \"overrides\": [", GLM_VERSION_MAJOR, GLM_VERSION_MINOR,
              GLM_VERSION_PATCH, GLM_VERSION_REVISION);
  for (int i = 0; ov[i]; i++) std::printf("%s\"%s\"", i ? ", " : "", ov[i]);
  std::printf("]}\n");
  return 0;
}

static int driver(int argc, char **argv) {
  if (argc >= 2 && !std::strcmp(argv[1], "frame")) return frame(argc, argv);
  if (argc >= 2 && !std::strcmp(argv[1], "probe")) return probe(argc, argv);
  if (argc == 2 && !std::strcmp(argv[1], "info")) return info();
  return fail("usage: glsl_ref frame|probe|info ... (see glsl_ref_main.cpp)");
}

}  // namespace glslref

int main(int argc, char **argv) { return glslref::driver(argc, argv); }
