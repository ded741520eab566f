// rm_frame_math.hip — the per-frame float math of the host (rm_frame_math.hpp).
//
// Built with librm's flags: -ffp-contract=off is what keeps every operation
// below one IEEE operation in source order, which the bit-identity with the
// device rests on.  No context, no HIP runtime call.
#include "rm_frame_math.hpp"

#include <cmath>
#include <cstring>

#include "rm_scene.hpp"

namespace rm {

// Step 0 of every primary ray (rm_scene.hpp PrepSlot), on the host: what the
// render kernels' scene_lazy would compute at the camera, with the same IEEE operations in the same order (x86-64 SSE floats,
// -ffp-contract=off), so d0 is bit-identical to the device's scene_exact at the
// camera (sqrt_core / sqrt_cr_nonneg / div_capbb are the IEEE sqrt and divide on
// the values reached here, rm_fastmath.hpp).  The bounds (slack, LB_k, b1, b2)
// only need to be valid: their 2^-12 / 2^-18 margins were made for v_sqrt's
// 1.5 ulp, and the IEEE sqrt is within them.
void prep_host(const float cam[3], float blend, float omblend, float out[16]) {
  using namespace rmd;
  const float px = cam[0], py = cam[1], pz = cam[2];
  const float ax = px - 15.0f, ay = py, az = pz + 10.0f, bx = px + 25.0f, cx = px + 5.0f;
  const float ay2 = ay * ay, az2 = az * az, cx2 = cx * cx;
  const float x0 = (ax * ax + ay2) + az2, x1 = (bx * bx + ay2) + az2, xs = (cx2 + ay2) + az2;
  const float d0s = std::sqrt(x0) - 3.0f, d1 = std::sqrt(x1) - 3.0f;
  const float qx = std::fabs(cx) - 3.0f, qy = std::fabs(ay) - 2.5f, qz = std::fabs(az) - 2.5f;
  const float mx = std::fmax(qx, 0.0f), my = std::fmax(qy, 0.0f), mz = std::fmax(qz, 0.0f);
  const float box = std::fmin(std::fmax(qx, std::fmax(qy, qz)), 0.0f) +
                    std::sqrt((mx * mx + my * my) + mz * mz);
  const float d4 = box * omblend + (std::sqrt(xs) - 3.0f) * blend;
  const float tz = pz - 10.0f;
  const float l = std::sqrt(cx2 + ay2) - 2.5f;
  const float d5 = std::sqrt(l * l + tz * tz) - 0.5f;
  const float cpx = cx - CAP_AX, cpy = (py + 2.0f) - CAP_AY, cpz = (pz + 30.0f) - CAP_AZ;
  const float hn = (cpx * CAP_BAX + cpy * CAP_BAY) + cpz * CAP_BAZ;
  const float h = std::fmin(std::fmax(hn / CAP_BB_HOST, 0.0f), 1.0f);
  const float ex = cpx - CAP_BAX * h, ey = cpy - CAP_BAY * h, ez = cpz - CAP_BAZ * h;
  const float d6 = std::sqrt((ex * ex + ey * ey) + ez * ez) - 1.0f;
  const float d7 = py + 5.5f;
  const float ds[6] = {d0s, d1, d4, d5, d6, d7};
  float d = ds[0];
  bool nan = false;
  for (float v : ds) {
    nan = nan || std::isnan(v);
    d = v < d ? v : d;
  }
  const float HI = 1.0f + 0x1p-12f;
  const float sl = 0x1p-14f * (((std::fabs(px) + std::fabs(py)) + std::fabs(pz)) * HI + 64.0f) * HI;
  const float sx = px - SH_CX, sy = py - SH_CY, sz = pz - SH_CZ;
  const float rc = std::fma(std::sqrt((sx * sx + sy * sy) + sz * sz), HI, 0x1p-18f);
  const float kx = px - CAP_MX, ky = py - CAP_MY, kz = pz - CAP_MZ;
  const float x[5] = {x0, x1, xs, (cx2 + ay2) + tz * tz, (kx * kx + ky * ky) + kz * kz};
  const float R[5] = {3.0f, 3.0f, R_BLEND_LO, R_TORUS, R_CAPSULE};
  std::memset(out, 0, 16 * sizeof(float));
  out[PREP_VALID] = (!nan && d > 0.0f && d <= 400.0f) ? 1.0f : 0.0f;
  out[PREP_D0] = d;
  out[PREP_SLACK] = sl;
  out[PREP_B1] = (rc + SH_RALL + sl + 0.0f) * HI;
  out[PREP_B2] = ((py + 5.5f) - sl - 0.0f * HI) - 0x1p-19f * (std::fabs(py) + 5.5f + 0.0f + sl);
  out[PREP_B3] = ((SH_YTOP - py) + sl + 0.0f * HI) + 0x1p-19f * (std::fabs(py) + SH_YTOP + 0.0f + sl);
  const float pl = (py + 5.5f) + sl;
  for (int k = 0; k < 5; ++k) {
    // the gaps of scene_lazy's re-test at the camera with U = d0, in its float
    // operations: g = (lb - d0) - slack, plane gap lb - pl
    const float lb = std::fma(std::sqrt(x[k]), CULL_REL_LO, -(CULL_ABS + R[k]));
    const float g = lb - d - sl;
    out[PREP_G + k] = g > 0.0f ? g : -INFINITY;
    out[PREP_H + k] = g > 0.0f ? lb - pl : -INFINITY;
  }
}

// Step 0 of a table's primary rays (rm_internal.hpp TablePrep), on the host:
// what the table kernel's first march step computes at the camera, with the
// device's float operations (rm_table.hip prim_dist: IEEE sqrt and divide,
// GLSL min/max, opU in table order; x86-64 SSE floats, -ffp-contract=off).
// The slot bounds only need to be valid: the 2^-12 margin made for v_sqrt
// covers the IEEE sqrt.  Invalid (TP_VALID = 0) when d0 is not in (0, 400].
namespace {
struct H3 {
  float x, y, z;
};
float hgmin(float x, float y) { return y < x ? y : x; }
float hgmax(float x, float y) { return x < y ? y : x; }
float hdot(H3 a, H3 b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
float hlen(H3 a) { return std::sqrt(hdot(a, a)); }
float hprim(const float* P, H3 p, float blend, float omblend) {
  int type, swz;
  std::memcpy(&type, &P[rm::TW_TYPE], 4);
  std::memcpy(&swz, &P[rm::TW_SWIZZLE], 4);
  H3 q{p.x - P[rm::TW_CENTER], p.y - P[rm::TW_CENTER + 1], p.z - P[rm::TW_CENTER + 2]};
  if (swz == RM_SWIZZLE_XZY) q = H3{q.x, q.z, q.y};
  const float* a = P + rm::TW_P;
  switch (type) {
    case RM_PRIM_SPHERE:
      return hlen(q) - a[0];
    case RM_PRIM_BOX:
    case RM_PRIM_BLEND: {
      const H3 d{std::fabs(q.x) - a[0], std::fabs(q.y) - a[1], std::fabs(q.z) - a[2]};
      const H3 m{hgmax(d.x, 0.0f), hgmax(d.y, 0.0f), hgmax(d.z, 0.0f)};
      const float box = hgmin(hgmax(d.x, hgmax(d.y, d.z)), 0.0f) + hlen(m);
      if (type == RM_PRIM_BOX) return box;
      return box * omblend + (hlen(q) - a[3]) * blend;
    }
    case RM_PRIM_TORUS: {
      const float l = std::sqrt(q.x * q.x + q.z * q.z) - a[0];
      return std::sqrt(l * l + q.y * q.y) - a[1];
    }
    case RM_PRIM_CAPSULE: {
      const H3 pa{q.x - a[0], q.y - a[1], q.z - a[2]}, ba{a[3], a[4], a[5]};
      const float h = hgmin(hgmax(hdot(pa, ba) / a[6], 0.0f), 1.0f);
      return hlen(H3{pa.x - ba.x * h, pa.y - ba.y * h, pa.z - ba.z * h}) - a[7];
    }
    default:
      return hdot(q, H3{a[0], a[1], a[2]}) + a[3];
  }
}
}  // namespace

void table_prep_host(const uint32_t* words, int32_t n, const float cam[3], float blend, float omblend,
                     float out[16]) {
  const float* t = reinterpret_cast<const float*>(words);
  const float* ex = t + (size_t)n * rm::TABLE_WORDS;
  const H3 p{cam[0], cam[1], cam[2]};
  std::memset(out, 0, 16 * sizeof(float));
  float d = INFINITY, U = INFINITY;
  for (int32_t k = 0; k < n; ++k) {
    const float* P = t + (size_t)k * rm::TABLE_WORDS;
    const float dk = hprim(P, p, blend, omblend);
    d = d < dk ? d : dk;  // opU(d, dk) = (d < dk) ? d : dk
    int type;
    std::memcpy(&type, &P[rm::TW_TYPE], 4);
    if (type == RM_PRIM_PLANE) U = hgmin(U, dk);
  }
  out[rm::TP_VALID] = (d > 0.0f && d <= 400.0f) ? 1.0f : 0.0f;
  out[rm::TP_D0] = d;
  // TLazy::dist's step-0 re-test at p = camera (dprev = +inf: U = the planes)
  const float sig2 = 2.0f * ex[rm::EX_SIGMA];
  const float a1 = (std::fabs(p.x) + std::fabs(p.y)) + std::fabs(p.z);
  const float sl0 = (a1 + ex[rm::EX_S]) * (1.0f + 0x1p-16f);
  const float sl = sig2 * (a1 + sl0) * (1.0f + 0x1p-10f);
  const int ns = (int)ex[rm::EX_NSLOTS];
  for (int j = 0; j < ns && j < rm::EX_MAX_SLOTS; ++j) {
    const float* B = t + (size_t)(int)ex[rm::EX_SLOTS + j] * rm::TABLE_WORDS + rm::TW_BALL;
    const float bx = p.x - B[0], by = p.y - B[1], bz = p.z - B[2];
    const float lb = std::fma(std::sqrt((bx * bx + by * by) + bz * bz), 1.0f - 0x1p-12f, -B[3]);
    out[rm::TP_G + j] = lb - U - sl;
  }
}

// Frame::unit_rd: every primary ray of the frame has |rd| within 2^-20 of 1.
// castRay (glsl:68-74) normalises v = uvx X + uvy Y + RN(D persp) (vec4, then
// .xyz): with the w components of X, Y, D zero, v.w = +-0 and, when |v|^2 stays
// in the normal range, every operation of normalize() has relative error <= u =
// 2^-24, so |rd| is within ~4.5u of 1.  The host bounds |v|^2 over the uv table's
// range [uv_lo, uv_hi]^2 exactly (a quadratic in (uvx, uvy): corners, edges and
// the interior critical point, in double), and requires min |v|^2 >= 2^-38 M^2
// (the float error of v, <= 3 sqrt(3) u M with M >= |v| the triangle bound,
// then moves |v| by < 16 %), min |v|^2 >= 2^-80 and M^2 <= 2^100.
//
// What relies on a passing check besides the unit march (rm_kernels.hip march<UNIT>):
// cast_ray's lean form (rm_scene.hpp cast_ray<LEAN>) drops the w lane of v on these
// frames, which uses two of the conditions below: the three w components are exactly
// 0, and X, Y, C and the uv range are finite (so v.w = (uvx 0 + uvy 0) + 0 persp is
// +-0 and not NaN, and v.z^2 + v.w^2 is v.z^2 bit for bit).  Its root takes sqrt_vote
// on every frame and depends on nothing here for its value; min |v|^2 >= 2^-80 with
// the float sum within 16 % only says that the vote passes (|v|^2 > 2^-96) on these
// frames, i.e. that they take sqrt_core alone.  Relaxing the w or the finiteness
// condition breaks cast_ray<true>; relaxing the 2^-80 floor only sends waves through
// the guarded root.
bool unit_rd_check(const rm_camera& k, float persp, const float uv_lo[2], const float uv_hi[2]) {
  if (k.xAxis[3] != 0.0f || k.yAxis[3] != 0.0f || k.dir[3] != 0.0f) return false;
  double X[3], Y[3], C[3];
  for (int i = 0; i < 3; ++i) {
    X[i] = k.xAxis[i];
    Y[i] = k.yAxis[i];
    C[i] = (double)(k.dir[i] * persp);  // the kernel's float product
    if (!std::isfinite(X[i]) || !std::isfinite(Y[i]) || !std::isfinite(C[i])) return false;
  }
  auto dotd = [](const double* a, const double* b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
  const double xx = dotd(X, X), yy = dotd(Y, Y), xy = dotd(X, Y), xc = dotd(X, C), yc = dotd(Y, C),
               cc = dotd(C, C);
  auto q = [&](double a, double b) { return a * a * xx + b * b * yy + 2 * a * b * xy + 2 * a * xc + 2 * b * yc + cc; };
  const double a0 = uv_lo[0], a1 = uv_hi[0], b0 = uv_lo[1], b1 = uv_hi[1];
  if (!(a0 <= a1) || !(b0 <= b1)) return false;
  auto clampd = [](double v, double lo, double hi) { return v < lo ? lo : (v > hi ? hi : v); };
  double m = std::fmin(std::fmin(q(a0, b0), q(a0, b1)), std::fmin(q(a1, b0), q(a1, b1)));
  for (double a : {a0, a1})
    if (yy > 0) m = std::fmin(m, q(a, clampd(-(a * xy + yc) / yy, b0, b1)));
  for (double b : {b0, b1})
    if (xx > 0) m = std::fmin(m, q(clampd(-(b * xy + xc) / xx, a0, a1), b));
  const double det = xx * yy - xy * xy;
  if (det > 0) {
    const double a = (-xc * yy + yc * xy) / det, b = (-yc * xx + xc * xy) / det;
    if (a >= a0 && a <= a1 && b >= b0 && b <= b1) m = std::fmin(m, q(a, b));
  }
  const double M = std::fmax(std::fabs(a0), std::fabs(a1)) * std::sqrt(xx) +
                   std::fmax(std::fabs(b0), std::fabs(b1)) * std::sqrt(yy) + std::sqrt(cc);
  // (m carries the double rounding of the quadratic, relative ~1e-15 of M^2:
  // the 2^-38 M^2 floor is far above it)
  return m >= std::ldexp(M * M, -38) && m >= std::ldexp(1.0, -80) && M * M <= std::ldexp(1.0, 100);
}

UvTable uv_table(int W, int H) {
  // uv of the pixel columns and rows with the shader's float operations
  // (glsl:301-305 and the cumulative sub-sample offsets of :309-332)
  const float ox[4] = {0.25f, 0.75f, 0.25f, 0.75f}, oy[4] = {0.25f, 0.25f, 0.75f, 0.75f};
  UvTable t;
  std::vector<float>& uv = t.uv;
  uv.resize((size_t)5 * (W + H));
  for (int p = 0; p < W + H; ++p) {
    const bool col = p < W;
    const int i = col ? p : p - W, n = col ? W : H;
    float v = (float)(i * 2 - n) / (float)n;
    uv[(size_t)p * 5] = v;
    for (int k = 0; k < 4; ++k) {
      v += (col ? ox[k] : oy[k]) / (float)n;
      uv[(size_t)p * 5 + 1 + k] = v;
    }
  }
  for (int a = 0; a < 2; ++a) {
    t.lo[a] = INFINITY;
    t.hi[a] = -INFINITY;
  }
  for (int p = 0; p < W + H; ++p)
    for (int k = 0; k < 5; ++k) {
      const int a = p < W ? 0 : 1;
      t.lo[a] = std::fmin(t.lo[a], uv[(size_t)p * 5 + k]);
      t.hi[a] = std::fmax(t.hi[a], uv[(size_t)p * 5 + k]);
    }
  // lane_uv (rm_scene.hpp) may form the same values arithmetically when, for every
  // column and row, RN(1/n)-times-a plus one fma remainder correction equals the
  // IEEE (2p - n) / n; the offsets' adds are the table's own operations
  t.exact = true;
  for (int p = 0; p < W + H && t.exact; ++p) {
    const bool col = p < W;
    const int i = col ? p : p - W, n = col ? W : H;
    const float a = (float)(i * 2 - n), nf = (float)n, r = 1.0f / nf;
    const float q0 = a * r;
    const float q = std::fma(std::fma(-q0, nf, a), r, q0);
    t.exact = q == uv[(size_t)p * 5] && std::signbit(q) == std::signbit(uv[(size_t)p * 5]);
  }
  return t;
}

const char* pattern_invalid(const rm_sample_pattern* p) {
  if (p->struct_size != sizeof(rm_sample_pattern)) return "rm_sample_pattern.struct_size is not sizeof(rm_sample_pattern)";
  if (p->flags & ~RM_PATTERN_CUMULATIVE) return "rm_sample_pattern.flags has an unknown bit";
  if (p->n < 1 || p->n > RM_MAX_SAMPLES) return "rm_sample_pattern.n must be in 1..RM_MAX_SAMPLES";
  for (int s = 0; s < p->n; ++s)
    // (written so that a NaN fails)
    if (!(std::fabs(p->dx[s]) <= 16.0f) || !(std::fabs(p->dy[s]) <= 16.0f))
      return "every offset below n must be finite and within 16 pixels";
  return nullptr;
}

void pattern_uv(const rm_sample_pattern& p, int W, int H, float* uvx, float* uvy, float lo[2], float hi[2]) {
  const int n = p.n;
  const bool cumulative = (p.flags & RM_PATTERN_CUMULATIVE) != 0;
  for (int a = 0; a < 2; ++a) {
    const int dim = a ? H : W;
    const float* d = a ? p.dy : p.dx;
    float* out = a ? uvy : uvx;
    const float dimf = (float)dim;
    float off[RM_MAX_SAMPLES];
    for (int s = 0; s < n; ++s) off[s] = (2.0f * d[s]) / dimf;
    lo[a] = INFINITY;
    hi[a] = -INFINITY;
    for (int i = 0; i < dim; ++i) {
      const float v0 = (float)(2 * i - dim) / dimf;
      float v = v0;
      for (int s = 0; s < n; ++s) {
        v = (cumulative ? v : v0) + off[s];
        if (out) out[(size_t)i * n + s] = v;
        lo[a] = std::fmin(lo[a], v);
        hi[a] = std::fmax(hi[a], v);
      }
    }
  }
}

}  // namespace rm

extern "C" {

int rm_sample_pattern_init(rm_sample_pattern* p, int32_t preset) {
  if (!p || preset < RM_PATTERN_REFERENCE || preset > RM_PATTERN_GRID4) return RM_ERR_INVALID;
  std::memset(p, 0, sizeof *p);
  p->struct_size = (uint32_t)sizeof *p;
  auto grid = [&](const float* v, int m) {  // {v}^2, x fastest
    p->n = m * m;
    for (int j = 0; j < m; ++j)
      for (int i = 0; i < m; ++i) {
        p->dx[j * m + i] = v[i];
        p->dy[j * m + i] = v[j];
      }
  };
  switch (preset) {
    case RM_PATTERN_REFERENCE: {
      const float dx[4] = {0.125f, 0.375f, 0.125f, 0.375f}, dy[4] = {0.125f, 0.125f, 0.375f, 0.375f};
      p->flags = RM_PATTERN_CUMULATIVE;
      p->n = 4;
      std::memcpy(p->dx, dx, sizeof dx);
      std::memcpy(p->dy, dy, sizeof dy);
      break;
    }
    case RM_PATTERN_GRID2: {
      const float v[2] = {-0.25f, 0.25f};
      grid(v, 2);
      break;
    }
    case RM_PATTERN_RGSS: {
      const float dx[4] = {0.125f, -0.375f, 0.375f, -0.125f}, dy[4] = {0.375f, 0.125f, -0.125f, -0.375f};
      p->n = 4;
      std::memcpy(p->dx, dx, sizeof dx);
      std::memcpy(p->dy, dy, sizeof dy);
      break;
    }
    case RM_PATTERN_GRID3: {
      const float v[3] = {-0.34375f, 0.0f, 0.34375f};
      grid(v, 3);
      break;
    }
    default: {
      const float v[4] = {-0.375f, -0.125f, 0.125f, 0.375f};
      grid(v, 4);
      break;
    }
  }
  return RM_OK;
}

int rm_pattern_uv_table(const rm_sample_pattern* p, int32_t width, int32_t height, float* uvx, float* uvy) {
  if (!p || rm::pattern_invalid(p)) return RM_ERR_INVALID;
  if (width < 1 || width > 65536 || height < 1 || height > 65536) return RM_ERR_INVALID;
  float lo[2], hi[2];
  rm::pattern_uv(*p, width, height, uvx, uvy, lo, hi);
  return RM_OK;
}

// (include/rm_api.h RM_HAS_ACCUMULATION) The radical inverse in double, every operation
// one IEEE double operation in the header's order: the product and the sum are separate.
static double radical_inverse(int64_t i, int b) {
  double f = 1.0 / b, r = 0.0;
  while (i > 0) {
    const double term = (double)(i % b) * f;
    r = r + term;
    i = i / b;
    f = f / (double)b;
  }
  return r;
}

int rm_sample_pattern_halton(rm_sample_pattern* p, int64_t first, int32_t n) {
  if (!p || n < 1 || n > RM_MAX_SAMPLES || first < 0 || first > ((int64_t)1 << 40)) return RM_ERR_INVALID;
  std::memset(p, 0, sizeof *p);
  p->struct_size = (uint32_t)sizeof *p;
  p->n = n;
  for (int s = 0; s < n; ++s) {
    const int64_t i = first + s + 1;
    p->dx[s] = (float)(radical_inverse(i, 2) - 0.5);
    p->dy[s] = (float)(radical_inverse(i, 3) - 0.5);
  }
  return RM_OK;
}

}  // extern "C"
