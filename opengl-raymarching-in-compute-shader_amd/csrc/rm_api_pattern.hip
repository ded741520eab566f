// rm_api_pattern.hip — librm's C-ABI for sample-pattern frames (include/rm_api.h
// RM_HAS_SAMPLE_PATTERN): rm_dispatch_pattern, and the pattern's
// device table, which the pattern refinements of the adaptive calls share
// (rm_api_adaptive.hip).  The pattern's presets and its uv table are pure host
// math (rm_frame_math.hip).
//
// One such dispatch is, on the context's stream: the upload of the pattern's uv
// table when the pattern differs from the last call's, and one kernel
// (rm_pattern.hip for the built-in scene, rm_table_pattern.hip for a table) that
// renders every pixel's n samples and stores their mean (for n = 1 a kernel on the
// pixel kernels' tile, one lane per pixel).
//
// This version: one-device, whole-frame contexts.  Out of scope, and refused:
// sharded, communicator and multi-device contexts, counting contexts, G-buffer
// contexts, batches and graph replay; hiprtc-specialised pattern kernels (the
// generic table code renders).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rm_ctx.hpp"
#include "rm_frame_math.hpp"

using namespace rm;

namespace {

// Floats of the largest table the context can need: RM_MAX_SAMPLES per column and row.
size_t table_cap(const rm_ctx* c) {
  return (size_t)RM_MAX_SAMPLES * ((size_t)c->cfg.width + (size_t)c->cfg.height);
}

// The fields of a valid pattern that the rule reads.
bool same_pattern(const rm_sample_pattern& a, const rm_sample_pattern& b) {
  return a.n == b.n && a.flags == b.flags && std::memcmp(a.dx, b.dx, sizeof(float) * (size_t)a.n) == 0 &&
         std::memcmp(a.dy, b.dy, sizeof(float) * (size_t)a.n) == 0;
}

}  // namespace

// The device table of pattern p: the context's when p is the last call's (of
// rm_dispatch_pattern or of a pattern refinement, rm_api_adaptive.hip: they share
// the table, its cache and pat_lo / pat_hi), else formed on the host (into pinned
// memory, once the previous upload has left it) and uploaded on the context's
// stream, behind whatever still reads the old one.
int rm::ensure_table(rm_ctx* c, const rm_sample_pattern& p, const char* call) {
  if (c->pat.n != 0 && same_pattern(c->pat, p)) return RM_OK;
  const size_t bytes = table_cap(c) * sizeof(float);
  const std::string what = std::string(call) + ": uv table";
  int rc = ensure(c, c->pat_uv, bytes, what.c_str());
  if (rc != RM_OK) return rc;
  if (!c->pat_host) {
    if (hipHostMalloc(reinterpret_cast<void**>(&c->pat_host), bytes, hipHostMallocDefault) != hipSuccess) {
      c->pat_host = nullptr;
      (void)hipGetLastError();
      return fail(c, RM_ERR_NOMEM, std::string(call) + ": host uv table of " + std::to_string(bytes) + " bytes");
    }
  }
  if (!c->pat_ev) RM_HIP(c, hipEventCreateWithFlags(&c->pat_ev, hipEventDisableTiming));
  if (c->pat_ev_pending) {
    RM_HIP(c, hipEventSynchronize(c->pat_ev));
    c->pat_ev_pending = false;
  }
  c->pat.n = 0;  // no table until the new one is queued
  const int W = c->cfg.width, H = c->cfg.height;
  float* uvx = c->pat_host;
  float* uvy = uvx + (size_t)W * (size_t)p.n;
  pattern_uv(p, W, H, uvx, uvy, c->pat_lo, c->pat_hi);
  const size_t used = ((size_t)W + (size_t)H) * (size_t)p.n * sizeof(float);
  RM_HIP(c, hipMemcpyAsync(c->pat_uv.p, c->pat_host, used, hipMemcpyHostToDevice, c->stream));
  RM_HIP(c, hipEventRecord(c->pat_ev, c->stream));
  c->pat_ev_pending = true;
  c->pat = p;
  return RM_OK;
}

extern "C" {

int rm_dispatch_pattern(rm_ctx* c, const rm_sample_pattern* p) {
  if (!c || !p) return RM_ERR_INVALID;
  if (const char* why = pattern_invalid(p)) return fail(c, RM_ERR_INVALID, std::string("rm_dispatch_pattern: ") + why);
  int rc = refuse_extension(c, "rm_dispatch_pattern");
  if (rc != RM_OK) return rc;
  if ((rc = check_uniforms(c, c->u)) != RM_OK) return rc;
  if ((rc = set_device(c)) != RM_OK) return rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  if ((rc = ensure_table(c, *p, "rm_dispatch_pattern")) != RM_OK) return rc;
  rmd::Frame F = make_frame(c);
  // the 4x4 pixel tiles of the sample kernels, or for one sample the pixel kernels' 8x8
  // tiles, whatever u.AA says; the uniforms stay
  F.aa = p->n > 1 ? 1 : 0;
  rm::pixel_grid(F.width, F.rows, F.aa != 0, &F.grid_x, &F.grid_y);
  // |rd| = 1 over the range of this pattern's uv, not the reference offsets' (make_frame's)
  F.unit_rd = unit_rd_check(c->u.camera, F.persp, c->pat_lo, c->pat_hi) ? 1 : 0;
  rmd::PatternArgs P;
  P.uvx = static_cast<const float*>(c->pat_uv.p);
  P.uvy = P.uvx + (size_t)c->cfg.width * (size_t)p->n;
  P.n = p->n;
  P.nf = (float)p->n;
  // the events in rm_dispatch's order: the timed pair brackets the kernel alone, the phase
  // events sit outside it
  if ((rc = phase(c, 0)) != RM_OK) return rc;
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  const hipError_t e = scene_kernels(c).pattern(F, P, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "pattern frame launch");
  if ((rc = t.end(c)) != RM_OK) return rc;
  if ((rc = phase(c, 1)) != RM_OK) return rc;
  if (c->timing) {
    c->ph_recorded = true;
    c->ph_comm = false;
  }
  c->dispatched = true;
  return RM_OK;
}

}  // extern "C"
