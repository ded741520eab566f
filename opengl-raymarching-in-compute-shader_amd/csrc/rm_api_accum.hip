// rm_api_accum.hip — librm's C-ABI for progressive accumulation (include/rm_api.h
// RM_HAS_ACCUMULATION): rm_dispatch_accumulate, the context's sum
// image and its sample count.  The Halton patterns are pure host math
// (rm_frame_math.hip rm_sample_pattern_halton).
//
// One such dispatch is rm_dispatch_pattern's (rm_api_pattern.hip: the pattern's uv
// table, uploaded when the pattern differs from the last call's, and one kernel),
// with the kernel that adds the pixel's samples onto the sum image and stores the
// frame from the sum (rm_accum.hip for the built-in scene, rm_table_accum.hip for a
// table).  The count is the host's: the kernel takes (float)N and whether the sum is
// continued as arguments.
//
// The contexts served and refused are rm_dispatch_pattern's.
#include <hip/hip_runtime.h>

#include <string>

#include "rm_ctx.hpp"
#include "rm_frame_math.hpp"

using namespace rm;

namespace {

// The sum image, on first use; kept until rm_destroy.
int ensure_sum(rm_ctx* c) {
  if (c->d_accum) return RM_OK;
  const size_t bytes = (size_t)c->cfg.width * (size_t)c->cfg.height * 4 * sizeof(float);
  if (hipMalloc(reinterpret_cast<void**>(&c->d_accum), bytes) != hipSuccess) {
    c->d_accum = nullptr;
    (void)hipGetLastError();
    return fail(c, RM_ERR_NOMEM, "the sum image of " + std::to_string(bytes) + " bytes");
  }
  return RM_OK;
}

}  // namespace

extern "C" {

int rm_dispatch_accumulate(rm_ctx* c, const rm_sample_pattern* p, uint32_t flags) {
  if (!c || !p) return RM_ERR_INVALID;
  if (flags & ~RM_ACCUM_RESTART) return fail(c, RM_ERR_INVALID, "rm_dispatch_accumulate: flags has an unknown bit");
  if (const char* why = pattern_invalid(p)) return fail(c, RM_ERR_INVALID, std::string("rm_dispatch_accumulate: ") + why);
  int rc = refuse_extension(c, "rm_dispatch_accumulate");
  if (rc != RM_OK) return rc;
  if ((rc = check_uniforms(c, c->u)) != RM_OK) return rc;
  if ((rc = set_device(c)) != RM_OK) return rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  if ((rc = ensure_sum(c)) != RM_OK) return rc;
  if ((rc = ensure_table(c, *p, "rm_dispatch_accumulate")) != RM_OK) return rc;
  // the frame and the table as rm_dispatch_pattern forms them
  rmd::Frame F = make_frame(c);
  F.aa = p->n > 1 ? 1 : 0;
  rm::pixel_grid(F.width, F.rows, F.aa != 0, &F.grid_x, &F.grid_y);
  F.unit_rd = unit_rd_check(c->u.camera, F.persp, c->pat_lo, c->pat_hi) ? 1 : 0;
  rmd::PatternArgs P;
  P.uvx = static_cast<const float*>(c->pat_uv.p);
  P.uvy = P.uvx + (size_t)c->cfg.width * (size_t)p->n;
  P.n = p->n;
  P.nf = (float)p->n;
  // the count stays the context's until the kernel that changes the sum is queued
  const int64_t before = (flags & RM_ACCUM_RESTART) ? 0 : c->accum_n;
  const int64_t after = before + p->n;
  rmd::AccumArgs A;
  A.sum = reinterpret_cast<float4*>(c->d_accum);
  A.nf = (float)after;  // int64 to float, round to nearest even
  A.seed = before > 0 ? 1 : 0;
  if ((rc = phase(c, 0)) != RM_OK) return rc;
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  const hipError_t e = scene_kernels(c).accum(F, P, A, c->stream);
  if (e != hipSuccess) return hip_fail(c, e, "accumulating frame launch");
  c->accum_n = after;
  c->dispatched = true;
  if ((rc = t.end(c)) != RM_OK) return rc;
  if ((rc = phase(c, 1)) != RM_OK) return rc;
  if (c->timing) {
    c->ph_recorded = true;
    c->ph_comm = false;
  }
  return RM_OK;
}

int rm_accum_reset(rm_ctx* c) {
  if (!c) return RM_ERR_INVALID;
  c->accum_n = 0;
  return RM_OK;
}

int rm_accum_samples(const rm_ctx* c, int64_t* samples) {
  if (!c || !samples) return RM_ERR_INVALID;
  *samples = c->accum_n;
  return RM_OK;
}

int rm_read_accum(rm_ctx* c, float* dst, size_t row_pitch, int flip_y) {
  if (!c || !dst) return RM_ERR_INVALID;
  if (c->accum_n == 0) return fail(c, RM_ERR_STATE, "rm_read_accum: no accumulated samples");
  return read_image(c, c->d_accum, 16, dst, row_pitch, flip_y);
}

int rm_get_accum(rm_ctx* c, void** device_ptr) {
  if (!c || !device_ptr) return RM_ERR_INVALID;
  int rc = refuse_extension(c, "rm_get_accum");
  if (rc != RM_OK) return rc;
  if ((rc = set_device(c)) != RM_OK) return rc;
  if ((rc = ensure_sum(c)) != RM_OK) return rc;
  *device_ptr = c->d_accum;
  return RM_OK;
}

}  // extern "C"
