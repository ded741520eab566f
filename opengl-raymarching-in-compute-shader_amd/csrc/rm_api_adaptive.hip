// rm_api_adaptive.hip — librm's C-ABI for adaptive supersampling (include/rm_api.h
// RM_HAS_ADAPTIVE_AA, RM_HAS_ADAPTIVE_EDGES, RM_HAS_ADAPTIVE_PATTERN; DESIGN.md §4.12,
// §4.15): rm_dispatch_adaptive, rm_dispatch_adaptive_edges, rm_dispatch_refine /
// _device, their pattern forms rm_dispatch_adaptive_pattern and
// rm_dispatch_refine_pattern / _device, and the mask and the count of the last such
// dispatch.
//
// One such dispatch is, on the context's stream: pass 1 (the kernel rm_dispatch
// would launch for the frame with AA off; on a G-buffer context the G-buffer
// kernel, which writes the records too), the flags (rm_adaptive.hip: colour
// contrast on pass 1's image, or the caller's mask; rm_adaptive_edges.hip: the
// caller's edge criteria on pass 1's G-buffer and / or image), their scan and
// list, and the refinement of the listed pixels (rm_adaptive.hip for the built-in
// scene, rm_table_adaptive.hip for a table), which writes colour only.  The host
// never learns the count.  The pattern forms refine at the offsets of a caller's
// sample pattern instead (rm_adaptive_pattern.hip, rm_table_adaptive_pattern.hip),
// from rm_dispatch_pattern's uv table (rm_api_pattern.hip ensure_table), uploaded
// before pass 1 when the pattern is not the last call's.
//
// This version: one-device, whole-frame contexts.  Out of scope, and refused:
// sharded, communicator and multi-device contexts (a pixel's neighbour may live
// on another rank), counting contexts, batches and graph replay; G-buffer
// contexts for every call but rm_dispatch_adaptive_edges, the pattern forms and the
// mask's and the count's readers; hiprtc-specialised refine kernels (the generic
// table code refines).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <string>

#include "rm_ctx.hpp"
#include "rm_frame_math.hpp"

using namespace rm;

// RM_ERR_STATE for the contexts this version does not serve, naming the call.
// gbuf_ok: the call admits a G-buffer context (rm_dispatch_adaptive_edges, and
// the mask's pointer for it).  rm_dispatch_pattern (rm_api_pattern.hip) refuses the same contexts.
int rm::refuse_extension(rm_ctx* c, const char* call, bool gbuf_ok) {
  const std::string who = std::string(call) + ": ";
  if (!c->subs.empty() || c->cfg.ngpus >= 1)
    return fail(c, RM_ERR_STATE, who + "not available on a multi-GPU context (rm_config.ngpus)");
  if (c->comm || c->group_member || c->comm_failed)
    return fail(c, RM_ERR_STATE, who + "not available on a communicator context (rm_comm_init)");
  if (c->cfg.nshards > 1) return fail(c, RM_ERR_STATE, who + "not available on a sharded context (nshards > 1)");
  if (c->cfg.counters) return fail(c, RM_ERR_STATE, who + "not available with counters");
  if (has_gbuf(c) && !gbuf_ok) return fail(c, RM_ERR_STATE, who + "not available on a G-buffer context (RM_OUT_GBUFFER)");
  if (c->graph_on) return fail(c, RM_ERR_STATE, who + "not available with rm_graph_enable on");
  return RM_OK;
}

namespace {

size_t adapt_tiles(const rm_ctx* c) {
  const size_t t = rmd::kAdaptTile;
  return ((c->cfg.width + t - 1) / t) * ((c->cfg.height + t - 1) / t);
}

// The context's buffers, on first use; kept until rm_destroy.
int ensure_buffers(rm_ctx* c) {
  if (c->d_aa_total) return RM_OK;
  const size_t npx = (size_t)c->cfg.width * (size_t)c->cfg.height;
  const size_t padded = (adapt_tiles(c) + rmd::kAdaptScanChunk - 1) / rmd::kAdaptScanChunk * rmd::kAdaptScanChunk;
  if (!c->d_aa_mask) RM_HIP(c, hipMalloc(&c->d_aa_mask, npx));
  if (!c->d_aa_list) RM_HIP(c, hipMalloc(&c->d_aa_list, npx * sizeof(uint32_t)));
  if (!c->d_aa_offsets) RM_HIP(c, hipMalloc(&c->d_aa_offsets, padded * sizeof(uint32_t)));
  if (!c->d_aa_counts) {
    RM_HIP(c, hipMalloc(&c->d_aa_counts, padded));
    // the tail of the last scan chunk stays zero: no kernel writes it
    RM_HIP(c, hipMemsetAsync(c->d_aa_counts, 0, padded, c->stream));
    RM_HIP(c, hipStreamSynchronize(c->stream));  // once: a later rm_set_stream need not order it
  }
  if (!c->aa_cus) {
    int cus = 0;
    RM_HIP(c, hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
    c->aa_cus = cus > 0 ? cus : 1;
  }
  RM_HIP(c, hipMalloc(&c->d_aa_total, sizeof(unsigned long long)));  // last: marks the set complete
  return RM_OK;
}

// The refinement's grid: the host does not know the count, so a fixed number of
// one-wave workgroups stride over the groups.  Four times the waves the device
// holds at k_adapt_refine's 8 per SIMD (32 per compute unit), or as many as the
// frame has groups: the hardware hands the queued waves to the SIMDs as they
// free up, which balances the groups' very uneven costs better than 32 per unit
// striding further each (4K cfg3 frames at threshold 8, alone on the device:
// 1.04 ms at 32 per unit, 0.99 at 64, 0.85 at 128, 0.86 at 65535 waves;
// profiles/adaptive_probe.txt).
// per: the list entries of a group, 16, or 64 for a pattern of one sample.
constexpr size_t kRefineWavesPerCU = 128;
int refine_waves(const rm_ctx* c, size_t per = 16) {
  if (c->aa_waves_env) return c->aa_waves_env;
  const size_t groups = ((size_t)c->cfg.width * (size_t)c->cfg.height + per - 1) / per;
  return (int)std::min(groups, (size_t)c->aa_cus * kRefineWavesPerCU);
}

// The classifier's plain form instead of its two-pair form (rm_adaptive_edges.hip):
// RM_AA_EDGES_NAIVE set to anything but "0".  Read by every call: a measurement
// switches it between two frames of one context.
bool edges_naive() {
  const char* v = std::getenv("RM_AA_EDGES_NAIVE");
  return v && *v && std::strcmp(v, "0") != 0;
}

// One adaptive frame.  The flags: the caller's edge criteria `cr`; else a device
// mask mask_src at mask_pitch; else (both null) colour contrast at `threshold`.
// The refinement: the reference's four samples, or with `pat` (valid) that
// pattern's, for the call `call`.
int adaptive_frame(rm_ctx* c, const void* mask_src, size_t mask_pitch, int threshold,
                   const rm_aa_criteria* cr = nullptr, const rm_sample_pattern* pat = nullptr,
                   const char* call = nullptr) {
  int rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  // (the table's upload, when there is one, before the timed pair)
  if (pat && (rc = ensure_table(c, *pat, call)) != RM_OK) return rc;
  rmd::Frame F = make_frame(c);
  F.aa = 0;  // pass 1 is the AA-off frame whatever u.AA says; the uniforms stay
  rm::pixel_grid(F.width, F.rows, false, &F.grid_x, &F.grid_y);
  rmd::AdaptArgs A;
  A.mask = c->d_aa_mask;
  A.counts = c->d_aa_counts;
  A.offsets = c->d_aa_offsets;
  A.total = c->d_aa_total;
  A.list = c->d_aa_list;
  A.width = c->cfg.width;
  A.height = c->cfg.height;
  A.tiles_x = (c->cfg.width + rmd::kAdaptTile - 1) / rmd::kAdaptTile;
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  if ((rc = phase(c, 0)) != RM_OK) return rc;
  // (image_gbuf: null without RM_OUT_GBUFFER; with it pass 1 writes the records the criteria read)
  hipError_t e = launch(pick_kernel(c, F), F, false, c->stream, image_gbuf(c));
  if (e != hipSuccess) return hip_fail(c, e, "adaptive pass 1 launch");
  if (cr) {
    const rmd::EdgeArgs E{image_gbuf(c), F.rgba8, F.rgba32f, cr->edges, cr->color_threshold, cr->depth_rel,
                          cr->normal_cos};
    e = launch_adapt_edges(A, E, !edges_naive(), c->stream);
    if (e == hipSuccess) e = launch_adapt_list(A, c->stream);
  } else {
    e = launch_adapt_flags(F, A, mask_src, mask_pitch, threshold, c->stream);
  }
  if (e != hipSuccess) return hip_fail(c, e, "adaptive flag launch");
  if (pat) {
    // |rd| = 1 over the range of this pattern's uv: pass 1's unit_rd (make_frame's) is
    // proved for the centre rays and the reference offsets only
    rmd::Frame R = F;
    R.unit_rd = unit_rd_check(c->u.camera, F.persp, c->pat_lo, c->pat_hi) ? 1 : 0;
    rmd::PatternArgs P;
    P.uvx = static_cast<const float*>(c->pat_uv.p);
    P.uvy = P.uvx + (size_t)c->cfg.width * (size_t)pat->n;
    P.n = pat->n;
    P.nf = (float)pat->n;
    e = scene_kernels(c).adapt_refine_pattern(R, A, P, refine_waves(c, pat->n == 1 ? 64 : 16), c->stream);
  } else {
    e = scene_kernels(c).adapt_refine(F, A, refine_waves(c), c->stream);
  }
  if (e != hipSuccess) return hip_fail(c, e, "adaptive refine launch");
  if ((rc = phase(c, 1)) != RM_OK) return rc;
  if ((rc = t.end(c)) != RM_OK) return rc;
  if (c->timing) {
    c->ph_recorded = true;
    c->ph_comm = false;
  }
  c->dispatched = true;
  c->aa_dispatched = true;
  return RM_OK;
}

// What every such dispatch checks and prepares before its frame.
int begin(rm_ctx* c, const char* call, bool gbuf_ok = false) {
  int rc = refuse_extension(c, call, gbuf_ok);
  if (rc != RM_OK) return rc;
  if ((rc = check_uniforms(c, c->u)) != RM_OK) return rc;
  if ((rc = set_device(c)) != RM_OK) return rc;
  return ensure_buffers(c);
}

// A context with RM_OUT_GBUFFER and no colour output has nothing to refine.
int check_colour(rm_ctx* c, const char* call) {
  if (!(c->cfg.outputs & (RM_OUT_RGBA8 | RM_OUT_RGBA32F)))
    return fail(c, RM_ERR_STATE, std::string(call) + ": the context has no colour output to refine");
  return RM_OK;
}

int check_mask(rm_ctx* c, const char* call, const void* mask, size_t* row_pitch) {
  if (!mask) return fail(c, RM_ERR_INVALID, std::string(call) + ": null mask");
  if (*row_pitch == 0) *row_pitch = (size_t)c->cfg.width;
  if (*row_pitch < (size_t)c->cfg.width)
    return fail(c, RM_ERR_INVALID, std::string(call) + ": row_pitch smaller than a row");
  return RM_OK;
}

// The checks of rm_dispatch_adaptive_edges' criteria, in its order, for `call`: the
// fields' ranges (RM_ERR_INVALID), then what the selected criteria and the refinement
// need of the context (RM_ERR_STATE).
int check_criteria(rm_ctx* c, const char* call, const rm_aa_criteria* cr) {
  const std::string who = std::string(call) + ": ";
  if (!cr) return fail(c, RM_ERR_INVALID, who + "null criteria");
  if (cr->struct_size != sizeof(rm_aa_criteria))
    return fail(c, RM_ERR_INVALID, who + "rm_aa_criteria.struct_size is not sizeof(rm_aa_criteria)");
  constexpr uint32_t kGeometry = RM_AA_EDGE_ID | RM_AA_EDGE_DEPTH | RM_AA_EDGE_NORMAL | RM_AA_EDGE_ALBEDO;
  if (cr->edges == 0 || (cr->edges & ~(kGeometry | RM_AA_EDGE_COLOR)))
    return fail(c, RM_ERR_INVALID, who + "edges must be a non-empty mask of RM_AA_EDGE_* bits");
  if ((cr->edges & RM_AA_EDGE_COLOR) && (cr->color_threshold < 0 || cr->color_threshold > 255))
    return fail(c, RM_ERR_INVALID, who + "color_threshold must be in 0..255");
  // (written so that a NaN fails)
  if ((cr->edges & RM_AA_EDGE_DEPTH) && !(cr->depth_rel >= 0.0f))
    return fail(c, RM_ERR_INVALID, who + "depth_rel must be >= 0 (+inf allowed)");
  if ((cr->edges & RM_AA_EDGE_NORMAL) && !(cr->normal_cos >= -1.0f && cr->normal_cos <= 1.0f))
    return fail(c, RM_ERR_INVALID, who + "normal_cos must be in [-1, 1]");
  if ((cr->edges & kGeometry) && !has_gbuf(c))
    return fail(c, RM_ERR_STATE, who + "the ID, DEPTH, NORMAL and ALBEDO criteria need RM_OUT_GBUFFER in rm_config.outputs");
  return check_colour(c, call);
}

// RM_ERR_INVALID, naming `call`, with rm::pattern_invalid's reason for a null or invalid pattern.
int check_pattern(rm_ctx* c, const char* call, const rm_sample_pattern* p) {
  if (!p) return fail(c, RM_ERR_INVALID, std::string(call) + ": null pattern");
  if (const char* why = pattern_invalid(p)) return fail(c, RM_ERR_INVALID, std::string(call) + ": " + why);
  return RM_OK;
}

}  // namespace

extern "C" {

int rm_dispatch_adaptive(rm_ctx* c, int32_t threshold) {
  if (!c) return RM_ERR_INVALID;
  if (threshold < 0 || threshold > 255)
    return fail(c, RM_ERR_INVALID, "rm_dispatch_adaptive: threshold must be in 0..255");
  const int rc = begin(c, "rm_dispatch_adaptive");
  if (rc != RM_OK) return rc;
  return adaptive_frame(c, nullptr, 0, threshold);
}

int rm_aa_criteria_init(rm_aa_criteria* cr) {
  if (!cr) return RM_ERR_INVALID;
  cr->struct_size = (uint32_t)sizeof(rm_aa_criteria);
  cr->edges = RM_AA_EDGE_ID | RM_AA_EDGE_DEPTH | RM_AA_EDGE_NORMAL;
  cr->color_threshold = 8;
  cr->depth_rel = 0.05f;
  cr->normal_cos = 0.9f;
  return RM_OK;
}

int rm_dispatch_adaptive_edges(rm_ctx* c, const rm_aa_criteria* cr) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_criteria(c, "rm_dispatch_adaptive_edges", cr);
  if (rc != RM_OK) return rc;
  if ((rc = begin(c, "rm_dispatch_adaptive_edges", true)) != RM_OK) return rc;
  return adaptive_frame(c, nullptr, 0, 0, cr);
}

int rm_dispatch_adaptive_pattern(rm_ctx* c, const rm_aa_criteria* cr, const rm_sample_pattern* p) {
  if (!c) return RM_ERR_INVALID;
  const char* call = "rm_dispatch_adaptive_pattern";
  int rc = check_pattern(c, call, p);
  if (rc != RM_OK) return rc;
  if ((rc = check_criteria(c, call, cr)) != RM_OK) return rc;
  if ((rc = begin(c, call, true)) != RM_OK) return rc;
  return adaptive_frame(c, nullptr, 0, 0, cr, p, call);
}

int rm_dispatch_refine(rm_ctx* c, const uint8_t* mask, size_t row_pitch) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_mask(c, "rm_dispatch_refine", mask, &row_pitch);
  if (rc != RM_OK) return rc;
  if ((rc = begin(c, "rm_dispatch_refine")) != RM_OK) return rc;
  // into the context's mask, tight, behind whatever still reads it; the caller's
  // buffer is free on return.  k_adapt_mask then normalises it in place.
  const size_t w = (size_t)c->cfg.width;
  RM_HIP(c, hipMemcpy2DAsync(c->d_aa_mask, w, mask, row_pitch, w, (size_t)c->cfg.height, hipMemcpyHostToDevice,
                             c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return adaptive_frame(c, c->d_aa_mask, w, 0);
}

int rm_dispatch_refine_device(rm_ctx* c, const void* mask_dev, size_t row_pitch) {
  if (!c) return RM_ERR_INVALID;
  int rc = check_mask(c, "rm_dispatch_refine_device", mask_dev, &row_pitch);
  if (rc != RM_OK) return rc;
  if ((rc = begin(c, "rm_dispatch_refine_device")) != RM_OK) return rc;
  return adaptive_frame(c, mask_dev, row_pitch, 0);
}

int rm_dispatch_refine_pattern(rm_ctx* c, const uint8_t* mask, size_t row_pitch, const rm_sample_pattern* p) {
  if (!c) return RM_ERR_INVALID;
  const char* call = "rm_dispatch_refine_pattern";
  int rc = check_pattern(c, call, p);
  if (rc != RM_OK) return rc;
  if ((rc = check_mask(c, call, mask, &row_pitch)) != RM_OK) return rc;
  if ((rc = check_colour(c, call)) != RM_OK) return rc;
  if ((rc = begin(c, call, true)) != RM_OK) return rc;
  // the upload of rm_dispatch_refine
  const size_t w = (size_t)c->cfg.width;
  RM_HIP(c, hipMemcpy2DAsync(c->d_aa_mask, w, mask, row_pitch, w, (size_t)c->cfg.height, hipMemcpyHostToDevice,
                             c->stream));
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return adaptive_frame(c, c->d_aa_mask, w, 0, nullptr, p, call);
}

int rm_dispatch_refine_pattern_device(rm_ctx* c, const void* mask_dev, size_t row_pitch,
                                      const rm_sample_pattern* p) {
  if (!c) return RM_ERR_INVALID;
  const char* call = "rm_dispatch_refine_pattern_device";
  int rc = check_pattern(c, call, p);
  if (rc != RM_OK) return rc;
  if ((rc = check_mask(c, call, mask_dev, &row_pitch)) != RM_OK) return rc;
  if ((rc = check_colour(c, call)) != RM_OK) return rc;
  if ((rc = begin(c, call, true)) != RM_OK) return rc;
  return adaptive_frame(c, mask_dev, row_pitch, 0, nullptr, p, call);
}

int rm_read_aa_mask(rm_ctx* c, uint8_t* dst, size_t row_pitch, int flip_y) {
  if (!c) return RM_ERR_INVALID;
  if (!c->aa_dispatched)
    return fail(c, RM_ERR_STATE, "rm_read_aa_mask: no adaptive dispatch (rm_dispatch_adaptive* / rm_dispatch_refine*) yet");
  return read_image(c, c->d_aa_mask, 1, dst, row_pitch, flip_y);
}

int rm_get_aa_mask(rm_ctx* c, void** device_ptr) {
  if (!c || !device_ptr) return RM_ERR_INVALID;
  int rc = refuse_extension(c, "rm_get_aa_mask", true);
  if (rc != RM_OK) return rc;
  if ((rc = set_device(c)) != RM_OK) return rc;
  if ((rc = ensure_buffers(c)) != RM_OK) return rc;
  *device_ptr = c->d_aa_mask;
  return RM_OK;
}

int rm_aa_refined(rm_ctx* c, int64_t* pixels) {
  if (!c || !pixels) return RM_ERR_INVALID;
  if (!c->aa_dispatched)
    return fail(c, RM_ERR_STATE, "rm_aa_refined: no adaptive dispatch (rm_dispatch_adaptive* / rm_dispatch_refine*) yet");
  const int rc = set_device(c);
  if (rc != RM_OK) return rc;
  unsigned long long n = 0;
  RM_HIP(c, hipStreamSynchronize(c->stream));
  RM_HIP(c, hipMemcpy(&n, c->d_aa_total, sizeof n, hipMemcpyDeviceToHost));
  *pixels = (int64_t)n;
  return RM_OK;
}

}  // extern "C"
