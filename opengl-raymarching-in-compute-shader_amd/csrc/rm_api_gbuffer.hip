// rm_api_gbuffer.hip — librm's C-ABI for the G-buffer image (RM_OUT_GBUFFER,
// include/rm_api.h): readback and device interop.  The image is
// allocated by rm_create and written by every rm_dispatch (rm_api.hip:
// pick_kernel chooses the G-buffer kernels, rm_gbuffer.hip / rm_table_gbuffer.hip).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "rm_ctx.hpp"

using namespace rm;

static_assert(sizeof(rm_gbuffer_px) == 32, "rm_gbuffer_px: two 16-byte stores per pixel (rm_scene.hpp gbuf_store)");

extern "C" {

int rm_read_gbuffer(rm_ctx* c, rm_gbuffer_px* dst, size_t row_pitch, int flip_y) {
  if (!c) return RM_ERR_INVALID;
  return read_image(c, image_gbuf(c), sizeof(rm_gbuffer_px), dst, row_pitch, flip_y);
}

int rm_set_output_gbuffer(rm_ctx* c, void* device_ptr) {
  if (!c) return RM_ERR_INVALID;
  if (!has_gbuf(c)) return fail(c, RM_ERR_STATE, "G-buffer output not enabled in rm_config.outputs");
  if (reinterpret_cast<uintptr_t>(device_ptr) % 16 != 0)
    return fail(c, RM_ERR_INVALID, "rm_set_output_gbuffer: device_ptr must be 16-byte aligned");
  c->ext_gbuf = device_ptr;
  return RM_OK;
}

int rm_get_output_gbuffer(rm_ctx* c, void** device_ptr) {
  if (!c || !device_ptr) return RM_ERR_INVALID;
  *device_ptr = image_gbuf(c);
  return RM_OK;
}

}  // extern "C"
