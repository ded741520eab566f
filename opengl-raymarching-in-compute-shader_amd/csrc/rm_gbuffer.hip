// rm_gbuffer.hip — k_gbuf_pixel / k_gbuf_sample: the built-in scene's frame kernels
// with the fused G-buffer output (RM_OUT_GBUFFER, include/rm_api.h).
//
// A translation unit of its own, so that the render kernels' code objects
// (rm_kernels.o, rm_kernels_aa.o) are what they were without it.  The device
// code is rm_kernels.hip's, included with both of its *_ONLY switches set: that
// leaves its templates (render, pixel_body, sample_body) and drops every kernel
// and launch wrapper of its own.
//
// The kernels are k_pixel / k_sample with one more sink: render<> hands the
// primary hit it already holds (the march's t, id and albedo, and the normal it
// computes for the light term) to GbufStore (rm_scene.hpp), which writes the
// pixel's 32-byte record at once.  No second march, no second get_normal, and
// nothing of the hit stays live across the shading.  The colour image is the
// plain kernels' bit for bit: the same instantiations of march, get_normal,
// softshadow and bounce in the same order.
#define RM_KERNELS_PIXEL_ONLY
#define RM_KERNELS_AA_ONLY
#include "rm_kernels.hip"

namespace rmd {

// Waves per SIMD the register allocation must allow.
#ifndef RM_GBUF_WAVES
#define RM_GBUF_WAVES 8
#endif

__global__ __launch_bounds__(64, RM_GBUF_WAVES) void k_gbuf_pixel(Frame F, GbufArgs A) {
  pixel_body<false, true>(F, blockIdx.y, A.px);
}
// Under AA the record is the first sample's ray (lane s == 0): the fused kernel
// casts no centre ray.
__global__ __launch_bounds__(64, RM_GBUF_WAVES) void k_gbuf_sample(Frame F, GbufArgs A) {
  sample_body<false, true>(F, blockIdx.y, A.px);
}

}  // namespace rmd

namespace rm {

// F.grid_x / grid_y are pixel_grid(F.width, F.rows, F.aa) (make_frame); gbuf is a
// 16-byte aligned device pointer to rows * width records.
hipError_t launch_gbuf(const rmd::Frame& F, void* gbuf, hipStream_t s) {
  const rmd::GbufArgs A{static_cast<float4*>(gbuf)};
  const dim3 grid(F.grid_x, F.grid_y);
  if (F.aa)
    hipLaunchKernelGGL(rmd::k_gbuf_sample, grid, dim3(64), 0, s, F, A);
  else
    hipLaunchKernelGGL(rmd::k_gbuf_pixel, grid, dim3(64), 0, s, F, A);
  return hipGetLastError();
}

}  // namespace rm
