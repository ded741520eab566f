// rm_table_gbuffer.hip — k_table_gbuf_pixel / k_table_gbuf_sample: a runtime scene
// table's frame kernels with the fused G-buffer output (RM_OUT_GBUFFER,
// include/rm_api.h).
//
// A translation unit of its own, so that rm_table.o's kernels are what they were
// without it, and outside the hiprtc sources: a G-buffer context with
// rm_scene_specialize on renders through this generic, LDS-staged code too.  The
// device code is rm_table.hip's (trender and the two bodies over the staged
// Table), included without its kernels' launch wrappers.  trender hands the
// primary hit it holds to GbufStore (rm_scene.hpp): see rm_gbuffer.hip.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

namespace rmd {

// One instance serves every table, as k_table_trace's (rm_table_trace.hip):
// EX_MAX_SLOTS lazy slots hold any table's, and TLazy is the march every table
// can take; the reference-shaped and plane-bounded shapes and the specialised
// kernels compute the same values.  No bound on the waves: the bounded generic
// kernels spill to scratch (rm_table.hip RM_TABLE_MIN_WAVES), these do not.
constexpr int kGbufKL = rm::EX_MAX_SLOTS;
__global__ __launch_bounds__(64) void k_table_gbuf_pixel(Frame F, GbufArgs A) {
  extern __shared__ float lds[];
  table_pixel_body<false, kGbufKL, 0, true>(F, lds, blockIdx.y, A.px);
}
__global__ __launch_bounds__(64) void k_table_gbuf_sample(Frame F, GbufArgs A) {
  extern __shared__ float lds[];
  table_sample_body<false, kGbufKL, 0, true>(F, lds, blockIdx.y, A.px);
}

}  // namespace rmd

namespace rm {

// The frame F of the table F.scene; gbuf is a 16-byte aligned device pointer to
// rows * width records.
hipError_t launch_table_gbuf(const rmd::Frame& F, void* gbuf, hipStream_t s) {
  const rmd::GbufArgs A{static_cast<float4*>(gbuf)};
  hipLaunchKernelGGL(F.aa ? rmd::k_table_gbuf_sample : rmd::k_table_gbuf_pixel, table_tile_grid(F), dim3(64),
                     table_lds_bytes(F.nprims), s, F, A);
  return hipGetLastError();
}

}  // namespace rm
