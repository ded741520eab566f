// rm_table_adaptive.hip — k_table_adapt_refine: the refinement of adaptive
// supersampling for a runtime scene table (rm_dispatch_adaptive /
// rm_dispatch_refine, include/rm_api.h).
//
// A translation unit of its own, so that rm_table.o's kernels are what they were
// without it, and outside the hiprtc sources: a context with rm_scene_specialize
// on refines through this generic, LDS-staged code too (the values are the same).
// The device code is rm_table.hip's, included without its kernels' launch
// wrappers.  The flags, the scan and the list are rm_adaptive.hip's kernels.
#define RM_TABLE_DEVICE_ONLY
#include "rm_table.hip"

#include "rm_adaptive_args.hpp"

namespace rmd {

// One instance serves every table, as k_table_gbuf_sample's (rm_table_gbuffer.hip).
// The loop is rm_adaptive.hip's k_adapt_refine over table_sample_body's pixel: the
// table staged once per wave, 16 list entries x 4 samples per round.
__global__ __launch_bounds__(64) void k_table_adapt_refine(Frame F, AdaptArgs A) {
  extern __shared__ float lds[];
  const unsigned long long total = *A.total;
  const unsigned long long ngroups = (total + 15ull) >> 4;
  if (blockIdx.x >= ngroups) return;  // (uniform: before stage's barriers)
  const Table S = stage(F, lds);
  for (unsigned long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    // the group's entries: 16, or what is left of the list
    const uint32_t* __restrict__ ent = A.list + g * 16ull;
    const unsigned long long left = total - g * 16ull;
    const int n = left < 16ull ? (int)left : 16;
    f3 col = mk(0.0f, 0.0f, 0.0f);
    {
      const int lane = threadIdx.x & 63;
      if ((lane >> 2) < n) {
        const uint32_t e = ent[lane >> 2];
        TCnt c = {0, 0, 0, 0, 0, 0};
        f3 ro, rd;
        cast_ray(F, lane_uv(F, 0, (int)(e & 0xffffu), lane & 3), lane_uv(F, 1, (int)(e >> 16), lane & 3), ro, rd);
        col = trender<false, rm::EX_MAX_SLOTS, 0>(F, S, ro, rd, c);
      }
    }
    // the lane id re-formed, and the list entry read again from it (see out_lane)
    const int ol = out_lane();
    const float r1 = __shfl(col.x, ol + 1), g1 = __shfl(col.y, ol + 1), b1 = __shfl(col.z, ol + 1);
    const float r2 = __shfl(col.x, ol + 2), g2 = __shfl(col.y, ol + 2), b2 = __shfl(col.z, ol + 2);
    const float r3 = __shfl(col.x, ol + 3), g3 = __shfl(col.y, ol + 3), b3 = __shfl(col.z, ol + 3);
    if ((ol & 3) == 0 && (ol >> 2) < n) {
      const uint32_t e = ent[ol >> 2];
      const size_t idx = (size_t)(e >> 16) * (size_t)F.width + (size_t)(e & 0xffffu);
      const float o0 = ((col.x + r1) + r2) + r3, o1 = ((col.y + g1) + g2) + g3, o2 = ((col.z + b1) + b2) + b3;
      store_pixel(F, idx, o0 / 4.0f, o1 / 4.0f, o2 / 4.0f, 1.0f);
    }
  }
}

}  // namespace rmd

namespace rm {

// The listed pixels of frame F of the table F.scene, on `waves` one-wave workgroups.
hipError_t launch_table_adapt_refine(const rmd::Frame& F, const rmd::AdaptArgs& A, int waves, hipStream_t s) {
  // the table, then the lazy slots' balls (Table::sb), as the render kernels stage them
  const size_t lds = (((rm::scene_words(F.nprims) + 3) & ~(size_t)3) + 4 * (size_t)rm::EX_MAX_SLOTS) * sizeof(float);
  hipLaunchKernelGGL(rmd::k_table_adapt_refine, dim3((unsigned)waves), dim3(64), lds, s, F, A);
  return hipGetLastError();
}

}  // namespace rm
