// rm_frame_math.hpp — the per-frame float math the host forms for the kernels
// (rm_frame_math.hip): pure arithmetic, no context and no HIP runtime call, so a
// CPU test can hold it against the oracle (tests/test_frame_math.py).
#pragma once

#include <vector>

#include "rm_internal.hpp"

namespace rm {

// Step 0 of every primary ray of the built-in scene (rm_scene.hpp PrepSlot) and
// of a compiled scene table (rm_internal.hpp TablePrep), at the camera.
void prep_host(const float cam[3], float blend, float omblend, float out[16]);
void table_prep_host(const uint32_t* words, int32_t n, const float cam[3], float blend, float omblend,
                     float out[16]);

// Frame::unit_rd: every primary ray of the frame has |rd| within 2^-20 of 1,
// for uv over [uv_lo[0], uv_hi[0]] x [uv_lo[1], uv_hi[1]].
bool unit_rd_check(const rm_camera& cam, float persp, const float uv_lo[2], const float uv_hi[2]);

// The uv table of a W x H frame (Frame::uvx / uvy): 5 values per pixel column,
// then 5 per row; the range of the columns' ([0]) and the rows' ([1]) values;
// and whether lane_uv's arithmetic (rm_scene.hpp) gives the same values.
struct UvTable {
  std::vector<float> uv;  // 5 * (W + H)
  float lo[2], hi[2];
  bool exact;
};
UvTable uv_table(int W, int H);

// Sample patterns (include/rm_api.h RM_HAS_SAMPLE_PATTERN; rm_sample_pattern_init and
// rm_pattern_uv_table are defined beside these, in rm_frame_math.hip).
// Why p (not null) is no valid pattern, or null for a valid one.
const char* pattern_invalid(const rm_sample_pattern* p);
// The uv of a valid pattern's samples by the header's rule, for a W x H frame: uvx
// [W][n] and uvy [H][n], either possibly null; and the range of the columns'
// (lo / hi [0]) and the rows' ([1]) values, which is what unit_rd_check has to cover
// for a pattern frame (the context's uv_lo / uv_hi cover the reference's offsets only).
void pattern_uv(const rm_sample_pattern& p, int W, int H, float* uvx, float* uvy, float lo[2], float hi[2]);

}  // namespace rm
