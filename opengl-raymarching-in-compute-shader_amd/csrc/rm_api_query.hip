// rm_api_query.hip — what the host layers of the three query families share: ray
// queries (rm_api_trace.hip), SDF field queries (rm_api_sdf.hip) and SDF mesh
// extraction (rm_api_mesh.hip).  Their frame constants, the refusals and the grid
// check they have in common, the grid kernels' arguments and the context's
// grown-on-demand device buffers (rm_ctx.hpp).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "rm_ctx.hpp"

using namespace rm;

// A dispatch's frame constants but for the two facts that hold for a frame's
// primary rays only: step 0 at the camera (prepv) and |rd| = 1 (unit_rd).  The
// images and counters in F are not touched by the query kernels.
rmd::Frame rm::query_frame(const rm_ctx* c) {
  rmd::Frame F = make_frame(c);
  std::memset(F.prepv, 0, sizeof F.prepv);
  F.unit_rd = 0;
  return F;
}

int rm::refuse_multi(rm_ctx* c, const char* who) {
  if (c->subs.empty()) return RM_OK;
  return fail(c, RM_ERR_STATE, std::string(who) + ": not available on a multi-device context (cfg.ngpus)");
}

int rm::grid_points(rm_ctx* c, const char* who, const rm_sdf_grid_desc* g, int64_t* total) {
  constexpr int32_t kMaxDim = 1 << 24;
  for (int a = 0; a < 3; ++a)
    if (g->dims[a] < 0 || g->dims[a] > kMaxDim)
      return fail(c, RM_ERR_INVALID, std::string(who) + ": every dim must be in 0..2^24");
  const std::string many = std::string(who) + ": more than 2^31 - 1 points";
  int64_t t = (int64_t)g->dims[0] * g->dims[1];  // <= 2^48
  if (t > INT32_MAX && g->dims[2] != 0) return fail(c, RM_ERR_INVALID, many);
  t = g->dims[2] == 0 ? 0 : t * g->dims[2];      // <= 2^55
  if (t > INT32_MAX) return fail(c, RM_ERR_INVALID, many);
  *total = t;
  return RM_OK;
}

rmd::SdfGridArgs rm::sdf_grid_args(const rm_sdf_grid_desc* g, void* dist, void* ids) {
  rmd::SdfGridArgs G;
  for (int a = 0; a < 3; ++a) {
    G.origin[a] = g->origin[a];
    G.step[a] = g->step[a];
  }
  G.nx = g->dims[0];
  G.ny = g->dims[1];
  G.nz = g->dims[2];
  // 16-byte stores where every row of every output starts on a 16-byte boundary
  const uintptr_t da = reinterpret_cast<uintptr_t>(dist), ia = reinterpret_cast<uintptr_t>(ids);
  G.xpl = (G.nx % 4 == 0 && da % 16 == 0 && ia % 16 == 0) ? 4 : 1;
  const int per_wave = 64 * G.xpl;
  G.bpr = (uint32_t)((G.nx + per_wave - 1) / per_wave);
  G.nwg = G.bpr * (uint32_t)G.ny * (uint32_t)G.nz;  // <= nx ny nz <= 2^31 - 1
  G.dist = static_cast<float*>(dist);
  G.ids = static_cast<int32_t*>(ids);
  return G;
}

// The queries' host paths are synchronous, and hipFree waits for the device:
// nothing of an earlier call is pending on a buffer that is replaced.
int rm::ensure(rm_ctx* c, DevBuf& b, size_t need, const char* what) {
  if (need <= b.cap) return RM_OK;
  if (b.p) (void)hipFree(b.p);
  b = DevBuf();
  size_t n = 64 * 1024;
  while (n < need) n *= 2;
  if (hipMalloc(&b.p, n) != hipSuccess) {
    b.p = nullptr;
    (void)hipGetLastError();
    return fail(c, RM_ERR_NOMEM, std::string(what) + " of " + std::to_string(need) + " bytes");
  }
  b.cap = n;
  return RM_OK;
}
