// rm_ctx.hpp — the context, and what the files of librm's C-ABI share:
// rm_api.hip (context, uniforms, dispatch, readback, timing, interop),
// rm_api_comm.hip (RCCL-gathered frames), rm_api_graph.hip (hipGraph replay),
// rm_api_trace.hip (ray queries), rm_api_gbuffer.hip (the G-buffer image),
// rm_api_sdf.hip (SDF field queries), rm_api_adaptive.hip (adaptive supersampling),
// rm_api_pattern.hip (sample-pattern frames and the pattern's table), rm_api_accum.hip
// (progressive accumulation), rm_api_mesh.hip (SDF mesh extraction) and rm_api_query.hip (what the three query
// families share: their frame constants, checks and staging buffers).
// Internal: nothing here is part of include/rm_api.h.
#pragma once

#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "rm_accum_args.hpp"
#include "rm_adaptive_args.hpp"
#include "rm_comm.hpp"
#include "rm_internal.hpp"
#include "rm_jit.hpp"
#include "rm_mesh_args.hpp"
#include "rm_pattern_args.hpp"
#include "rm_scene.hpp"
#include "rm_sdf_args.hpp"

static_assert(RM_MAX_BATCH == rmd::kMaxBatch, "rm_api.h RM_MAX_BATCH == rm_scene.hpp kMaxBatch");

namespace rm {

// ---- the kernels' launch wrappers (rm_kernels.hip, rm_table.hip) ---------------------
// A query family (rays, SDF fields, adaptive refinement) is one body in its header
// (rm_trace.hpp, rm_sdf.hpp, rm_adaptive_args.hpp) over the fast-path scene interface
// (Fast, rm_trace.hpp: BuiltinFast in rm_builtin_fast.hpp, TableFast in rm_table_lit.hpp)
// and the literal path's (Scene: BuiltinLit, TableLit), and per scene a translation
// unit with the kernel that calls the body and the launch wrapper below.
void pixel_grid(int width, int rows, bool aa, int32_t* gx, int32_t* gy);
hipError_t launch_pixel(const rmd::Frame& F, bool counters, hipStream_t s);
hipError_t launch_table(const rmd::Frame& F, bool counters, hipStream_t s, int nslots, int shape);
hipError_t launch_table_frames(const rmd::FrameBatch& B, int n, hipStream_t s, int nslots, int shape);
int table_shape(const uint32_t* words, int32_t n);
hipError_t launch_unshard(const void* gathered, void* frame, int width, int height, int row_block,
                          int row_block0, int nshards, int rows_cap, hipStream_t s, size_t rank_stride_rows = 0,
                          bool rgb3 = false);
hipError_t launch_frames(const rmd::FrameBatch& B, int n, hipStream_t s);
// ray queries (rm_trace.hip, rm_table_trace.hip): n >= 1 rays, device pointers
hipError_t launch_trace(const rmd::Frame& F, const void* origins, const void* dirs, void* hits, int64_t n,
                        uint32_t flags, hipStream_t s);
hipError_t launch_table_trace(const rmd::Frame& F, const void* origins, const void* dirs, void* hits,
                              int64_t n, uint32_t flags, hipStream_t s);
// SDF field queries (rm_sdf.hip, rm_table_sdf.hip): n >= 1 points, a grid of dims >= 1
// (rm_sdf_args.hpp SdfGridArgs), device pointers
hipError_t launch_sdf_points(const rmd::Frame& F, const void* points, void* out, int64_t n, uint32_t flags,
                             hipStream_t s);
hipError_t launch_table_sdf_points(const rmd::Frame& F, const void* points, void* out, int64_t n, uint32_t flags,
                                   hipStream_t s);
hipError_t launch_sdf_grid(const rmd::Frame& F, const rmd::SdfGridArgs& G, hipStream_t s);
hipError_t launch_table_sdf_grid(const rmd::Frame& F, const rmd::SdfGridArgs& G, hipStream_t s);
// the frame kernels with the G-buffer output (rm_gbuffer.hip, rm_table_gbuffer.hip):
// gbuf is a 16-byte aligned device pointer to F.rows * F.width rm_gbuffer_px
hipError_t launch_gbuf(const rmd::Frame& F, void* gbuf, hipStream_t s);
hipError_t launch_table_gbuf(const rmd::Frame& F, void* gbuf, hipStream_t s);
// adaptive supersampling (rm_adaptive.hip, rm_table_adaptive.hip): the flags of pass 1's
// image F.rgba8 / F.rgba32f (mask_src null) or of a device mask, scanned and listed; then
// the listed pixels rendered as the AA-on frame's, on `waves` one-wave workgroups
hipError_t launch_adapt_flags(const rmd::Frame& F, const rmd::AdaptArgs& A, const void* mask_src, size_t mask_pitch,
                              int threshold, hipStream_t s);
// the flags of the caller's edge criteria on pass 1's G-buffer and / or image
// (rm_adaptive_edges.hip; exchange: its two-pair form), then their scan and list alone
hipError_t launch_adapt_edges(const rmd::AdaptArgs& A, const rmd::EdgeArgs& E, bool exchange, hipStream_t s);
hipError_t launch_adapt_list(const rmd::AdaptArgs& A, hipStream_t s);
hipError_t launch_adapt_refine(const rmd::Frame& F, const rmd::AdaptArgs& A, int waves, hipStream_t s);
hipError_t launch_table_adapt_refine(const rmd::Frame& F, const rmd::AdaptArgs& A, int waves, hipStream_t s);
// a sample-pattern frame (rm_pattern.hip, rm_table_pattern.hip): frame F, whose grid_x / grid_y
// are pixel_grid's with aa set, at the pattern's device table P
hipError_t launch_pattern(const rmd::Frame& F, const rmd::PatternArgs& P, hipStream_t s);
hipError_t launch_table_pattern(const rmd::Frame& F, const rmd::PatternArgs& P, hipStream_t s);
// an accumulating pattern frame (rm_accum.hip, rm_table_accum.hip): launch_pattern's frame and
// table, and the sum image, the divisor and whether the sum is continued (rm_accum_args.hpp)
hipError_t launch_accum(const rmd::Frame& F, const rmd::PatternArgs& P, const rmd::AccumArgs& A, hipStream_t s);
hipError_t launch_table_accum(const rmd::Frame& F, const rmd::PatternArgs& P, const rmd::AccumArgs& A,
                              hipStream_t s);
// pattern refinement in the adaptive calls (rm_adaptive_pattern.hip, rm_table_adaptive_pattern.hip):
// the listed pixels rendered as the pattern frame's, at the pattern's device table P, on `waves`
// one-wave workgroups
hipError_t launch_adapt_refine_pattern(const rmd::Frame& F, const rmd::AdaptArgs& A, const rmd::PatternArgs& P,
                                       int waves, hipStream_t s);
hipError_t launch_table_adapt_refine_pattern(const rmd::Frame& F, const rmd::AdaptArgs& A, const rmd::PatternArgs& P,
                                             int waves, hipStream_t s);
// SDF mesh extraction (rm_mesh.hip), every dim >= 2: the waves' ballots and counts of M.vol,
// their scans and the mesh's counts; then the vertices below M.vcap and the quads below
// M.qcap; the device call's records below min(counts[0], vcap) out of n >= 1 staged ones
hipError_t launch_mesh_count(const rmd::MeshArgs& M, hipStream_t s);
hipError_t launch_mesh_emit(const rmd::MeshArgs& M, hipStream_t s);
hipError_t launch_mesh_attr_copy(const void* src, void* dst, const void* counts, int64_t vcap, int64_t n,
                                 hipStream_t s);

// Which kernel renders a frame (rm_api.hip pick_kernel): the built-in scene's, or
// for a runtime scene table its specialised kernels (jit) or the generic table
// kernel's instance (nslots, shape: rm_table.hip launch_table).  Frames of one
// RenderKernel share a launch of a batch, and a captured graph.  A G-buffer
// context (RM_OUT_GBUFFER) renders with the G-buffer kernels: one for the
// built-in scene, one for every table (jit null, nslots and shape unused).
struct RenderKernel {
  bool table = false;
  bool gbuf = false;
  int aa = 0;                   // the grid shape depends on it
  const JitTable* jit = nullptr;
  int nslots = 0, shape = 0;    // the generic table kernel's instance (jit null)
  bool operator==(const RenderKernel& o) const {
    return table == o.table && gbuf == o.gbuf && aa == o.aa && jit == o.jit && nslots == o.nslots &&
           shape == o.shape;
  }
  // The launched kernel's argument is a FrameBatch, not a Frame: every table
  // production kernel renders a single frame as a batch of one (rm_table.hip
  // launch_table_kl, rm_jit.hip launch_table_jit); the counting kernels and the
  // built-in scene's take the Frame.
  bool takes_batch(bool counters) const { return table && !counters; }
};

// The kernels that are not frame kernels, for the built-in scene or for a runtime
// scene table (rm_api.hip scene_kernels): the launch wrappers above.
struct SceneKernels {
  decltype(launch_trace)* trace;
  decltype(launch_sdf_points)* sdf_points;
  decltype(launch_sdf_grid)* sdf_grid;
  decltype(launch_adapt_refine)* adapt_refine;
  decltype(launch_pattern)* pattern;
  decltype(launch_adapt_refine_pattern)* adapt_refine_pattern;
  decltype(launch_accum)* accum;
};

// A device buffer the context owns and grows on demand (rm_api_query.hip ensure).
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;  // bytes
};

}  // namespace rm

// The graph path: the captured frame (the render kernel, and for a rank of an
// RCCL-gathered frame the gather and the assembly after it) whose render node
// gets the frame's by-value constants per replay (hipGraphExecKernelNodeSetParams).
struct rm_graph_slot {
  hipGraph_t graph = nullptr;
  hipGraphNode_t render = nullptr;  // the render kernel's node (its argument: RenderKernel::takes_batch)
  hipGraphExec_t exec = nullptr;
  rm::RenderKernel kernel;          // the kernel captured
  const void* send = nullptr;       // buffers the captured gather / assembly use
  const void* frame = nullptr;
};

struct rm_ctx {
  rm_config cfg{};
  int device = 0;
  int rows = 0;  // rows rendered per dispatch (height, or the shard's rows_cap)
  rm_uniforms u{};
  hipStream_t stream = nullptr;
  bool own_stream = false;
  uint8_t* d_rgba8 = nullptr;     // own RGBA8 image
  uint8_t* ext_rgba8 = nullptr;   // caller-provided RGBA8 image (rm_set_output_rgba8)
  // the RGBA8 shard images are packed RGB, 3 B per pixel (rm_config.shard_format:
  // RGB8, or AUTO once the context gathers): the render writes them, the gather
  // moves them, k_unshard expands them with alpha 255
  bool rgb3 = false;
  float* d_rgba32f = nullptr;
  void* d_gbuf = nullptr;         // own G-buffer image (RM_OUT_GBUFFER): [rows][width] rm_gbuffer_px
  void* ext_gbuf = nullptr;       // caller-provided one (rm_set_output_gbuffer)
  uint32_t* d_counts = nullptr;
  unsigned long long* d_counters = nullptr;
  float* d_uv = nullptr;          // per-column / per-row uv table (Frame::uvx / uvy)
  bool uv_exact = false;          // lane_uv's arithmetic equals the table (rm_frame_math.hip uv_table)
  float uv_lo[2] = {0, 0}, uv_hi[2] = {0, 0};  // range of the table's column / row values
  uint32_t* d_scene = nullptr;    // runtime scene table (rm_set_scene), compiled words
  int nprims = 0;                 // 0: the built-in scene and its specialised kernel
  std::vector<rm_primitive> scene;     // the table as given (rm_get_scene)
  std::vector<uint32_t> scene_words;   // host copy of d_scene (source of the async upload)
  bool specialize = false;             // rm_scene_specialize: tables render with hiprtc kernels
  const rm::JitTable* jit = nullptr;   // the current table's specialised kernels, or null
  bool dispatched = false;
  bool timing = false;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;
  std::vector<int> ev_frames;  // frames each timed launch rendered (a batch: n)
  size_t ev_used = 0;
  double total_ms = 0.0;
  int64_t launches = 0;
  bool graph_on = false;
  rm_graph_slot gs;
  // RCCL-gathered frames (rm_comm_init, or one device of a multi-GPU context)
  ncclComm_t comm = nullptr;
  bool own_comm = false;      // destroyed with the context
  bool group_member = false;  // a device of a multi-GPU context: its parent issues the gather
  bool comm_warm = false;     // a gather has run eagerly (before any graph capture)
  int crank = 0, cranks = 1;
  uint8_t* d_gathered = nullptr;  // rank 0: [cranks][rows][width] RGBA8; its own shard renders into slot 0
  uint8_t* d_frame = nullptr;     // rank 0: the assembled [height][width] frame
  float* d_gathered32 = nullptr;  // the same two for RGBA32F (16 B/px)
  float* d_frame32 = nullptr;
  long comm_timeout_ms = 0;       // deadline of every wait on the communicator (0: none)
  bool comm_failed = false;       // the communicator was aborted (RM_ERR_COMM from then on)
  std::string comm_why;           // why it was aborted
  // phase events of the last timed eager dispatch: render start / end, gather end, assembly end
  hipEvent_t ph[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ph_recorded = false, ph_comm = false;
  // frame batches (rm_dispatch_frames)
  int batch_n = 1;                  // frames of the last dispatch (a plain dispatch: 1)
  std::vector<uint8_t*> ring8;      // frames 0..n-2 of the last batch (rank 0 of a communicator: assembled)
  std::vector<float*> ring32;
  // communicator contexts: two batch slots, so batch j + 1 renders while batch j
  // gathers on gstream.  A slot's send8 / send32 hold this rank's shards of the
  // batch's frames, [n][rows][width]; rank 0's is the whole gather buffer,
  // [nranks][n][rows][width], its own shards rendering in place into [0].
  struct BatchSlot {
    uint8_t* send8 = nullptr;
    float* send32 = nullptr;
    int cap = 0;                   // frames the buffers hold
    hipEvent_t rendered = nullptr; // the batch's render, on stream
    hipEvent_t freed = nullptr;    // its gather and assembly, on gstream
    bool pending = false;          // freed recorded and not yet waited for
  } bslot[2];
  int bnext = 0, blast = -1;        // the next slot; the slot of the last batch
  hipStream_t gstream = nullptr;    // gathers + assembly of batches
  hipEvent_t gdone = nullptr;       // the last batch's work on gstream
  hipEvent_t out_ev = nullptr;      // rm_wait_output: the tail of the context's stream
  bool gdone_pending = false;       // plain dispatches order after it
  // The staging buffers of the query families' host paths, which are synchronous: neither
  // is live once a call returns, so the three families share them.  rm_trace_rays: the
  // origins, and the dirs behind them at a 256-byte boundary; the hits.  rm_sdf_points: the
  // points; the records.  rm_sdf_grid: the ids; the distances.  rm_sdf_mesh: the positions;
  // the records.
  rm::DevBuf stage_in, stage_out;
  // adaptive supersampling (rm_api_adaptive.hip), allocated on first use: the 0/1 mask
  // [height][width], the flagged pixels' list [height * width], the 8x8 tiles' counts and
  // offsets (whole scan chunks, rm_adaptive_args.hpp) and the total
  uint8_t* d_aa_mask = nullptr;
  uint32_t* d_aa_list = nullptr;
  uint8_t* d_aa_counts = nullptr;
  uint32_t* d_aa_offsets = nullptr;
  unsigned long long* d_aa_total = nullptr;
  bool aa_dispatched = false;  // the mask and the total are those of a dispatch
  int aa_waves_env = 0;        // RM_AA_REFINE_WAVES at rm_create (0: unset)
  int aa_cus = 0;              // the device's compute units (first adaptive dispatch)
  // SDF mesh extraction (rm_api_mesh.hip): the distance volume; the counts and the per-wave
  // arrays (rm_mesh_args.hpp); rm_sdf_mesh's staging of the indices; rm_sdf_mesh_device's of
  // the records
  rm::DevBuf mesh_vol, mesh_waves, mesh_idx, mesh_attr;
  // sample-pattern frames and pattern refinement (rm_api_pattern.hip ensure_table): the last
  // pattern of either kind of call, its uv table on the device (uvx [width][n], then uvy
  // [height][n]) and the range of its values per axis
  rm::DevBuf pat_uv;
  rm_sample_pattern pat{};  // pat.n == 0: none yet
  float pat_lo[2] = {0, 0}, pat_hi[2] = {0, 0};
  float* pat_host = nullptr;     // the table's pinned host copy, the source of the upload
  hipEvent_t pat_ev = nullptr;   // the last upload, on the stream it was queued on
  bool pat_ev_pending = false;   // recorded and not yet waited for: pat_host is still being read
  // progressive accumulation (rm_api_accum.hip): the sum image [height][width] float4, allocated
  // on first use, and the samples in it; only rm_dispatch_accumulate and rm_accum_reset touch them
  float* d_accum = nullptr;
  int64_t accum_n = 0;
  // a multi-GPU context (rm_config.ngpus): one shard context per device, subs[0] = rank 0
  std::vector<rm_ctx*> subs;
  std::string err;
};

namespace rm {

// ---- errors (rm_api.hip) ---------------------------------------------------------------
// Sets the context's error, or with c null the thread's creation error
// (rm_last_error(nullptr)), and returns code.
int fail(rm_ctx* c, int code, const std::string& msg);
int hip_fail(rm_ctx* c, hipError_t e, const char* what);

#define RM_HIP(c, call)                              \
  do {                                               \
    hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return rm::hip_fail(c, e_, #call); \
  } while (0)

// ---- where images live --------------------------------------------------------------
// A plain context renders into its RGBA8 image (the caller's, or its own).  Rank 0
// of an RCCL-gathered frame renders its shard into slot 0 of the gather buffer and
// its readable image is the assembled frame; the other ranks' is their shard.
inline bool comm_root(const rm_ctx* c) { return c->comm && c->crank == 0; }
inline uint8_t* render_dst(const rm_ctx* c) {
  if (!(c->cfg.outputs & RM_OUT_RGBA8)) return nullptr;
  if (comm_root(c)) return c->d_gathered;
  return c->ext_rgba8 ? c->ext_rgba8 : c->d_rgba8;
}
inline uint8_t* image_rgba8(const rm_ctx* c) {
  if (!c->subs.empty()) return image_rgba8(c->subs[0]);
  if (comm_root(c)) return c->ext_rgba8 ? c->ext_rgba8 : c->d_frame;
  return render_dst(c);
}
inline float* render_dst32(const rm_ctx* c) {
  if (!(c->cfg.outputs & RM_OUT_RGBA32F)) return nullptr;
  return comm_root(c) ? c->d_gathered32 : c->d_rgba32f;
}
inline float* image_rgba32f(const rm_ctx* c) {
  if (!c->subs.empty()) return image_rgba32f(c->subs[0]);
  if (comm_root(c)) return c->d_frame32;
  return render_dst32(c);
}
// A G-buffer context has no communicator and no devices of its own: it renders
// into, and reads, one image.
inline bool has_gbuf(const rm_ctx* c) { return (c->cfg.outputs & RM_OUT_GBUFFER) != 0; }
inline void* image_gbuf(const rm_ctx* c) {
  if (!has_gbuf(c)) return nullptr;
  return c->ext_gbuf ? c->ext_gbuf : c->d_gbuf;
}
inline int image_rows(const rm_ctx* c) {
  if (!c->subs.empty() || comm_root(c)) return c->cfg.height;
  return c->rows;
}
inline bool full_frame(const rm_ctx* c) { return c->cfg.nshards <= 1 || !c->subs.empty() || comm_root(c); }
// Bytes per pixel of the context's RGBA8 shard images (rm_config.shard_format).
inline size_t bpp8(const rm_ctx* c) { return c->rgb3 ? 3 : 4; }
// Shard 0's rows per round (rm_config.rank0_rows; 0 = row_block, rm_shard.hpp).
inline int row_block0(const rm_ctx* c) { return c->cfg.rank0_rows > 0 ? c->cfg.rank0_rows : c->cfg.row_block; }
inline bool has_comm(const rm_ctx* c) { return c->comm || (!c->subs.empty() && c->subs[0]->comm); }

// The caller's current device, restored at the end of a scope that visits
// others (a multi-GPU context's waits and teardown).
struct KeepDevice {
  int dev = 0;
  const bool have = hipGetDevice(&dev) == hipSuccess;
  KeepDevice() = default;
  KeepDevice(const KeepDevice&) = delete;
  ~KeepDevice() {
    if (have) (void)hipSetDevice(dev);
  }
};

// ---- rm_api.hip: context and dispatch --------------------------------------------------
int set_device(rm_ctx* c);
int check_uniforms(rm_ctx* c, const rm_uniforms& u);
// The end of a failed rm_create: c's error becomes the creation error, c is freed.
int create_fail(rm_ctx* c, int code);
rmd::Frame make_frame(const rm_ctx* c);
RenderKernel pick_kernel(const rm_ctx* c, const rmd::Frame& F);
const SceneKernels& scene_kernels(const rm_ctx* c);
// One frame, with or without counters (gbuf: the G-buffer image of a k.gbuf
// kernel); the frames B.f[0..n) of one RenderKernel.
hipError_t launch(const RenderKernel& k, const rmd::Frame& F, bool counters, hipStream_t s, void* gbuf = nullptr);
hipError_t launch(const RenderKernel& k, const rmd::FrameBatch& B, int n, hipStream_t s);
// The bracket of a timed launch (rm_enable_timing; nothing with timing off): begin records
// the first event of the context's next pair on its stream, end the second, and only end
// claims the pair, with the frames the launch rendered.  A call that fails in between
// leaves the pool as it found it.  Brackets do not nest on one context.
struct Timed {
  bool on = false;
  int begin(rm_ctx* c);
  int end(rm_ctx* c, int frames = 1);
};
int order_after_batch(rm_ctx* c);
int render_launch(rm_ctx* c);
int phase(rm_ctx* c, int k, hipStream_t st = nullptr);
int ensure_ring(rm_ctx* c, int n, int rows);
int launch_batch(rm_ctx* c, const rm_uniforms* u, int n, uint8_t* const* out8, float* const* out32);
// Synchronous readback of a [image_rows][width] device image of bpp bytes per pixel.
int read_image(rm_ctx* c, const void* dev, size_t bpp, void* dst, size_t row_pitch, int flip_y,
               bool packed3 = false);

// ---- rm_api_comm.hip: RCCL-gathered frames -----------------------------------------------
long default_comm_timeout_ms();
int comm_dead(rm_ctx* c);
int comm_wait(rm_ctx* c);
int create_multi(rm_ctx** out, const rm_config* cfg);
void comm_teardown(rm_ctx* c);
int comm_gather(rm_ctx* c);
int comm_assemble(rm_ctx* c);
int multi_frame(rm_ctx* c, bool graph);
int comm_batch(rm_ctx* c, const rm_uniforms* u, int n);

// ---- rm_api_query.hip: what the ray queries, the field queries and the mesh extraction share ----
// The query's frame constants: a dispatch's, without the two facts about a frame's primary rays.
rmd::Frame query_frame(const rm_ctx* c);
// RM_ERR_STATE on a multi-device context; `who` names the family in the message.
int refuse_multi(rm_ctx* c, const char* who);
// The check of a grid descriptor (not null): every dim in 0..2^24, at most 2^31 - 1 points.
// *total: the grid's points.  `who` starts the messages.
int grid_points(rm_ctx* c, const char* who, const rm_sdf_grid_desc* g, int64_t* total);
// The grid kernels' arguments for a grid of dims >= 1 and device outputs (4-byte aligned, one
// of them possibly null): the lane mapping is chosen from nx and the outputs' alignment.
rmd::SdfGridArgs sdf_grid_args(const rm_sdf_grid_desc* g, void* dist, void* ids);
// b of at least `need` bytes, replaced when too small (hipFree waits for the device, so
// nothing pending uses the old one); `what` names it in RM_ERR_NOMEM.
int ensure(rm_ctx* c, DevBuf& b, size_t need, const char* what);

// ---- rm_api_adaptive.hip -----------------------------------------------------------------
// RM_ERR_STATE, naming `call`, for the contexts the adaptive dispatches and rm_dispatch_pattern
// do not serve: multi-device, communicator, sharded, counting, graph-replay and (unless
// gbuf_ok) G-buffer contexts.
int refuse_extension(rm_ctx* c, const char* call, bool gbuf_ok = false);

// ---- rm_api_pattern.hip -------------------------------------------------------------------
// The device table of the valid pattern p (c->pat_uv, c->pat_lo / pat_hi): the context's when p
// is the last call's, whichever of rm_dispatch_pattern and the pattern refinements made it, else
// uploaded on the context's stream.  `call` starts the messages.
int ensure_table(rm_ctx* c, const rm_sample_pattern& p, const char* call);

// ---- rm_api_graph.hip: hipGraph replay -----------------------------------------------------
void graph_release(rm_ctx* c);
int graph_frame(rm_ctx* c);

}  // namespace rm
