// rm_api.hip — librm's C-ABI: context, uniforms, dispatch, readback, timing.
//
// Replaces the reference's GL program + dispatch (see include/rm_api.h for the
// call-by-call mapping).  There is no CPU backend: without a HIP device
// rm_create fails with RM_ERR_NO_DEVICE — librm never falls back to the CPU.
//
// The context itself and what this file shares with rm_api_comm.hip (RCCL-gathered
// frames) and rm_api_graph.hip (hipGraph replay) are in rm_ctx.hpp; the per-frame
// float math is rm_frame_math.hip.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <utility>
#include <vector>

#include "rm_ctx.hpp"
#include "rm_frame_math.hpp"

using namespace rm;

namespace {
thread_local std::string g_create_error;
void free_all(rm_ctx* c);
}  // namespace

int rm::fail(rm_ctx* c, int code, const std::string& msg) {
  if (c)
    c->err = msg;
  else
    g_create_error = msg;
  return code;
}

int rm::hip_fail(rm_ctx* c, hipError_t e, const char* what) {
  return fail(c, RM_ERR_HIP, std::string(what) + ": " + hipGetErrorString(e));
}

int rm::set_device(rm_ctx* c) {
  RM_HIP(c, hipSetDevice(c->device));
  return RM_OK;
}

int rm::create_fail(rm_ctx* c, int code) {
  g_create_error = c->err;
  free_all(c);
  delete c;
  return code;
}

namespace {

// The stream wait of every synchronising call: bounded on a communicator context.
int stream_wait(rm_ctx* c) {
  if (c->comm_failed) return comm_dead(c);
  if (has_comm(c)) return comm_wait(c);
  RM_HIP(c, hipStreamSynchronize(c->stream));
  return RM_OK;
}

}  // namespace

rmd::Frame rm::make_frame(const rm_ctx* c) {
  const rm_uniforms& u = c->u;
  rmd::Frame F;
  std::memset(&F, 0, sizeof F);
  std::memcpy(F.cam_pos, u.camera.pos, sizeof F.cam_pos);
  std::memcpy(F.cam_dir, u.camera.dir, sizeof F.cam_dir);
  std::memcpy(F.cam_y, u.camera.yAxis, sizeof F.cam_y);
  std::memcpy(F.cam_x, u.camera.xAxis, sizeof F.cam_x);
  std::memcpy(F.lpos, u.light.position, sizeof F.lpos);
  std::memcpy(F.lamb, u.light.ambient, sizeof F.lamb);
  std::memcpy(F.ldif, u.light.diffuse, sizeof F.ldif);
  std::memcpy(F.lspec, u.light.specular, sizeof F.lspec);
  F.lconst = u.light.constant;
  F.llin = u.light.linear;
  F.lquad = u.light.quadratic;
  // Uniform-only subexpressions, evaluated once on the host with the same
  // float operations the GLSL performs per call (glsl:70, 117, 185/236).
  F.blend = std::sin(u.iTime) / 2.0f + 0.5f;
  F.omblend = 1.0f - F.blend;
  F.k = (u.shadow_mode == RM_SHADOW_HARD) ? INFINITY : 2.0f;
  // the soft-shadow exit's ratio bound (rm_scene.hpp shadow_exit_init), the
  // device's former per-call expression in the same float operations
  F.shc = (F.k == INFINITY) ? 0.0f : (1.0f + 0x1p-9f) / F.k * (1.0f + 0x1p-12f);
  F.persp = 45.0f * static_cast<float>(0.01745329251994329576923690768489);
  // the shadow exit's light-in-ball test (rm_scene.hpp), once per frame
  F.light_ball = rmd::light_in_ball(F.lpos) ? 1 : 0;
  F.uvx = c->d_uv;
  F.uvy = c->d_uv + (size_t)5 * c->cfg.width;
  F.uv_exact = c->uv_exact ? 1 : 0;
  F.unit_rd = unit_rd_check(u.camera, F.persp, c->uv_lo, c->uv_hi) ? 1 : 0;
  const float uv_ox[4] = {0.25f, 0.75f, 0.25f, 0.75f}, uv_oy[4] = {0.25f, 0.25f, 0.75f, 0.75f};
  for (int a = 0; a < 2; ++a) {
    const float n = (float)(a ? c->cfg.height : c->cfg.width);
    F.uv_dims[a] = n;
    F.uv_rcp[a] = 1.0f / n;
    for (int k = 0; k < 4; ++k) F.uv_off[a][k] = (a ? uv_oy[k] : uv_ox[k]) / n;
  }
  F.bounces = u.bounceVar;
  F.aa = u.AA ? 1 : 0;
  F.width = c->cfg.width;
  F.height = c->cfg.height;
  F.row_block = c->cfg.row_block;
  F.row_block0 = row_block0(c);
  F.shard = c->cfg.shard;
  F.nshards = c->cfg.nshards > 1 ? c->cfg.nshards : 1;
  F.rows = c->rows;
  F.rgba8 = render_dst(c);
  F.rgb3 = c->rgb3 ? 1 : 0;
  F.rgba32f = render_dst32(c);
  F.sdf_counts = c->cfg.counters ? c->d_counts : nullptr;
  F.counters = c->cfg.counters ? c->d_counters : nullptr;
  if (c->nprims) table_prep_host(c->scene_words.data(), c->nprims, F.cam_pos, F.blend, F.omblend, F.prepv);
  else prep_host(F.cam_pos, F.blend, F.omblend, F.prepv);
  F.scene = c->nprims ? reinterpret_cast<const float*>(c->d_scene) : nullptr;
  F.nprims = c->nprims;
  rm::pixel_grid(F.width, F.rows, F.aa != 0, &F.grid_x, &F.grid_y);
  return F;
}

// The specialised table kernels for frame F, or null: they take sqrt(x) - R in
// the fast exact form for march and normal points (rm_table.hip sqrt_sub), which
// needs every such point within 2^53 of every entry.  Entries lie within 10^15
// of the origin (rm::exit_bounds), a march moves at most nmax tmax = 2.05e5
// along a unit ray and five bounces add 1.3e5 more, so a camera within 10^15
// of the origin keeps them there; a frame whose camera is farther out (or not
// finite) renders with the generic kernel.
//
// The light position is not bounded here: shadow rays (rd = light.position - pos,
// unnormalised, glsl:184, 235) march with the full-range form (TLazy::dist ->
// prim_dist<false>, rm_table.hip), so however far the light is, no shadow point
// reaches the short form (tests/test_gpu_scene.py far-light case).
static const rm::JitTable* frame_jit(const rm_ctx* c, const rmd::Frame& F) {
  if (!c->jit) return nullptr;
  for (int i = 0; i < 3; ++i)
    if (!(std::fabs(F.cam_pos[i]) <= 1e15f)) return nullptr;
  return c->jit;
}

// The kernel that renders frame F of the context (rm_ctx.hpp RenderKernel): the
// one place that decides it, for a dispatch, a run of a batch and a graph.
RenderKernel rm::pick_kernel(const rm_ctx* c, const rmd::Frame& F) {
  RenderKernel k;
  k.aa = F.aa;
  k.table = c->nprims != 0;
  k.gbuf = has_gbuf(c);
  if (k.gbuf) return k;
  if (!k.table || (k.jit = frame_jit(c, F))) return k;
  // the generic table kernel's instance (rm_table.hip launch_table): the lazy
  // slots it holds (EX_NSLOTS of the compiled words fit) and its production
  // march (table_shape: 1 the built-in shape of reference-shaped tables, 2 the
  // block shape of any plane-bounded table, 0 TLazy)
  const float* ex = reinterpret_cast<const float*>(c->scene_words.data()) + (size_t)c->nprims * rm::TABLE_WORDS;
  k.nslots = (int)ex[rm::EX_NSLOTS] <= rm::TABLE_FEW_SLOTS ? rm::TABLE_FEW_SLOTS : rm::EX_MAX_SLOTS;
  k.shape = rm::table_shape(c->scene_words.data(), c->nprims);
  return k;
}

// The same decision for the kernels that are not frame kernels: the built-in
// scene's, or for a table always the generic code (its specialised kernels render
// frames only).
const SceneKernels& rm::scene_kernels(const rm_ctx* c) {
  static const SceneKernels builtin{launch_trace, launch_sdf_points, launch_sdf_grid, launch_adapt_refine,
                                    launch_pattern, launch_adapt_refine_pattern, launch_accum};
  static const SceneKernels table{launch_table_trace, launch_table_sdf_points, launch_table_sdf_grid,
                                  launch_table_adapt_refine, launch_table_pattern,
                                  launch_table_adapt_refine_pattern, launch_table_accum};
  return c->nprims ? table : builtin;
}

hipError_t rm::launch(const RenderKernel& k, const rmd::Frame& F, bool counters, hipStream_t s, void* gbuf) {
  if (k.gbuf) {
    // (rm_create refuses counters with the bit; a missing image is an error, not a plain frame)
    if (!gbuf || counters) return hipErrorInvalidValue;
    return k.table ? rm::launch_table_gbuf(F, gbuf, s) : rm::launch_gbuf(F, gbuf, s);
  }
  if (!k.table) return rm::launch_pixel(F, counters, s);
  if (k.jit) return rm::launch_table_jit(k.jit, F, counters, s);
  return rm::launch_table(F, counters, s, k.nslots, k.shape);
}

hipError_t rm::launch(const RenderKernel& k, const rmd::FrameBatch& B, int n, hipStream_t s) {
  if (!k.table) return rm::launch_frames(B, n, s);
  if (k.jit) return rm::launch_table_jit_frames(k.jit, B, n, s);
  return rm::launch_table_frames(B, n, s, k.nslots, k.shape);
}

namespace {

void free_all(rm_ctx* c) {
  graph_release(c);
  comm_teardown(c);
  for (rm_ctx* s : c->subs) rm_destroy(s);
  c->subs.clear();
  c->comm = nullptr;
  for (void** p : {(void**)&c->d_gathered, (void**)&c->d_frame, (void**)&c->d_gathered32, (void**)&c->d_frame32,
                   (void**)&c->d_rgba8, (void**)&c->d_rgba32f, &c->d_gbuf, (void**)&c->d_counts, (void**)&c->d_counters,
                   (void**)&c->d_uv, (void**)&c->d_scene, (void**)&c->d_aa_mask, (void**)&c->d_aa_list,
                   (void**)&c->d_aa_counts, (void**)&c->d_aa_offsets, (void**)&c->d_aa_total,
                   (void**)&c->d_accum}) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
  for (DevBuf* b : {&c->stage_in, &c->stage_out, &c->mesh_vol, &c->mesh_waves, &c->mesh_idx, &c->mesh_attr,
                    &c->pat_uv}) {
    if (b->p) (void)hipFree(b->p);
    *b = DevBuf();
  }
  c->aa_dispatched = false;
  c->accum_n = 0;
  c->pat.n = 0;
  if (c->pat_ev) {
    if (c->pat_ev_pending) (void)hipEventSynchronize(c->pat_ev);
    (void)hipEventDestroy(c->pat_ev);
  }
  c->pat_ev = nullptr;
  c->pat_ev_pending = false;
  if (c->pat_host) (void)hipHostFree(c->pat_host);
  c->pat_host = nullptr;
  if (c->gstream) (void)hipStreamSynchronize(c->gstream);
  for (uint8_t* p : c->ring8) (void)hipFree(p);
  for (float* p : c->ring32) (void)hipFree(p);
  c->ring8.clear();
  c->ring32.clear();
  for (auto& b : c->bslot) {
    if (b.send8) (void)hipFree(b.send8);
    if (b.send32) (void)hipFree(b.send32);
    if (b.rendered) (void)hipEventDestroy(b.rendered);
    if (b.freed) (void)hipEventDestroy(b.freed);
    b = rm_ctx::BatchSlot();
  }
  if (c->gdone) (void)hipEventDestroy(c->gdone);
  c->gdone = nullptr;
  if (c->out_ev) (void)hipEventDestroy(c->out_ev);
  c->out_ev = nullptr;
  if (c->gstream) (void)hipStreamDestroy(c->gstream);
  c->gstream = nullptr;
  for (auto& p : c->ev_pool) {
    (void)hipEventDestroy(p.first);
    (void)hipEventDestroy(p.second);
  }
  c->ev_pool.clear();
  c->ev_frames.clear();
  for (hipEvent_t& e : c->ph) {
    if (e) (void)hipEventDestroy(e);
    e = nullptr;
  }
  if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
  c->stream = nullptr;
}

}  // namespace

int rm::check_uniforms(rm_ctx* c, const rm_uniforms& u) {
  if (u.bounceVar < 0 || u.bounceVar > 5)
    return fail(c, RM_ERR_INVALID, "bounceVar must be in 0..5 (main.cpp:199-204)");
  if (u.shadow_mode != RM_SHADOW_SOFT && u.shadow_mode != RM_SHADOW_HARD)
    return fail(c, RM_ERR_INVALID, "shadow_mode must be RM_SHADOW_SOFT or RM_SHADOW_HARD");
  return RM_OK;
}

#ifdef RM_STATS
namespace rm {
hipError_t debug_stats(unsigned long long* out, bool clear);
}
#endif

extern "C" {

#ifdef RM_STATS
/* Diagnostic builds only (-DRM_STATS, tools/build_variant.sh): the 64 wave /
 * lane counters of rm_scene.hpp's RM_STAT points, then cleared. */
int rm_debug_stats(unsigned long long *out64) {
  return rm::debug_stats(out64, true) == hipSuccess ? 0 : -1;
}
#endif

/* Diagnostic read for the tests (not declared in rm_api.h, like rm_debug_stats;
 * rmarch binds it on first use, Renderer.debug_frame_flags): the wave-uniform
 * branches a frame of the context's current uniforms takes, as make_frame sets
 * them: out2[0] = Frame::unit_rd (cast_ray's lean form, the unit march),
 * out2[1] = Frame::light_ball (the shadow exit without the ball's bound). */
int rm_debug_frame_flags(const rm_ctx* c, int32_t* out2) {
  if (!c || !out2) return RM_ERR_INVALID;
  const rmd::Frame F = rm::make_frame(c);
  out2[0] = F.unit_rd;
  out2[1] = F.light_ball;
  return RM_OK;
}

const char* rm_last_error(const rm_ctx* ctx) {
  return ctx ? ctx->err.c_str() : g_create_error.c_str();
}

int rm_device_count(int* count) {
  if (!count) return RM_ERR_INVALID;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  *count = (e == hipSuccess) ? n : 0;
  return RM_OK;
}

int rm_config_init(rm_config* cfg, int32_t width, int32_t height) {
  if (!cfg) return RM_ERR_INVALID;
  std::memset(cfg, 0, sizeof *cfg);
  cfg->struct_size = (uint32_t)sizeof(rm_config);
  cfg->magic = RM_CONFIG_MAGIC;
  cfg->width = width;
  cfg->height = height;
  cfg->device = -1;
  cfg->outputs = RM_OUT_RGBA8;
  cfg->nshards = 1;
  return RM_OK;
}

int rm_create(rm_ctx** out, const rm_config* cfg) {
  if (!out || !cfg) return fail(nullptr, RM_ERR_INVALID, "rm_create: null argument");
  *out = nullptr;
  // A host built against an older rm_api.h passes a smaller struct without this
  // field (its first word is the width): refuse it rather than read past its end.
  if (cfg->struct_size != (uint32_t)sizeof(rm_config) || cfg->magic != RM_CONFIG_MAGIC)
    return fail(nullptr, RM_ERR_INVALID,
                "rm_create: rm_config.struct_size must be sizeof(rm_config) = " +
                    std::to_string(sizeof(rm_config)) + " and rm_config.magic RM_CONFIG_MAGIC (rm_config_init; "
                    "API version " + std::to_string(RM_API_VERSION) + ")");
  if (cfg->width <= 0 || cfg->height <= 0 || cfg->width > 65536 || cfg->height > 65536)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: width/height must be in 1..65536");
  if (cfg->ngpus < 0 || cfg->ngpus > 64)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: ngpus must be in 0..64");
  if (cfg->shard_format < RM_SHARD_AUTO || cfg->shard_format > RM_SHARD_RGB8)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: shard_format must be RM_SHARD_AUTO, _RGBA8 or _RGB8");
  if (cfg->ngpus >= 1) {
    if (cfg->kernel < RM_KERNEL_AUTO || cfg->kernel > RM_KERNEL_PIXEL)
      return fail(nullptr, RM_ERR_INVALID, "rm_create: unknown kernel variant");
    return create_multi(out, cfg);
  }
  if (cfg->outputs & ~(RM_OUT_RGBA8 | RM_OUT_RGBA32F | RM_OUT_GBUFFER))
    return fail(nullptr, RM_ERR_INVALID, "rm_create: unknown output bits");
  if ((cfg->outputs & RM_OUT_GBUFFER) && cfg->counters)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: RM_OUT_GBUFFER is not available with counters");
  if (cfg->kernel < RM_KERNEL_AUTO || cfg->kernel > RM_KERNEL_PIXEL)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: unknown kernel variant");
  if (cfg->nshards > 1 && rm_shard_rows(cfg->height, cfg->row_block, cfg->rank0_rows, cfg->nshards, cfg->shard,
                                         nullptr, nullptr) != RM_OK)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: bad row_block/rank0_rows/shard/nshards (rm_shard_rows)");
  if (cfg->rank0_rows < 0) return fail(nullptr, RM_ERR_INVALID, "rm_create: rank0_rows must be >= 0");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, RM_ERR_NO_DEVICE,
                "rm_create: no HIP device (librm has no CPU fallback; use a GPU box)");
  rm_ctx* c = new (std::nothrow) rm_ctx();
  if (!c) return fail(nullptr, RM_ERR_NOMEM, "rm_create: out of host memory");
  c->cfg = *cfg;
  c->cfg.devices = nullptr;  // not kept: the caller owns the array
  if (c->cfg.outputs == 0) c->cfg.outputs = RM_OUT_RGBA8;
  if (c->cfg.nshards <= 1) {
    c->cfg.nshards = 1;
    c->cfg.shard = 0;
    if (c->cfg.row_block <= 0) c->cfg.row_block = 1;
  }
  // the grid of adaptive supersampling's refinement (rm_api_adaptive.hip), when set
  if (const char* v = std::getenv("RM_AA_REFINE_WAVES")) {
    const long n = std::strtol(v, nullptr, 10);
    if (n >= 1 && n <= 65535) c->aa_waves_env = (int)n;
  }
  c->rgb3 = c->cfg.nshards > 1 && c->cfg.shard_format == RM_SHARD_RGB8 && (c->cfg.outputs & RM_OUT_RGBA8);
  if (cfg->device >= 0) {
    c->device = cfg->device;
  } else {
    if (hipGetDevice(&c->device) != hipSuccess) c->device = 0;
  }
  if (c->device >= ndev) {
    delete c;
    return fail(nullptr, RM_ERR_INVALID, "rm_create: device ordinal out of range");
  }
  int rc = RM_OK;
  auto bail = [&](int code) { return create_fail(c, code); };
  if ((rc = set_device(c)) != RM_OK) return bail(rc);
  rm_shard_rows(c->cfg.height, c->cfg.row_block, c->cfg.rank0_rows, c->cfg.nshards, c->cfg.shard, nullptr,
                &c->rows);
  const size_t npx = (size_t)c->rows * (size_t)c->cfg.width;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) return bail(hip_fail(c, e, "hipStreamCreate"));
  c->own_stream = true;
  if (c->cfg.outputs & RM_OUT_RGBA8) {
    if ((e = hipMalloc(&c->d_rgba8, npx * 4)) != hipSuccess) return bail(hip_fail(c, e, "hipMalloc rgba8"));
    // on the context's own (non-blocking) stream: a NULL-stream memset is not
    // ordered before kernels on it and could land after the first dispatch
    if ((e = hipMemsetAsync(c->d_rgba8, 0, npx * 4, c->stream)) != hipSuccess)
      return bail(hip_fail(c, e, "hipMemset"));
  }
  if (c->cfg.outputs & RM_OUT_RGBA32F) {
    if ((e = hipMalloc(&c->d_rgba32f, npx * 16)) != hipSuccess) return bail(hip_fail(c, e, "hipMalloc rgba32f"));
    if ((e = hipMemsetAsync(c->d_rgba32f, 0, npx * 16, c->stream)) != hipSuccess)
      return bail(hip_fail(c, e, "hipMemset"));
  }
  if (has_gbuf(c)) {
    if ((e = hipMalloc(&c->d_gbuf, npx * sizeof(rm_gbuffer_px))) != hipSuccess)
      return bail(hip_fail(c, e, "hipMalloc gbuffer"));
    if ((e = hipMemsetAsync(c->d_gbuf, 0, npx * sizeof(rm_gbuffer_px), c->stream)) != hipSuccess)
      return bail(hip_fail(c, e, "hipMemset"));
  }
  if (c->cfg.counters) {
    if ((e = hipMalloc(&c->d_counts, npx * 4)) != hipSuccess) return bail(hip_fail(c, e, "hipMalloc counts"));
    if ((e = hipMalloc(&c->d_counters, 8 * sizeof(unsigned long long))) != hipSuccess)
      return bail(hip_fail(c, e, "hipMalloc counters"));
  }
  {
    const rm::UvTable t = rm::uv_table(c->cfg.width, c->cfg.height);
    for (int a = 0; a < 2; ++a) {
      c->uv_lo[a] = t.lo[a];
      c->uv_hi[a] = t.hi[a];
    }
    c->uv_exact = t.exact;
    if ((e = hipMalloc(&c->d_uv, t.uv.size() * sizeof(float))) != hipSuccess ||
        (e = hipMemcpy(c->d_uv, t.uv.data(), t.uv.size() * sizeof(float), hipMemcpyHostToDevice)) != hipSuccess)
      return bail(hip_fail(c, e, "uv table"));
  }
  if ((e = hipStreamSynchronize(c->stream)) != hipSuccess) return bail(hip_fail(c, e, "hipStreamSynchronize"));
  rm_default_uniforms(&c->u);
  c->comm_timeout_ms = default_comm_timeout_ms();
  *out = c;
  return RM_OK;
}

void rm_destroy(rm_ctx* ctx) {
  if (!ctx) return;
  (void)hipSetDevice(ctx->device);
  // a collective that never completes must not hang the teardown: the bounded
  // wait aborts the communicator on its deadline, and the aborted gather quits
  if (has_comm(ctx) && !ctx->comm_failed && !ctx->group_member) (void)comm_wait(ctx);
  if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
  if (ctx->gstream) (void)hipStreamSynchronize(ctx->gstream);
  free_all(ctx);
  delete ctx;
}

// ---- uniforms -------------------------------------------------------------------
static int set_floats(rm_ctx* c, const char* name, const float* v, int n) {
  if (!c || !name) return RM_ERR_INVALID;
  int m = 0;
  float* dst = rm::uniform_floats(&c->u, name, &m);
  if (!dst) return RM_WARN_UNKNOWN_UNIFORM;
  // glUniform with a mismatched component count is a GL error that leaves the
  // uniform unchanged; report it instead of writing.
  if (m != n) return fail(c, RM_ERR_INVALID, std::string("uniform '") + name + "' has " +
                                                 std::to_string(m) + " components");
  std::memcpy(dst, v, sizeof(float) * n);
  return RM_OK;
}

static int set_int(rm_ctx* c, const char* name, int32_t v) {
  if (!c || !name) return RM_ERR_INVALID;
  int32_t* dst = rm::uniform_ints(&c->u, name);
  if (!dst) {
    int m = 0;
    if (rm::uniform_floats(&c->u, name, &m))
      return fail(c, RM_ERR_INVALID, std::string("uniform '") + name + "' is a float");
    return RM_WARN_UNKNOWN_UNIFORM;
  }
  rm_uniforms t = c->u;
  *rm::uniform_ints(&t, name) = v;
  int rc = check_uniforms(c, t);
  if (rc != RM_OK) return rc;
  *dst = v;
  return RM_OK;
}

int rm_set_bool(rm_ctx* c, const char* name, int value) { return set_int(c, name, value ? 1 : 0); }
int rm_set_int(rm_ctx* c, const char* name, int32_t value) { return set_int(c, name, value); }
int rm_set_uint(rm_ctx* c, const char* name, const uint32_t* value) {
  if (!value) return RM_ERR_INVALID;
  return set_int(c, name, (int32_t)*value);
}
int rm_set_float(rm_ctx* c, const char* name, float value) { return set_floats(c, name, &value, 1); }
int rm_set_vec2(rm_ctx* c, const char* name, float x, float y) {
  const float v[2] = {x, y};
  return set_floats(c, name, v, 2);
}
int rm_set_vec3(rm_ctx* c, const char* name, float x, float y, float z) {
  const float v[3] = {x, y, z};
  return set_floats(c, name, v, 3);
}
int rm_set_vec4(rm_ctx* c, const char* name, float x, float y, float z, float w) {
  const float v[4] = {x, y, z, w};
  return set_floats(c, name, v, 4);
}

int rm_set_uniforms(rm_ctx* c, const rm_uniforms* u) {
  if (!c || !u) return RM_ERR_INVALID;
  int rc = check_uniforms(c, *u);
  if (rc != RM_OK) return rc;
  c->u = *u;
  return RM_OK;
}

int rm_get_uniforms(const rm_ctx* c, rm_uniforms* u) {
  if (!c || !u) return RM_ERR_INVALID;
  *u = c->u;
  return RM_OK;
}

}  // extern "C"

// ---- dispatch ---------------------------------------------------------------------

// The context's next event pair (rm_ctx.hpp Timed), created on first use; the
// pairs below ev_used are claimed and wait for rm_kernel_time_ms.
int rm::Timed::begin(rm_ctx* c) {
  if (!c->timing) return RM_OK;
  if (c->ev_used == c->ev_pool.size()) {
    std::pair<hipEvent_t, hipEvent_t> p;
    RM_HIP(c, hipEventCreate(&p.first));
    RM_HIP(c, hipEventCreate(&p.second));
    c->ev_pool.push_back(p);
    c->ev_frames.push_back(1);
  }
  RM_HIP(c, hipEventRecord(c->ev_pool[c->ev_used].first, c->stream));
  on = true;
  return RM_OK;
}

int rm::Timed::end(rm_ctx* c, int frames) {
  if (!on) return RM_OK;
  RM_HIP(c, hipEventRecord(c->ev_pool[c->ev_used].second, c->stream));
  c->ev_frames[c->ev_used++] = frames;
  return RM_OK;
}

// A plain dispatch after a batch on a communicator context: its render may
// write the image the batch's assembly writes, and its gather must follow the
// batch's on the communicator, so the context's stream waits for the gather
// stream's last batch (rm_dispatch_frames).
int rm::order_after_batch(rm_ctx* c) {
  c->batch_n = 1;
  if (!c->gdone_pending) return RM_OK;
  RM_HIP(c, hipStreamWaitEvent(c->stream, c->gdone, 0));
  c->gdone_pending = false;
  return RM_OK;
}

// The render kernel of one frame on the context's stream (== glDispatchCompute).
int rm::render_launch(rm_ctx* c) {
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  if (c->cfg.counters) {
    RM_HIP(c, hipMemsetAsync(c->d_counters, 0, 8 * sizeof(unsigned long long), c->stream));
  }
  rmd::Frame F = make_frame(c);
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  const hipError_t e = launch(pick_kernel(c, F), F, c->cfg.counters != 0, c->stream, image_gbuf(c));
  if (e != hipSuccess) return hip_fail(c, e, "kernel launch");
  if ((rc = t.end(c)) != RM_OK) return rc;
  c->dispatched = true;
  return RM_OK;
}

// Phase k of the frame (0 render start, 1 render end, 2 gather end, 3 assembly
// end) on the context's stream, when timing is on (rm_frame_phases).
int rm::phase(rm_ctx* c, int k, hipStream_t st) {
  if (!c->timing) return RM_OK;
  if (!c->ph[k]) RM_HIP(c, hipEventCreate(&c->ph[k]));
  RM_HIP(c, hipEventRecord(c->ph[k], st ? st : c->stream));
  return RM_OK;
}

// ---- frame batches (rm_dispatch_frames) ------------------------------------------
// One launch renders n frames (grid.z = frame, rm_kernels.hip k_*_frames), so
// the waves of frame k + 1 fill the SIMDs that frame k's longest waves leave
// idle.  Frames 0..n-2 go to a ring of images the context keeps, frame n-1 to
// the context's image, so afterwards the context reads as after n rm_dispatch
// calls.  (A communicator context's batch: rm_api_comm.hip comm_batch.)

// Images for frames 0..n-2 of a batch, `rows` x width, per enabled format.
int rm::ensure_ring(rm_ctx* c, int n, int rows) {
  const size_t px = (size_t)rows * (size_t)c->cfg.width;
  while ((c->cfg.outputs & RM_OUT_RGBA8) && (int)c->ring8.size() < n - 1) {
    uint8_t* p = nullptr;
    RM_HIP(c, hipMalloc(&p, px * 4));
    c->ring8.push_back(p);
  }
  while ((c->cfg.outputs & RM_OUT_RGBA32F) && (int)c->ring32.size() < n - 1) {
    float* p = nullptr;
    RM_HIP(c, hipMalloc(&p, px * 16));
    c->ring32.push_back(p);
  }
  return RM_OK;
}

// The frame constants of frames[0..n) with their output pointers, launched in
// runs of one kernel (pick_kernel: one AA setting, and for a runtime scene table
// one of its kernels, the specialised ones or the generic one for a frame
// frame_jit refuses); one grid per run.  out8[k] / out32[k]: frame k's
// destinations.
int rm::launch_batch(rm_ctx* c, const rm_uniforms* u, int n, uint8_t* const* out8, float* const* out32) {
  static thread_local rmd::FrameBatch B;  // 11.9 KB of kernel arguments
  int m = 0;
  RenderKernel run;  // the kernel of the run B.f[0..m)
  auto flush = [&]() -> int {
    if (m == 0) return RM_OK;
    const hipError_t e = launch(run, B, m, c->stream);
    m = 0;
    if (e != hipSuccess) return hip_fail(c, e, "batch launch");
    return RM_OK;
  };
  int rc = RM_OK;
  for (int k = 0; k < n; ++k) {
    c->u = u[k];
    rmd::Frame F = make_frame(c);
    F.rgba8 = out8[k];
    F.rgba32f = out32[k];
    F.sdf_counts = nullptr;
    F.counters = nullptr;
    const RenderKernel kern = pick_kernel(c, F);
    if (m > 0 && !(kern == run) && (rc = flush()) != RM_OK) return rc;
    run = kern;
    B.f[m++] = F;
  }
  return flush();
}

static int plain_batch(rm_ctx* c, const rm_uniforms* u, int n) {
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  if ((rc = ensure_ring(c, n, c->rows)) != RM_OK) return rc;
  uint8_t* const dst8 = render_dst(c);
  float* const dst32 = render_dst32(c);
  uint8_t* out8[RM_MAX_BATCH];
  float* out32[RM_MAX_BATCH];
  for (int k = 0; k < n; ++k) {
    out8[k] = dst8 ? (k < n - 1 ? c->ring8[k] : dst8) : nullptr;
    out32[k] = dst32 ? (k < n - 1 ? c->ring32[k] : dst32) : nullptr;
  }
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  if ((rc = phase(c, 0)) != RM_OK) return rc;
  if ((rc = launch_batch(c, u, n, out8, out32)) != RM_OK) return rc;
  if ((rc = phase(c, 1)) != RM_OK) return rc;
  if ((rc = t.end(c, n)) != RM_OK) return rc;
  if (c->timing) {
    c->ph_recorded = true;
    c->ph_comm = false;
  }
  c->batch_n = n;
  c->dispatched = true;
  return RM_OK;
}

extern "C" {

int rm_dispatch(rm_ctx* c) {
  if (!c) return RM_ERR_INVALID;
  if (!c->subs.empty()) return multi_frame(c, false);
  if (c->comm_failed) return comm_dead(c);
  int rc;
  if ((rc = phase(c, 0)) != RM_OK) return rc;
  if ((rc = render_launch(c)) != RM_OK) return rc;
  if ((rc = phase(c, 1)) != RM_OK) return rc;
  // one rank of an RCCL-gathered frame: gather on rank 0, which assembles
  const bool comm = c->comm && !c->group_member;
  if (comm) {
    if ((rc = comm_gather(c)) != RM_OK) return rc;
    if ((rc = phase(c, 2)) != RM_OK) return rc;
    if ((rc = comm_assemble(c)) != RM_OK) return rc;
    if ((rc = phase(c, 3)) != RM_OK) return rc;
  }
  if (c->timing) {
    c->ph_recorded = true;
    c->ph_comm = comm;
  }
  return RM_OK;
}

int rm_dispatch_frames(rm_ctx* c, const rm_uniforms* u, int32_t n) {
  if (!c || !u) return RM_ERR_INVALID;
  if (n < 1 || n > RM_MAX_BATCH)
    return fail(c, RM_ERR_INVALID, "rm_dispatch_frames: n must be in 1.." + std::to_string(RM_MAX_BATCH));
  for (int k = 0; k < n; ++k) {
    const int rc = check_uniforms(c, u[k]);
    if (rc != RM_OK) return rc;
  }
  if (c->cfg.counters) return fail(c, RM_ERR_STATE, "rm_dispatch_frames: not available with counters");
  if (has_gbuf(c)) return fail(c, RM_ERR_STATE, "rm_dispatch_frames: not available on a G-buffer context (RM_OUT_GBUFFER)");
  // launch_batch walks c->u (and every member's) through the frames; a failed
  // batch leaves the uniforms of the last successful dispatch
  const rm_uniforms before = c->u;
  int rc;
  if (has_comm(c) && !c->group_member) rc = comm_batch(c, u, n);
  else rc = plain_batch(c, u, n);
  const rm_uniforms& now = rc == RM_OK ? u[n - 1] : before;
  c->u = now;
  for (rm_ctx* s : c->subs) s->u = now;
  return rc;
}

int rm_synchronize(rm_ctx* c) {
  if (!c) return RM_ERR_INVALID;
  if (c->subs.empty()) {
    const int rc = set_device(c);
    if (rc != RM_OK) return rc;
  }
  return stream_wait(c);
}

}  // extern "C"

// packed3: `dev` is an RGB8 shard image (rows of width x 3 bytes), read back as
// RGBA8 with alpha 255 (rm_config.shard_format).
int rm::read_image(rm_ctx* c, const void* dev, size_t bpp, void* dst, size_t row_pitch, int flip_y, bool packed3) {
  if (!c || !dst) return RM_ERR_INVALID;
  if (!dev) return fail(c, RM_ERR_STATE, "output format not enabled in rm_config.outputs");
  if (!c->dispatched) return fail(c, RM_ERR_STATE, "no dispatch yet");
  if (flip_y && !full_frame(c))
    return fail(c, RM_ERR_INVALID, "flip_y is not defined for a packed shard image");
  if (!c->subs.empty()) {  // the frame is on device 0, behind every device's stream
    const int rc = rm_synchronize(c);
    if (rc != RM_OK) return rc;
    c = c->subs[0];
  }
  const size_t w = (size_t)c->cfg.width * bpp;
  if (row_pitch == 0) row_pitch = w;
  if (row_pitch < w) return fail(c, RM_ERR_INVALID, "row_pitch smaller than a row");
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if ((rc = stream_wait(c)) != RM_OK) return rc;
  const size_t rows = (size_t)image_rows(c);
  if (packed3) {
    const size_t w3 = (size_t)c->cfg.width * 3;
    std::vector<uint8_t> tmp(w3 * rows);
    RM_HIP(c, hipMemcpy(tmp.data(), dev, tmp.size(), hipMemcpyDeviceToHost));
    for (size_t r = 0; r < rows; ++r) {
      const uint8_t* s3 = tmp.data() + r * w3;
      uint8_t* d4 = static_cast<uint8_t*>(dst) + r * row_pitch;
      for (int x = 0; x < c->cfg.width; ++x) {
        d4[4 * x] = s3[3 * x];
        d4[4 * x + 1] = s3[3 * x + 1];
        d4[4 * x + 2] = s3[3 * x + 2];
        d4[4 * x + 3] = 255;
      }
    }
    return RM_OK;  // (a shard image: flip_y was refused above)
  }
  RM_HIP(c, hipMemcpy2D(dst, row_pitch, dev, w, w, rows, hipMemcpyDeviceToHost));
  if (flip_y) {
    // Row 0 of the device image is the bottom row (quad.hpp:9); flip in place
    // so the top row comes first (image-file order).
    std::vector<char> tmp(w);
    char* base = static_cast<char*>(dst);
    for (size_t r = 0; r < rows / 2; ++r) {
      char* a = base + r * row_pitch;
      char* b = base + (rows - 1 - r) * row_pitch;
      std::memcpy(tmp.data(), a, w);
      std::memcpy(a, b, w);
      std::memcpy(b, tmp.data(), w);
    }
  }
  return RM_OK;
}

extern "C" {

int rm_read_rgba8(rm_ctx* c, uint8_t* dst, size_t row_pitch, int flip_y) {
  if (!c) return RM_ERR_INVALID;
  return read_image(c, image_rgba8(c), 4, dst, row_pitch, flip_y, c->rgb3 && !full_frame(c));
}

int rm_read_rgba32f(rm_ctx* c, float* dst, size_t row_pitch, int flip_y) {
  if (!c) return RM_ERR_INVALID;
  return read_image(c, image_rgba32f(c), 16, dst, row_pitch, flip_y);
}

// Frame k of the last batch: the context's image for k = n-1; else rank 0's
// (or a plain context's) ring, or another rank's shard in the batch's slot.
static int read_frame(rm_ctx* c, int32_t k, bool f32, void* dst, size_t row_pitch, int flip_y) {
  if (!c) return RM_ERR_INVALID;
  rm_ctx* t = c->subs.empty() ? c : c->subs[0];
  const int n = t->batch_n;
  if (k < 0 || k >= n)
    return fail(c, RM_ERR_INVALID, "frame " + std::to_string(k) + " of a batch of " + std::to_string(n));
  if (k == n - 1) return f32 ? rm_read_rgba32f(c, (float*)dst, row_pitch, flip_y)
                             : rm_read_rgba8(c, (uint8_t*)dst, row_pitch, flip_y);
  const void* dev;
  if (t->comm && !comm_root(t)) {
    const rm_ctx::BatchSlot& b = t->bslot[t->blast];
    const size_t px = (size_t)t->rows * (size_t)t->cfg.width;
    dev = f32 ? (const void*)(b.send32 ? b.send32 + (size_t)k * px * 4 : nullptr)
              : (const void*)(b.send8 ? b.send8 + (size_t)k * px * bpp8(t) : nullptr);
  } else {
    dev = f32 ? (const void*)((size_t)k < t->ring32.size() ? t->ring32[k] : nullptr)
              : (const void*)((size_t)k < t->ring8.size() ? t->ring8[k] : nullptr);
  }
  return read_image(c, dev, f32 ? 16 : 4, dst, row_pitch, flip_y, !f32 && t->rgb3 && !full_frame(t));
}

int rm_read_frame_rgba8(rm_ctx* c, int32_t k, uint8_t* dst, size_t row_pitch, int flip_y) {
  return read_frame(c, k, false, dst, row_pitch, flip_y);
}

int rm_read_frame_rgba32f(rm_ctx* c, int32_t k, float* dst, size_t row_pitch, int flip_y) {
  return read_frame(c, k, true, dst, row_pitch, flip_y);
}

int rm_get_counters(rm_ctx* c, rm_counters* out) {
  if (!c || !out) return RM_ERR_INVALID;
  if (!c->cfg.counters) return fail(c, RM_ERR_STATE, "context created without counters");
  if (!c->dispatched) return fail(c, RM_ERR_STATE, "no dispatch yet");
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  unsigned long long h[8];
  RM_HIP(c, hipStreamSynchronize(c->stream));
  RM_HIP(c, hipMemcpy(h, c->d_counters, sizeof h, hipMemcpyDeviceToHost));
  out->rays = h[0];
  out->march_steps = h[1];
  out->reflect_steps = h[2];
  out->shadow_steps = h[3];
  out->normals = h[4];
  out->lights = h[5];
  out->sdf_evals = h[1] + h[2] + h[3] + 4 * h[4];
  return RM_OK;
}

int rm_read_sdf_counts(rm_ctx* c, uint32_t* dst) {
  if (!c || !dst) return RM_ERR_INVALID;
  if (!c->cfg.counters) return fail(c, RM_ERR_STATE, "context created without counters");
  if (!c->dispatched) return fail(c, RM_ERR_STATE, "no dispatch yet");
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  RM_HIP(c, hipStreamSynchronize(c->stream));
  RM_HIP(c, hipMemcpy(dst, c->d_counts, (size_t)c->rows * c->cfg.width * 4, hipMemcpyDeviceToHost));
  return RM_OK;
}

// ---- runtime scene table ----------------------------------------------------------
int rm_set_scene(rm_ctx* c, const rm_primitive* prims, int32_t n) {
  if (!c) return RM_ERR_INVALID;
  if (!c->subs.empty()) {  // every device renders the same table
    for (rm_ctx* s : c->subs) {
      const int rc = rm_set_scene(s, prims, n);
      if (rc != RM_OK) return fail(c, rc, s->err);
    }
    c->nprims = c->subs[0]->nprims;
    c->scene = c->subs[0]->scene;
    return RM_OK;
  }
  if (!prims && n == 0) {  // back to the built-in scene
    c->nprims = 0;
    c->scene.clear();
    c->jit = nullptr;
    return RM_OK;
  }
  std::vector<uint32_t> words(rm::scene_words(n > 0 && n <= RM_MAX_PRIMITIVES ? n : 0));
  const char* why = "rm_set_scene: bad table";
  if (rm::compile_scene(prims, n, words.data(), &why) != RM_OK) return fail(c, RM_ERR_INVALID, why);
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  // compile first: a table whose specialisation fails leaves the context as it was
  const rm::JitTable* jit = nullptr;
  if (c->specialize && !has_gbuf(c)) {  // (a G-buffer context renders tables with the generic code)
    std::string err;
    if ((rc = rm::jit_table(words.data(), n, &jit, err)) != RM_OK) return fail(c, rc, err);
    if (!jit->mod) jit = nullptr;  // no spill-free bound: the generic kernel
  }
  if (!c->d_scene) {
    RM_HIP(c, hipMalloc(&c->d_scene, rm::scene_words(RM_MAX_PRIMITIVES) * sizeof(uint32_t)));
  }
  // Ordered on the context's stream after the frames already queued (they keep
  // reading the previous table); the host copy must outlive the async copy, so
  // wait for it before the staging vector is replaced.
  RM_HIP(c, hipStreamSynchronize(c->stream));
  c->scene_words = std::move(words);
  RM_HIP(c, hipMemcpyAsync(c->d_scene, c->scene_words.data(), c->scene_words.size() * sizeof(uint32_t),
                           hipMemcpyHostToDevice, c->stream));
  c->scene.assign(prims, prims + n);
  c->nprims = n;
  c->jit = jit;
  return RM_OK;
}

int rm_scene_compile(const rm_primitive* prims, int32_t n, uint32_t* words, size_t capacity, size_t* nwords) {
  if (!nwords) return fail(nullptr, RM_ERR_INVALID, "rm_scene_compile: null nwords");
  *nwords = 0;
  if (n < 1 || n > RM_MAX_PRIMITIVES)
    return fail(nullptr, RM_ERR_INVALID, "rm_scene_compile: need 1..RM_MAX_PRIMITIVES primitives");
  std::vector<uint32_t> w(rm::scene_words(n));
  const char* why = "rm_scene_compile: bad table";
  if (rm::compile_scene(prims, n, w.data(), &why) != RM_OK) return fail(nullptr, RM_ERR_INVALID, why);
  *nwords = w.size();
  if (words) {
    if (capacity < w.size()) return fail(nullptr, RM_ERR_INVALID, "rm_scene_compile: capacity < *nwords");
    std::memcpy(words, w.data(), w.size() * sizeof(uint32_t));
  }
  return RM_OK;
}

int rm_scene_specialize(rm_ctx* c, int enable) {
  if (!c) return RM_ERR_INVALID;
  for (rm_ctx* s : c->subs) {
    const int rc = rm_scene_specialize(s, enable);
    if (rc != RM_OK) return fail(c, rc, s->err);
  }
  c->specialize = enable != 0;
  if (!c->subs.empty()) return RM_OK;
  if (!c->specialize) {
    c->jit = nullptr;
    return RM_OK;
  }
  // a G-buffer context renders tables with the generic code: nothing to compile
  if (!c->nprims || c->jit || has_gbuf(c)) return RM_OK;
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  std::string err;
  const rm::JitTable* jit = nullptr;
  if ((rc = rm::jit_table(c->scene_words.data(), c->nprims, &jit, err)) != RM_OK) {
    c->specialize = false;
    return fail(c, rc, err);
  }
  c->jit = jit->mod ? jit : nullptr;  // no spill-free bound: the generic kernel
  return RM_OK;
}

int rm_scene_kernel_waves(const rm_ctx* c, int32_t* waves) {
  if (!c || !waves) return RM_ERR_INVALID;
  const rm_ctx* r = c->subs.empty() ? c : c->subs[0];
  *waves = r->jit ? r->jit->waves : 0;
  return RM_OK;
}

int rm_get_scene(const rm_ctx* c, rm_primitive* out, int32_t capacity, int32_t* n) {
  if (!c || !n) return RM_ERR_INVALID;
  *n = c->nprims;
  if (out && c->nprims) {
    if (capacity < c->nprims) return RM_ERR_INVALID;
    std::memcpy(out, c->scene.data(), sizeof(rm_primitive) * c->nprims);
  }
  return RM_OK;
}

// ---- device interop ----------------------------------------------------------------
int rm_set_stream(rm_ctx* c, void* hip_stream) {
  if (!c) return RM_ERR_INVALID;
  if (!c->subs.empty())
    return fail(c, RM_ERR_STATE, "a multi-GPU context runs one stream per device (its own)");
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if (c->own_stream && c->stream) {
    RM_HIP(c, hipStreamSynchronize(c->stream));
    (void)hipStreamDestroy(c->stream);
    c->stream = nullptr;
    c->own_stream = false;
  }
  if (hip_stream) {
    c->stream = static_cast<hipStream_t>(hip_stream);
  } else {
    RM_HIP(c, hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    c->own_stream = true;
  }
  return RM_OK;
}

int rm_set_output_rgba8(rm_ctx* c, void* device_ptr) {
  if (!c) return RM_ERR_INVALID;
  if (!c->subs.empty()) {  // the frame's destination on device 0
    const int rc = rm_set_output_rgba8(c->subs[0], device_ptr);
    return rc == RM_OK ? rc : fail(c, rc, c->subs[0]->err);
  }
  if (!(c->cfg.outputs & RM_OUT_RGBA8))
    return fail(c, RM_ERR_STATE, "RGBA8 output not enabled in rm_config.outputs");
  c->ext_rgba8 = static_cast<uint8_t*>(device_ptr);
  return RM_OK;
}

int rm_get_output_rgba8(rm_ctx* c, void** device_ptr) {
  if (!c || !device_ptr) return RM_ERR_INVALID;
  *device_ptr = image_rgba8(c);
  return RM_OK;
}

// The images live on the context's device (a multi-GPU context's: device 0).
// Everything that writes them is on its stream, or for a communicator batch on
// its gather stream, which the stream itself waits for before any later write
// (order_after_batch); so the caller's stream waits for an event at the tail of
// each.
int rm_wait_output(rm_ctx* c, void* hip_stream) {
  if (!c) return RM_ERR_INVALID;
  rm_ctx* t = c->subs.empty() ? c : c->subs[0];
  if (t->comm_failed || c->comm_failed) return comm_dead(c);
  int rc = set_device(t);
  if (rc != RM_OK) return fail(c, rc, t->err);
  hipStream_t dst = static_cast<hipStream_t>(hip_stream);
  if (!t->out_ev) RM_HIP(c, hipEventCreateWithFlags(&t->out_ev, hipEventDisableTiming));
  RM_HIP(c, hipEventRecord(t->out_ev, t->stream));
  RM_HIP(c, hipStreamWaitEvent(dst, t->out_ev, 0));
  if (t->gstream) RM_HIP(c, hipStreamWaitEvent(dst, t->gdone, 0));
  return RM_OK;
}

int rm_unshard_rgba8(rm_ctx* c, const void* gathered_dev, void* frame_dev) {
  if (!c || !gathered_dev || !frame_dev) return RM_ERR_INVALID;
  if (!c->subs.empty()) return fail(c, RM_ERR_STATE, "a multi-GPU context assembles its own frames");
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  hipError_t e = rm::launch_unshard(gathered_dev, frame_dev, c->cfg.width, c->cfg.height,
                                    c->cfg.row_block, row_block0(c), c->cfg.nshards, c->rows, c->stream, 0,
                                    c->rgb3);
  if (e != hipSuccess) return hip_fail(c, e, "unshard launch");
  return RM_OK;
}

int rm_unshard_batch_rgba8(rm_ctx* c, const void* gathered_dev, int32_t k, int32_t n, void* frame_dev) {
  if (!c || !gathered_dev || !frame_dev) return RM_ERR_INVALID;
  if (n < 1 || k < 0 || k >= n) return fail(c, RM_ERR_INVALID, "rm_unshard_batch_rgba8: need 0 <= k < n");
  if (!c->subs.empty()) return fail(c, RM_ERR_STATE, "a multi-GPU context assembles its own frames");
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  const size_t px = (size_t)c->rows * (size_t)c->cfg.width;
  const uint8_t* src = static_cast<const uint8_t*>(gathered_dev) + (size_t)k * px * bpp8(c);
  hipError_t e = rm::launch_unshard(src, frame_dev, c->cfg.width, c->cfg.height, c->cfg.row_block,
                                    row_block0(c), c->cfg.nshards, c->rows, c->stream, (size_t)n * (size_t)c->rows,
                                    c->rgb3);
  if (e != hipSuccess) return hip_fail(c, e, "unshard launch");
  return RM_OK;
}

// A multi-GPU context times device 0's render kernel.
int rm_enable_timing(rm_ctx* c, int enable) {
  if (!c) return RM_ERR_INVALID;
  if (!c->subs.empty()) return rm_enable_timing(c->subs[0], enable);
  c->timing = enable != 0;
  return RM_OK;
}

int rm_kernel_time_ms(rm_ctx* c, double* total_ms, int64_t* launches, int reset) {
  if (!c) return RM_ERR_INVALID;
  if (!c->subs.empty()) {
    const int rc = rm_kernel_time_ms(c->subs[0], total_ms, launches, reset);
    return rc == RM_OK ? rc : fail(c, rc, c->subs[0]->err);
  }
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  for (size_t i = 0; i < c->ev_used; ++i) {
    RM_HIP(c, hipEventSynchronize(c->ev_pool[i].second));
    float ms = 0.0f;
    RM_HIP(c, hipEventElapsedTime(&ms, c->ev_pool[i].first, c->ev_pool[i].second));
    c->total_ms += ms;
    c->launches += c->ev_frames[i];  // a batch counts its frames
  }
  c->ev_used = 0;
  if (total_ms) *total_ms = c->total_ms;
  if (launches) *launches = c->launches;
  if (reset) {
    c->total_ms = 0.0;
    c->launches = 0;
  }
  return RM_OK;
}

int rm_frame_phases(rm_ctx* c, double* render_ms, double* gather_ms, double* assemble_ms) {
  if (!c) return RM_ERR_INVALID;
  rm_ctx* t = c->subs.empty() ? c : c->subs[0];
  if (!t->ph_recorded) return fail(c, RM_ERR_STATE, "no timed eager dispatch yet (rm_enable_timing, rm_dispatch)");
  int rc = set_device(t);
  if (rc != RM_OK) return rc;
  if ((rc = stream_wait(c)) != RM_OK) return rc;
  (void)set_device(t);
  float ms[3] = {0.0f, 0.0f, 0.0f};
  RM_HIP(c, hipEventElapsedTime(&ms[0], t->ph[0], t->ph[1]));
  if (t->ph_comm) {
    RM_HIP(c, hipEventElapsedTime(&ms[1], t->ph[1], t->ph[2]));
    RM_HIP(c, hipEventElapsedTime(&ms[2], t->ph[2], t->ph[3]));
  }
  if (render_ms) *render_ms = ms[0];
  if (gather_ms) *gather_ms = ms[1];
  if (assemble_ms) *assemble_ms = ms[2];
  return RM_OK;
}

}  // extern "C"
