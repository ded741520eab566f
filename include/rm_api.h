/*
 * rm_api.h — C-ABI of librm, the MI355X-native SDF ray marcher.
 *
 * This is the drop-in boundary that replaces the reference's GL compute
 * program + dispatch (Qirias/OpenGL-RayMarching-in-Compute-Shader):
 *
 *   reference                                   replaced by
 *   ------------------------------------------  ------------------------------------
 *   CreateCompute            shader.hpp:186-197  rm_create (kernels are compiled AOT)
 *   setBool/setInt/setuInt/  shader.hpp:19-69    rm_set_bool/int/uint/float/vec2/3/4
 *   setFloat/setVec2/3/4     (called by name from main.cpp:99-120)
 *   glDispatchCompute        main.cpp:123        rm_dispatch (async, on the ctx stream)
 *   glMemoryBarrier          main.cpp:125        rm_synchronize
 *   Texture::GenerateTexture texture.cpp:10-21   device image owned by rm_ctx
 *   (no readback in the ref; quad draw only)     rm_read_rgba8 / rm_read_rgba32f
 *   Camera ctor/setMouse/lookAt camera.cpp:8-51  rm_camera_* (glm-free, same formulas)
 *
 * Conventions: every entry point returns 0 (RM_OK) on success and a negative
 * RM_ERR_* on failure, with a message available from rm_last_error(ctx).  The
 * one non-error positive code is RM_WARN_UNKNOWN_UNIFORM: like GL's location
 * -1 (shader.hpp:21 glUniform*(-1, ...) is a silent no-op) an unknown uniform
 * name changes nothing, but the caller can see that it happened.
 * No C++ exception crosses this boundary.  One context per host thread (the
 * same constraint as the reference's thread-bound GL context, main.cpp:59).
 * The context owns its device buffers and stream; the caller owns host buffers.
 */
#ifndef RM_API_H
#define RM_API_H

#ifndef __HIPCC_RTC__
#include <stddef.h>
#include <stdint.h>
#endif

#ifdef __cplusplus
extern "C" {
#endif

#define RM_API_VERSION 6
#define RM_CONFIG_MAGIC 0x36434D52u /* "RMC6" little-endian: rm_config layout of API version 6 */

/* ---- status codes --------------------------------------------------------- */
#define RM_OK 0
#define RM_WARN_UNKNOWN_UNIFORM 1 /* name not in the uniform block: no-op */
#define RM_ERR_INVALID (-1)       /* bad argument / shape */
#define RM_ERR_HIP (-2)           /* HIP runtime error */
#define RM_ERR_NOMEM (-3)         /* device or host allocation failed */
#define RM_ERR_NO_DEVICE (-4)     /* no HIP device (librm never falls back to CPU) */
#define RM_ERR_STATE (-5)         /* call not valid in this state */
#define RM_ERR_COMM (-6)          /* RCCL error, or a communicator deadline passed (a peer rank
                                     failed, stalled or never joined): the communicator was
                                     aborted; the context reports RM_ERR_COMM from then on and
                                     can only be destroyed (rm_comm_set_timeout) */

/* ---- output image formats (bitmask for rm_config.outputs) ----------------- */
#define RM_OUT_RGBA8 1   /* display format (what the quad shows, Quad.glsl:21-25) */
#define RM_OUT_RGBA32F 2 /* the reference texture's true storage (texture.cpp:19) */
/* (RM_OUT_GBUFFER 4, every pixel's primary hit: the G-buffer section below) */

/* ---- RGBA8 shard image formats (rm_config.shard_format, API version 6) ----
 * The reference stores alpha = 1.0 in every pixel (finalColor = vec4(render(),
 * 1.0), and the mean of four such, computeShader.glsl:314-341), so a shard that
 * travels to rank 0 need not carry it: an RGB8 shard image is [rows_cap][width]
 * x 3 bytes (R, G, B), and the un-shard writes alpha 255.  The assembled frame
 * is the same RGBA8 image byte for byte; the gather moves 3/4 of the bytes. */
#define RM_SHARD_AUTO 0  /* RGB8 once the context gathers (rm_comm_init, ngpus), else RGBA8 */
#define RM_SHARD_RGBA8 1 /* 4 B per pixel, the display format */
#define RM_SHARD_RGB8 2  /* 3 B per pixel (sharded contexts only; whole frames stay RGBA8) */

/* ---- shadow modes (rm_uniforms.shadow_mode) ------------------------------- */
#define RM_SHADOW_SOFT 0 /* reference: softshadow(k = 2.0)  computeShader.glsl:185,236 */
#define RM_SHADOW_HARD 1 /* extension: k = +inf -> shadow in {0.05, 1}  (BASELINE cfg 1) */

/* ---- kernel variants (rm_config.kernel) ----------------------------------- */
#define RM_KERNEL_AUTO 0       /* the fastest measured variant: RM_KERNEL_PIXEL */
#define RM_KERNEL_PIXEL 1      /* one thread per pixel, 8x8 pixel tile per wave, culled sdf */

/* Uniform block of computeShader.glsl:7,59-66.  vec4s carry w = 0
 * (main.cpp:103-106).  Layout is plain C, not std140. */
typedef struct rm_camera {
  float pos[4];   /* camera.pos    glsl:16 */
  float dir[4];   /* camera.dir    glsl:17 (forward) */
  float yAxis[4]; /* camera.yAxis  glsl:18 (up) */
  float xAxis[4]; /* camera.xAxis  glsl:19 (right) */
} rm_camera;

typedef struct rm_light { /* glsl:22-32 */
  float position[3];
  float ambient[3];
  float diffuse[3];
  float specular[3];
  float constant;
  float linear;
  float quadratic;
} rm_light;

typedef struct rm_uniforms {
  rm_camera camera;     /* glsl:65 */
  rm_light light;       /* glsl:66 */
  float iTime;          /* glsl:62  drives the box/sphere blend, sin(iTime)/2+0.5 (glsl:117) */
  int32_t bounceVar;    /* glsl:60  0..5 (main.cpp:199-204) */
  int32_t AA;           /* glsl:59  4x supersampling on/off */
  uint32_t workgroups;  /* glsl:7   launch geometry only; ignored (librm picks its own) */
  float drand48;        /* glsl:61  unused by the shader; accepted and ignored */
  float mouse[3];       /* glsl:63  unused by the shader; accepted and ignored */
  float iMouse[2];      /* glsl:64  unused by the shader; accepted and ignored */
  int32_t shadow_mode;  /* extension: RM_SHADOW_SOFT (reference) or RM_SHADOW_HARD */
} rm_uniforms;

/* Work counters, in the reference's units (calls as written in the GLSL). */
typedef struct rm_counters {
  uint64_t rays;          /* castRay calls                       glsl:68 */
  uint64_t march_steps;   /* sdf() calls inside RayMarch         glsl:131-139 */
  uint64_t reflect_steps; /* sdf() calls inside reflectedRay     glsl:150-158 */
  uint64_t shadow_steps;  /* sdf() calls inside softshadow       glsl:205-213 */
  uint64_t normals;       /* GetNormal calls (4 sdf each)        glsl:278-288 */
  uint64_t lights;        /* getPointLight calls                 glsl:253-276 */
  uint64_t sdf_evals;     /* march + reflect + shadow + 4*normals */
} rm_counters;

typedef struct rm_config {
  /* sizeof(rm_config) and RM_CONFIG_MAGIC (rm_config_init sets both).  rm_create
   * refuses a config where either differs (RM_ERR_INVALID) instead of reading
   * a stale layout: a v1/v2 host's first two words are width and height, a v3
   * host's second word is its width (<= 65536), and none of them can equal the
   * magic, whatever the struct sizes happen to be (a v3 struct has
   * the same size as this one on LP64). */
  uint32_t struct_size;
  uint32_t magic;
  int32_t width;      /* image width  (SCREEN_WIDTH,  main.cpp:16) */
  int32_t height;     /* image height (SCREEN_HEIGHT, main.cpp:17) */
  int32_t device;     /* HIP device ordinal; -1 = current device */
  int32_t outputs;    /* RM_OUT_* bitmask; 0 = RM_OUT_RGBA8 */
  int32_t kernel;     /* RM_KERNEL_*; 0 = auto */
  int32_t counters;   /* nonzero: collect rm_counters + per-pixel sdf counts (slower) */
  /* Row sharding (multi-GPU): the image's rows are cut into
   * rounds; a round holds rank0_rows rows of shard 0, then row_block rows of
   * shard 1, 2, ..., nshards-1 (rank0_rows = row_block: block b belongs to
   * shard b % nshards).  This context renders only shard `shard`'s rows, packed
   * in round order, into a [rows_cap][width] image (rows_cap = rm_shard_rows()).
   * nshards <= 1 means the whole image. */
  int32_t row_block;
  int32_t shard;
  int32_t nshards;
  /* Rows of shard 0 per round (API version 5); 0 = row_block.  Shard 0 is the
   * rank that assembles every gathered frame (k_unshard), so fewer rows for it
   * balance its render + assembly against the other ranks' render
   * (rm_shard_rows; bench.py --rank0-share). */
  int32_t rank0_rows;
  /* RM_SHARD_* (API version 6): the layout of this context's RGBA8 shard images
   * (its own, a caller's rm_set_output_rgba8 buffer, the batch ring, rank 0's
   * gather buffer) and of the gathered input of rm_unshard_rgba8 /
   * rm_unshard_batch_rgba8.  rm_read_rgba8 / rm_read_frame_rgba8 of an RGB8 shard
   * return RGBA8 (alpha 255; the padding rows too).  Ignored unless sharded. */
  int32_t shard_format;
  /* Multi-GPU frames in one process.  ngpus >= 1 makes the
   * context drive ngpus devices: devices[0..ngpus), or device, device+1, ...
   * when devices is NULL (device -1 = the current device).  Device i renders
   * shard i of the interleaved row blocks (row_block rows per block, 0 = 8);
   * ncclGather over a single-process communicator (ncclCommInitRankConfig per device in one group) collects
   * the shards on devices[0], which assembles the frame (k_unshard).  The
   * setters, rm_dispatch, rm_synchronize, rm_read_rgba8, rm_set_scene and the
   * graph calls work as on a one-GPU context; the frame lives on devices[0].
   * RGBA8 and/or RGBA32F outputs, no counters, shard/nshards must be 0.
   * ngpus = 0: one device, no RCCL (API version 1 behaviour). */
  int32_t ngpus;
  const int32_t *devices;
} rm_config;

typedef struct rm_ctx rm_ctx;

/* ---- lifetime ------------------------------------------------------------- */
/* Zero-fills *cfg and sets struct_size, width, height, device = -1 (current),
 * outputs = RM_OUT_RGBA8, nshards = 1: a one-GPU context with the defaults. */
int rm_config_init(rm_config *cfg, int32_t width, int32_t height);
int rm_create(rm_ctx **out, const rm_config *cfg);
void rm_destroy(rm_ctx *ctx);
const char *rm_last_error(const rm_ctx *ctx);
int rm_api_version(void);
int rm_device_count(int *count);

/* ---- uniforms: by-name setters mirroring shader.hpp:19-69 ------------------
 * Names are the GLSL ones: "iTime", "workgroups", "AA", "bounceVar",
 * "drand48", "mouse", "iMouse", "camera.pos", "camera.dir", "camera.yAxis",
 * "camera.xAxis", "light.position", "light.ambient", "light.diffuse",
 * "light.specular", "light.constant", "light.linear", "light.quadratic",
 * plus the extension "shadow_mode". */
int rm_set_bool(rm_ctx *ctx, const char *name, int value);
int rm_set_int(rm_ctx *ctx, const char *name, int32_t value);
int rm_set_uint(rm_ctx *ctx, const char *name, const uint32_t *value);
int rm_set_float(rm_ctx *ctx, const char *name, float value);
int rm_set_vec2(rm_ctx *ctx, const char *name, float x, float y);
int rm_set_vec3(rm_ctx *ctx, const char *name, float x, float y, float z);
int rm_set_vec4(rm_ctx *ctx, const char *name, float x, float y, float z, float w);
int rm_set_uniforms(rm_ctx *ctx, const rm_uniforms *u);
int rm_get_uniforms(const rm_ctx *ctx, rm_uniforms *u);

/* Defaults of main.cpp:100-120 for the lights/flags and the reference's
 * start-up camera (pos 0, looking down -z): AA on, bounceVar 0, soft shadow. */
int rm_default_uniforms(rm_uniforms *u);

/* ---- dispatch / barrier / readback --------------------------------------- */
/* Render one frame with the current uniforms. Asynchronous on the context's
 * stream (== glDispatchCompute, main.cpp:123). */
int rm_dispatch(rm_ctx *ctx);
/* Render frames[0..n) (API version 4), n <= RM_MAX_BATCH: the same images as
 * rm_set_uniforms(frames[k]) + rm_dispatch for k = 0..n-1, in one launch.  The
 * frames of a batch render concurrently, so the waves of frame k+1 fill the
 * SIMDs that frame k's longest waves leave idle (one tail per batch instead of
 * one per frame).  Asynchronous on the context's stream.  Afterwards the
 * context's uniforms are frames[n-1], its image (rm_read_rgba8 / _rgba32f,
 * rm_get_output_rgba8) holds frame n-1, and rm_read_frame_rgba8 /
 * rm_read_frame_rgba32f read any frame k of the batch (frames 0..n-2 live in a
 * ring the context allocates, n-1 images of each enabled format).  On a
 * communicator context (rm_comm_init, rm_config.ngpus) every rank renders its
 * shards of the n frames in one launch, one ncclGather moves all n shards, and
 * rank 0 assembles the n frames; the gather runs on a second stream of the
 * context, so the next batch renders while this one gathers (a consumer on the
 * caller's own stream orders itself after it with rm_wait_output).  A runtime
 * scene table's frames batch the same way (API version 5; its specialised
 * kernels too).  Frames with a different AA setting, or (specialised tables) a
 * camera that needs the generic kernel, render in separate launches.  Not
 * available with cfg.counters.  Every frame's uniforms are checked before any
 * launch; a batch that still fails (a HIP or RCCL error part way) leaves the
 * context's uniforms as before the call, and its image and ring hold
 * undefined contents until the next successful dispatch. */
#define RM_MAX_BATCH 32
int rm_dispatch_frames(rm_ctx *ctx, const rm_uniforms *frames, int32_t n);
/* Wait for all work queued on the context (== glMemoryBarrier + the
 * implicit sync of the draw, main.cpp:125-134).  On a context with a
 * communicator this wait (and the one inside every readback) is a bounded
 * poll of the stream and of the communicator's asynchronous error: an RCCL
 * error or the deadline aborts the communicator and returns RM_ERR_COMM. */
int rm_synchronize(rm_ctx *ctx);
/* Synchronous readback. Row 0 of the image is the bottom row (py = 0,
 * quad.hpp:9); flip_y != 0 writes the top row first (image-file order).
 * row_pitch is in bytes; 0 = tightly packed. For a sharded context the
 * packed [rows_cap][width] shard image is read (flip_y must be 0). */
int rm_read_rgba8(rm_ctx *ctx, uint8_t *dst, size_t row_pitch, int flip_y);
int rm_read_rgba32f(rm_ctx *ctx, float *dst, size_t row_pitch, int flip_y);
/* Frame k of the last rm_dispatch_frames batch (k = n-1 is the context's image;
 * after a plain rm_dispatch only k = 0 exists).  Same layout rules as above. */
int rm_read_frame_rgba8(rm_ctx *ctx, int32_t k, uint8_t *dst, size_t row_pitch, int flip_y);
int rm_read_frame_rgba32f(rm_ctx *ctx, int32_t k, float *dst, size_t row_pitch, int flip_y);
/* Counters of the last dispatch (requires cfg.counters). */
int rm_get_counters(rm_ctx *ctx, rm_counters *out);
/* Per-pixel sdf() evaluation counts of the last dispatch, summed over the
 * pixel's samples, reference units (requires cfg.counters). */
int rm_read_sdf_counts(rm_ctx *ctx, uint32_t *dst);

/* ---- hipGraph frame replay (BASELINE cfg 5) ------------------------------ */
/* rm_graph_enable(ctx, 1) switches the context to graph replay: the first
 * rm_graph_dispatch captures the render-kernel launch into a graph; every
 * later rm_graph_dispatch writes the current frame constants into the kernel
 * node's by-value argument (hipGraphExecKernelNodeSetParams) and replays the
 * graph on the context's stream (re-captured only when AA toggles, which
 * changes the grid and kernel).  Same kernel and image as rm_dispatch.
 * Not available with cfg.counters. */
int rm_graph_enable(rm_ctx *ctx, int enable);
int rm_graph_dispatch(rm_ctx *ctx);

/* ---- runtime scene table ------------------------------
 * The reference's scene is the hard-coded sdf() of computeShader.glsl:107-123:
 * an opU chain of primitives, each a RayHit {distance, colour, id, material}.
 * rm_set_scene replaces it with a table of up to RM_MAX_PRIMITIVES such
 * entries, evaluated in table order with the same opU rule (a later entry wins
 * unless the running distance is strictly smaller, glsl:105).  The table is
 * staged in LDS by every workgroup of the table kernel.  rm_default_scene
 * returns the reference's scene as a table; rendered through the table kernel
 * it gives the same image as the built-in scene's specialised kernel.
 * The shading rules stay the reference's: id 7 takes the floor branch
 * (shadow, no bounce; glsl:240-247, 177) and material 0 (MATTE) stops the
 * bounce colour accumulation (glsl:189-190). */
#define RM_MAX_PRIMITIVES 32
#define RM_PRIM_SPHERE 0  /* sdSphere(q, r)                               glsl:83 */
#define RM_PRIM_BOX 1     /* sdBox(q, b)                                  glsl:87-91 */
#define RM_PRIM_BLEND 2   /* mix(sdBox(q, b), sdSphere(q, r), sin(iTime)/2 + 0.5)  glsl:115-117 */
#define RM_PRIM_TORUS 3   /* sdTorus(q, (R, r))                           glsl:93-96 */
#define RM_PRIM_CAPSULE 4 /* sdCapsule(q, a, b, r)                        glsl:98-103 */
#define RM_PRIM_PLANE 5   /* sdPlane(q, (nx, ny, nz, w))                  glsl:85 */
#define RM_SWIZZLE_XYZ 0  /* q = p - center */
#define RM_SWIZZLE_XZY 1  /* q = (p - center).xzy  (the torus of glsl:119) */
#define RM_PAINT_SOLID 0    /* RayHit.color = color */
#define RM_PAINT_CHECKERS 1 /* RayHit.color = checkers(p)                 glsl:77-80 */

typedef struct rm_primitive {
  int32_t type;    /* RM_PRIM_* */
  int32_t swizzle; /* RM_SWIZZLE_* */
  int32_t id;      /* RayHit.id (glsl:42) */
  int32_t paint;   /* RM_PAINT_* */
  float material;  /* RayHit.material: 1 REFLECTIVE, 0 MATTE (glsl:4-5) */
  float color[3];
  float center[3];
  /* sphere {r}; box {bx, by, bz}; blend {bx, by, bz, r}; torus {R, r};
   * capsule {ax, ay, az, bx, by, bz, r}; plane {nx, ny, nz, w} */
  float param[7];
} rm_primitive;

/* The reference scene (glsl:107-123) as 6 table entries (the blended box and
 * sphere of glsl:115-117 are one RM_PRIM_BLEND entry, id 4).  *n = 6. */
int rm_default_scene(rm_primitive *out, int32_t capacity, int32_t *n);
/* Render with `prims[0..n)` from the next dispatch on.  prims == NULL and
 * n == 0 return to the built-in scene (the specialised kernel). */
int rm_set_scene(rm_ctx *ctx, const rm_primitive *prims, int32_t n);
/* The table in use (*n = 0: the built-in scene). */
int rm_get_scene(const rm_ctx *ctx, rm_primitive *out, int32_t capacity, int32_t *n);
/* enable != 0: tables render with kernels compiled for the table itself
 * (hiprtc, at this call for the current table and at every later
 * rm_set_scene; the analogue of the reference compiling its shader at run time,
 * CreateCompute shader.hpp:186-197).  Same image as the generic table kernel;
 * compiles are cached per process and device.  A failed compile returns
 * RM_ERR_HIP with the compiler log in rm_last_error and leaves the scene as it
 * was.  A frame whose camera lies farther than 1e15 from the origin (or is not
 * finite) renders with the generic kernel: the specialised kernels take an
 * exact short form of sqrt(x) - R that needs bounded march points.
 * enable == 0: the generic (LDS-staged) table kernel. */
int rm_scene_specialize(rm_ctx *ctx, int enable);
/* The register bound of the specialised table kernels in use: *waves = the
 * waves per SIMD they were compiled for (8, 7 or 6: the most at which they need
 * no scratch), or 0 when the generic table kernel (or the built-in scene)
 * renders; a table that spills at 6 waves is not specialised, and neither is
 * one of more than 12 entries (not compiled at all: past a dozen entries the
 * compile takes minutes and fits no bound). */
int rm_scene_kernel_waves(const rm_ctx *ctx, int32_t *waves);
/* Diagnostics (API version 5): the table as rm_set_scene compiles it on the host
 * for the device (no device needed): the n entries' words, then the exit header
 * with the bounds of the provable exits and the culling balls.  *nwords = its
 * length; words == NULL queries the length only.  RM_ERR_INVALID (with the
 * reason in rm_last_error(NULL)) for a table rm_set_scene would refuse. */
int rm_scene_compile(const rm_primitive *prims, int32_t n, uint32_t *words, size_t capacity, size_t *nwords);
/* Diagnostics: the code object rm_scene_specialize would load for this table
 * on `arch` (e.g. "gfx950"), compiled without a device.  *size = its size;
 * out == NULL queries the size only; *size = 0: the table is not specialised
 * (see rm_scene_kernel_waves). */
int rm_jit_code_object(const rm_primitive *prims, int32_t n, const char *arch, void *out,
                       size_t capacity, size_t *size);

/* ---- device-side interop (plain pointers; for stream/collective plumbing) - */
/* Use an external stream (hipStream_t passed as void*); NULL = own stream. */
int rm_set_stream(rm_ctx *ctx, void *hip_stream);
/* Render RGBA8 into a caller-owned device buffer of >= rows*width*4 bytes
 * (rows = height, or rows_cap when sharded) instead of the context's own.
 * A sharded context with RGB8 shards writes rows of width*3 bytes there.
 * NULL restores the internal buffer. */
int rm_set_output_rgba8(rm_ctx *ctx, void *device_ptr);
/* Device pointer of the RGBA8 image the next dispatch writes (a shard of an
 * RGB8 context: packed rows of width*3 bytes, rm_config.shard_format). */
int rm_get_output_rgba8(rm_ctx *ctx, void **device_ptr);
/* Orders `hip_stream` (hipStream_t as void*; NULL = the null stream) after every
 * write to the context's images queued so far: work the caller enqueues on it
 * afterwards sees the last dispatch's frames (API version 5).  Needed on a
 * communicator context (rm_comm_init, rm_config.ngpus): a batch's gather and
 * rank 0's assembly run on the context's internal gather stream, so frame n-1
 * in rm_get_output_rgba8 / rm_set_output_rgba8's buffer (and the batch's ring)
 * is not ordered by rm_set_stream's stream alone.  rm_synchronize and the
 * readbacks wait for it as well.  Asynchronous: records events, waits on none. */
int rm_wait_output(rm_ctx *ctx, void *hip_stream);
/* Assemble a full image from nshards packed shard images laid out
 * back-to-back ([nshards][rows_cap][width] RGBA8, e.g. the result of an RCCL
 * gather; RGB8, 3 B per pixel, when the context's shard_format is RGB8) into
 * `frame` ([height][width] RGBA8), both device pointers, on the context's
 * stream. Uses the context's width/height/row_block/rank0_rows/nshards and
 * shard format. */
int rm_unshard_rgba8(rm_ctx *ctx, const void *gathered_dev, void *frame_dev);
/* The same for frame k of an n-frame batch gathered as rm_dispatch_frames
 * gathers it: [nshards][n][rows_cap][width] RGBA8 or RGB8 (each rank's n shards
 * back to back, ranks in order), e.g. by a host that moves the shards itself. */
int rm_unshard_batch_rgba8(rm_ctx *ctx, const void *gathered_dev, int32_t k, int32_t n, void *frame_dev);
/* Kernel timing: when enabled, HIP events bracket every render-kernel launch
 * on the launch stream; rm_kernel_time_ms returns the summed kernel time and
 * launch count since the last reset (synchronizes). */
int rm_enable_timing(rm_ctx *ctx, int enable);
int rm_kernel_time_ms(rm_ctx *ctx, double *total_ms, int64_t *launches, int reset);
/* Phases of the last rm_dispatch issued with timing enabled (synchronizes):
 * the render kernel, then on a communicator context the gather (render end to
 * gather end on this rank's stream, so it includes waiting for the slowest
 * peer's shard) and rank 0's assembly (0 elsewhere).  A multi-GPU context
 * reports device 0.  RM_ERR_STATE before such a dispatch. */
int rm_frame_phases(rm_ctx *ctx, double *render_ms, double *gather_ms, double *assemble_ms);

/* ---- ray queries: caller-supplied rays against the scene ---------------------
 * The reference marches camera rays only (castRay, glsl:68-74).  These calls run
 * its RayMarch / GetNormal / softshadow / render on any rays: picking, depth or
 * id under a point, line of sight to the light, collision probes, a per-pixel
 * depth / normal / id pass.  Ray i is (origins[i], dirs[i]), [n][3] floats each;
 * hit i is one rm_ray_hit.
 *
 *  - A query uses the context's current uniforms and scene at the time of the
 *    call: iTime drives the blend; the light and camera.pos feed getPointLight
 *    (its view vector) under RM_TRACE_SHADE; bounceVar and shadow_mode apply as in
 *    a dispatch; the scene is the built-in one or the rm_set_scene table (a
 *    context with rm_scene_specialize on traces with the generic table code).
 *    The uniforms are checked as rm_set_uniforms checks them.
 *  - rd is NOT normalised and need not be unit length: t is the GLSL's parameter
 *    along rd as given, the point ro + rd * t (what RayMarch does, glsl:125-142).
 *  - Every input, of any value, gives the reference's result: zero, huge,
 *    infinite and NaN ro or rd included.
 *  - Queries are ordered on the context's stream (rm_set_stream's when one is
 *    set) after the dispatches already queued.  They touch neither the
 *    context's images nor its counters nor its batch ring, and are not part of
 *    graph replay.  A context with cfg.counters traces with the production device
 *    code and leaves rm_counters alone.  With rm_enable_timing on, a trace launch
 *    is bracketed and counted like a render launch.
 *  - The rays of one wave are 64 consecutive indices: a caller that wants speed
 *    keeps neighbouring rays neighbouring; any order is correct.
 *  - A sharded context, or one of an rm_comm_init communicator, traces locally:
 *    the call is not collective.  A multi-device context (cfg.ngpus >= 1):
 *    RM_ERR_STATE.
 *
 * Returns: n == 0 is RM_OK and writes nothing.  RM_ERR_INVALID for a null
 * pointer with n > 0, n < 0 or n > 2^31 - 1, a hits_dev that is not 16-byte
 * aligned, unknown flag bits, RM_TRACE_SHADOW combined with any other flag,
 * RM_TRACE_SHADE | RM_TRACE_REFLECTED, and rm_pick outside the frame. */
#define RM_HAS_TRACE 1
/* rm_trace flags */
#define RM_TRACE_HIT       0  /* RayMarch(ro, rd) glsl:125-142: t, id, material, albedo */
#define RM_TRACE_REFLECTED 1  /* reflectedRay's limits instead (256 steps, tmax 200; glsl:144-161) */
#define RM_TRACE_NORMAL    2  /* + GetNormal(ro + rd*t) on a hit (glsl:278-288) */
#define RM_TRACE_SHADE     4  /* + render(ro, rd) glsl:218-251: the colour a pixel sample with this ray gets */
#define RM_TRACE_SHADOW    8  /* alone: t = softshadow(ro, rd, k) glsl:201-216, k from shadow_mode */

typedef struct rm_ray_hit {   /* 48 bytes */
  float   t;          /* RayHit.hitpoint; -1 = miss (the GLSL's dummy).  SHADOW: the shadow factor */
  int32_t id;         /* RayHit.id; -1 on a miss */
  float   material;   /* RayHit.material; 1.0 on a miss (the dummy's) */
  float   albedo[3];  /* RayHit.color (checkers(p) for the floor); 0 on a miss */
  float   normal[3];  /* RM_TRACE_NORMAL and a hit, else 0 */
  float   color[3];   /* RM_TRACE_SHADE, else 0 */
} rm_ray_hit;

/* Host rays and hits; synchronous (upload, trace, download through staging
 * buffers the context owns, grown on demand, freed by rm_destroy). */
int rm_trace_rays(rm_ctx *ctx, const float *origins, const float *dirs, int64_t n, uint32_t flags, rm_ray_hit *hits);
/* Device pointers; asynchronous on the context's stream.  hits_dev: 16-byte aligned. */
int rm_trace_rays_device(rm_ctx *ctx, const void *origins_dev, const void *dirs_dev, int64_t n, uint32_t flags,
                         void *hits_dev);
/* The ray of pixel (px, py) of the context's frame as a frame without
 * supersampling casts it: uv = (2 p - dims) / dims (glsl:301-305), castRay with
 * the current camera; flags RM_TRACE_HIT | RM_TRACE_NORMAL; synchronous.  Row 0 is
 * the bottom row: a window cursor's y maps to height - 1 - y. */
int rm_pick(rm_ctx *ctx, int32_t px, int32_t py, rm_ray_hit *hit);

/* ---- SDF field queries: distance, id and normal at points and on grids ---------
 * A ray query cannot return a distance at a point.  These calls evaluate the
 * scene's sdf() (glsl:107-123) and GetNormal() (glsl:278-288) themselves: keep a
 * camera or a particle set out of the objects, bake the scene into a 3-D
 * distance volume for meshing, a physics broad phase or another renderer's 3-D
 * texture.
 *
 * Points: point i is points[i], [n][3] floats; its answer is one rm_ray_hit.
 *  - t is sdf(p).hitpoint: the GLSL's sdf() returns a RayHit whose hitpoint is
 *    the distance (negative inside an object).  id, material and albedo are the
 *    opU winner's (albedo is checkers(p) for a checkers entry); normal is
 *    GetNormal(p) under RM_SDF_NORMAL, else 0; color is always 0.  There is no
 *    miss record: sdf() always has a winner.  A NaN distance loses every <, so
 *    the last entry wins.
 * Grids: point (i, j, k) has the coordinate origin[a] + (float)idx * step[a] on
 * each axis a: one IEEE multiply, then one IEEE add, no FMA.
 *  - The outputs are dist[nz][ny][nx] float and ids[nz][ny][nx] int32
 *    (RayHit.id), x fastest.  Either pointer may be NULL, not both.  Device
 *    pointers need 4-byte alignment only (16-byte stores are used where the
 *    pointers and nx allow).  Every dim is in 0..2^24 and their product at most
 *    2^31 - 1; a zero dim (the others valid) is RM_OK, writes nothing and looks at
 *    no pointer, as n == 0 does for points.  origin and step may be
 *    any floats: zero, negative, infinite or NaN.
 *
 *  - A query uses the context's current uniforms and scene at the time of the
 *    call; of the uniforms only iTime is read (it drives the blend).  The
 *    uniforms are checked as rm_set_uniforms checks them.  The scene is the
 *    built-in one or the rm_set_scene table (a context with rm_scene_specialize
 *    on queries with the generic table code).
 *  - Every input, of any value, gives the reference's result: -0, huge, infinite
 *    and NaN coordinates included.
 *  - Queries are ordered on the context's stream (rm_set_stream's when one is
 *    set) after the work already queued.  They touch neither the context's
 *    images nor its G-buffer nor its counters nor its batch ring, and are not
 *    part of graph replay.  A context with cfg.counters queries with the
 *    production device code and leaves rm_counters alone.  With rm_enable_timing
 *    on, a query's launch is bracketed and counted like a trace launch.
 *  - The points of one wave are 64 consecutive indices: a caller that wants speed
 *    keeps neighbouring points neighbouring; any order is correct.
 *  - A sharded context, or one of an rm_comm_init communicator, evaluates
 *    locally: the call is not collective.  A multi-device context
 *    (cfg.ngpus >= 1): RM_ERR_STATE.  G-buffer contexts are allowed.
 *
 * Returns: n == 0 is RM_OK and writes nothing.  RM_ERR_INVALID for a null
 * pointer with work to do, n < 0 or n > 2^31 - 1, unknown flag bits, an out_dev
 * that is not 16-byte aligned, a grid with both outputs NULL, a dim that is
 * negative or above 2^24, a product above 2^31 - 1, a grid output that is not
 * 4-byte aligned.  A null context: RM_ERR_INVALID, nothing touched. */
#define RM_HAS_SDF_QUERY 1
/* rm_sdf flags */
#define RM_SDF_VALUE  0   /* sdf(p) glsl:107-123: t = RayHit.hitpoint (the distance, negative inside), id, material, albedo */
#define RM_SDF_NORMAL 2   /* + GetNormal(p) glsl:278-288 (same bit as RM_TRACE_NORMAL) */

/* Host points and records; synchronous (upload, evaluate, download through
 * staging buffers the context owns, grown on demand, freed by rm_destroy). */
int rm_sdf_points(rm_ctx *ctx, const float *points, int64_t n, uint32_t flags, rm_ray_hit *out);
/* Device pointers; asynchronous on the context's stream.  out_dev: 16-byte aligned. */
int rm_sdf_points_device(rm_ctx *ctx, const void *points_dev, int64_t n, uint32_t flags, void *out_dev);

typedef struct rm_sdf_grid_desc {  /* 36 bytes; x, y, z */
  float   origin[3];
  float   step[3];
  int32_t dims[3];
} rm_sdf_grid_desc;
/* Host outputs; synchronous. */
int rm_sdf_grid(rm_ctx *ctx, const rm_sdf_grid_desc *grid, float *dist, int32_t *ids);
/* Device outputs; asynchronous on the context's stream. */
int rm_sdf_grid_device(rm_ctx *ctx, const rm_sdf_grid_desc *grid, void *dist_dev, void *ids_dev);

/* ---- SDF mesh extraction: a surface-nets mesh of the scene from a grid -----------
 * rm_sdf_grid gives the distance volume; these calls give the surface in it, on
 * the device: one vertex per sign-changing cell, one quad per sign-changing grid
 * edge, with an id, a colour and a GetNormal per vertex.  For collision meshes,
 * export to a rasteriser or a printer, a wireframe or proxy view.  The rule below
 * is a sequence of single IEEE operations in a fixed order and the output order
 * follows from the grid order alone, so the mesh is reproducible bit for bit.
 *
 * Grid: rm_sdf_grid's.  Point (i, j, k) has the coordinate origin[a] +
 *    (float)idx * step[a] per axis, d(i, j, k) is exactly the float rm_sdf_grid
 *    returns for it, and the limits are the same: every dim in 0..2^24, their
 *    product at most 2^31 - 1.
 * Inside: a point is inside iff d < 0.0f.  NaN, +0 and -0 are outside.
 * Cells and vertices: cell (i, j, k), i < nx - 1, j < ny - 1, k < nz - 1, is
 *    active iff its 8 corners are neither all inside nor all outside.  Active
 *    cells are numbered in cell order, x fastest, then y, then z: that number is
 *    the cell's vertex index.  A grid with a dim below 2 has no cell: counts
 *    0 / 0, RM_OK, nothing written but *counts.
 * Vertex position: the mean of the crossings on the cell's 12 edges.
 *  - Edge order: axis a = x, y, z; with u = (a + 1) % 3 and v = (a + 2) % 3 the
 *    edge starts at the corner offsets (du, dv) = (0,0), (1,0), (0,1), (1,1) and
 *    runs from A to B = A + e_a.
 *  - An edge whose ends differ in "inside" contributes a point p:
 *    t = dA / (dA - dB); p[a] = cA + t * (cB - cA), cA and cB the two grid
 *    coordinates on axis a; p[u] and p[v] are A's grid coordinates.
 *  - Per component: acc = 0.0f; acc = acc + p in edge order; pos = acc /
 *    (float)count.  Each of these is one IEEE single-precision operation in the
 *    order written, no FMA.
 * Quads: for every grid point A = (i, j, k) in point order (x fastest) and for
 *    a = x, y, z in that order, the edge A -> A + e_a emits a quad iff it exists,
 *    its ends differ in "inside", and it is interior: 1 <= A[u] <= n[u] - 2 and
 *    1 <= A[v] <= n[v] - 2.
 *  - The quad joins the vertices of the four cells around the edge, at the cell
 *    offsets (du, dv) = (-1,-1), (0,-1), (0,0), (-1,0) from A; all four are
 *    active by construction.  If A is inside the corners come in that order:
 *    counter-clockwise seen from +a, outward normal +a.  If B is inside the
 *    order is 0, 3, 2, 1.  Quads are numbered in emission order.
 *  - Boundary edges emit nothing: a surface that leaves the grid ends in an open
 *    border one cell inside it.
 * Attributes: attr[v] is the record rm_sdf_points gives for pos[v], bit for bit:
 *    t the residual distance, id / material / albedo the opU winner's, normal
 *    under RM_MESH_NORMAL else 0, color 0.
 * Capacities, as snprintf: *counts always holds the whole mesh; vertices
 *    v < vcap and quads q < qcap are written, whole records only, and nothing
 *    past them is touched; RM_OK either way.  A written quad may name a vertex
 *    >= vcap.  vcap == 0 and qcap == 0 with null outputs is the count-only
 *    query; attr == NULL skips the attributes.
 *  - Every input gives this rule's result: any origin or step (zero, negative,
 *    infinite or NaN; a NaN volume is all outside and gives an empty mesh) and
 *    any iTime.
 *
 *  - The call uses the context's current uniforms (only iTime is read) and scene
 *    (built-in or rm_set_scene table; generic table code under
 *    rm_scene_specialize).  The distance volume and the per-wave bookkeeping
 *    live in buffers the context owns, grown on demand, freed by rm_destroy.
 *  - It is ordered on the context's stream.  It touches neither the context's
 *    images nor its G-buffer nor its counters nor its batch ring nor its AA
 *    mask, and is not part of graph replay.  With rm_enable_timing on, one event
 *    pair brackets the whole sequence and it counts as one launch.
 *  - It runs locally on sharded and communicator contexts; G-buffer and
 *    counters contexts are allowed.  cfg.ngpus >= 1: RM_ERR_STATE.
 *
 * Returns RM_ERR_INVALID, nothing written, for: a null context, grid or counts;
 * unknown flag bits; negative capacities; a null pos / indices with a capacity
 * > 0; a pos_dev / indices_dev / attr_dev that is not 16-byte aligned; a
 * counts_dev that is not 8-byte aligned; the grid errors of rm_sdf_grid. */
#define RM_HAS_SDF_MESH 1
#define RM_MESH_QUADS     0u  /* indices: [quads][4] uint32, one 16-byte record per quad */
#define RM_MESH_TRIANGLES 1u  /* indices: [quads][6] uint32: (q0,q1,q2),(q0,q2,q3) of the same quad */
#define RM_MESH_NORMAL    2u  /* attr[v].normal = GetNormal(pos[v]) (the bit of RM_SDF_NORMAL) */

typedef struct rm_sdf_mesh_counts { uint64_t vertices, quads; } rm_sdf_mesh_counts; /* 16 bytes */

/* Host outputs; synchronous.  pos: [vcap][3] float; attr: [vcap] rm_ray_hit or NULL;
 * indices: [qcap][4 or 6] uint32.  *counts is always the whole mesh's. */
int rm_sdf_mesh(rm_ctx *ctx, const rm_sdf_grid_desc *grid, uint32_t flags,
                float *pos, rm_ray_hit *attr, int64_t vcap,
                uint32_t *indices, int64_t qcap, rm_sdf_mesh_counts *counts);
/* Device outputs; asynchronous on the context's stream; counts_dev: 8-byte aligned device
 * memory of one rm_sdf_mesh_counts.  The host never learns the counts. */
int rm_sdf_mesh_device(rm_ctx *ctx, const rm_sdf_grid_desc *grid, uint32_t flags,
                       void *pos_dev, void *attr_dev, int64_t vcap,
                       void *indices_dev, int64_t qcap, void *counts_dev);

/* ---- G-buffer: every pixel's primary hit, from the frame kernels themselves ----
 * The reference's author wanted a normal and a depth view of the frame (both
 * commented out in render(), glsl:229, 248-249).  With RM_OUT_GBUFFER in
 * rm_config.outputs (with RM_OUT_RGBA8 and/or RM_OUT_RGBA32F, or alone) the
 * context owns a third image, [rows][width] of rm_gbuffer_px (rows: the height,
 * or a shard's rows_cap; row 0 is the bottom row, as for the colour images), and
 * every rm_dispatch writes it from the primary hit the frame kernel holds anyway:
 * the price of its stores, not of a second march (rm_trace_rays_device over the
 * frame's rays marches every ray again).
 *
 *  - A record holds rm_ray_hit's fields of the same names with the same miss
 *    values, so it compares field by field with a RM_TRACE_HIT | RM_TRACE_NORMAL
 *    trace of the pixel's ray.  `material` is left out to keep the record at 32
 *    bytes (two 16-byte stores per pixel): it is 0 for id 7 of the built-in
 *    scene, and the table entry's for a table.
 *  - Which ray: without supersampling the pixel's one castRay ray, the ray rm_pick
 *    casts.  With AA on, the FIRST sample's ray: uv after the first offset pair,
 *    (2 p - dims) / dims + 0.25 / dims (glsl:311-313).  The supersampling kernel
 *    casts no centre ray; t, id, normal and albedo are one sample's, not averages.
 *  - The padding rows of a sharded context hold the miss record.
 *  - The colour images are what they are without the bit, bit for bit.
 *  - This version: rm_dispatch on a one-device context, whole or row-sharded
 *    (nshards > 1 without a communicator); the built-in scene and rm_set_scene
 *    tables; AA on and off; every bounceVar and shadow_mode.  rm_create refuses
 *    the bit together with cfg.counters or cfg.ngpus >= 1 (RM_ERR_INVALID).  On a
 *    G-buffer context rm_dispatch_frames, rm_graph_enable(ctx, 1),
 *    rm_graph_dispatch and rm_comm_init return RM_ERR_STATE.
 *  - rm_scene_specialize on a G-buffer context: accepted, but tables render
 *    through the generic table code (as ray queries do), no kernel is compiled
 *    and rm_scene_kernel_waves reports 0.  The images are the same. */
#define RM_HAS_GBUFFER 1
#define RM_OUT_GBUFFER 4 /* rm_config.outputs: the per-pixel primary hit (rm_gbuffer_px) */

typedef struct rm_gbuffer_px {  /* 32 bytes */
  float   t;          /* RayHit.hitpoint of the pixel's primary ray; -1 = miss */
  int32_t id;         /* RayHit.id; -1 on a miss */
  float   normal[3];  /* GetNormal(ro + rd*t) on a hit, else 0 */
  float   albedo[3];  /* RayHit.color (checkers(p) on the floor); 0 on a miss */
} rm_gbuffer_px;

/* Synchronous readback of the last dispatch's G-buffer; row_pitch (bytes, 0 =
 * width * 32), flip_y and the shard rules are rm_read_rgba32f's.  RM_ERR_STATE
 * without RM_OUT_GBUFFER or before the first dispatch. */
int rm_read_gbuffer(rm_ctx *ctx, rm_gbuffer_px *dst, size_t row_pitch, int flip_y);
/* Render the G-buffer into a caller-owned device buffer of rows * width * 32
 * bytes, 16-byte aligned (else RM_ERR_INVALID); NULL restores the context's own.
 * rm_wait_output and rm_synchronize order it like the colour images. */
int rm_set_output_gbuffer(rm_ctx *ctx, void *device_ptr);
int rm_get_output_gbuffer(rm_ctx *ctx, void **device_ptr);

/* ---- adaptive supersampling: 4 samples only where the frame has edges -----------
 * An extension, like RM_SHADOW_HARD.  The frame of these calls is the AA-off
 * frame with every FLAGGED pixel replaced by that pixel of the AA-on frame, so
 * every pixel is exactly one of two reference values.
 *
 *  - Pass 1: every pixel is what rm_dispatch with AA = 0 writes (the centre ray,
 *    glsl:301-305).
 *  - Flagging, rm_dispatch_adaptive: pixel p is flagged iff some 4-neighbour q
 *    (left, right, below, above) inside the frame has
 *    max over R, G, B of |p_c - q_c| > threshold, on the RGBA8 values of pass 1
 *    (round(clamp(c, 0, 1) * 255), NaN -> 0: what rm_read_rgba8 returns; a context
 *    with only RM_OUT_RGBA32F quantises the same floats the same way).  Alpha
 *    takes no part.  Threshold 255 flags nothing (the frame is the AA-off frame);
 *    a 1x1 frame has no neighbour and flags nothing.
 *  - Flagging, rm_dispatch_refine / _device: the caller's mask, [height][width]
 *    bytes, row 0 the bottom row, rows row_pitch bytes apart (0 = width); any
 *    non-zero byte flags its pixel (foveation, a G-buffer criterion of the
 *    caller's own, a previous frame's mask).  The context keeps its own
 *    normalised 0/1 copy, which rm_read_aa_mask and rm_get_aa_mask return; the
 *    device mask may be that copy itself (row_pitch 0 or width).
 *  - Refinement: a flagged pixel gets the reference's four cumulative sample rays
 *    (glsl:309-336), summed ((c0 + c1) + c2) + c3, then / 4: the AA-on frame's
 *    pixel bit for bit in RGBA32F and byte for byte in RGBA8.
 *  - The reference's AA samples sit at +0.125 .. +1 pixel from the pixel's centre
 *    ray, not around it: a refined pixel is the reference's AA pixel with that
 *    shift.  These calls do not re-centre it (rm_dispatch_adaptive_pattern and
 *    rm_dispatch_refine_pattern below refine with a centred pattern).
 *  - u.AA is ignored and the context's uniforms stay as they are; bounceVar,
 *    shadow_mode, iTime, the light and the camera apply as in rm_dispatch.
 *  - Afterwards the context reads as after an rm_dispatch (rm_read_rgba8 /
 *    _rgba32f, rm_get_output_rgba8, rm_set_output_rgba8, rm_wait_output,
 *    rm_synchronize).  Nothing is sticky: the next rm_dispatch or
 *    rm_dispatch_frames is what it always was.  Everything is queued on the
 *    context's stream (rm_set_stream's when one is set); with rm_enable_timing
 *    one event pair brackets the whole sequence, one launch of one frame.
 *  - This version: one-device, whole-frame contexts; the built-in scene and
 *    rm_set_scene tables (with rm_scene_specialize on, pass 1 uses the kernel
 *    rm_dispatch would, the refinement the generic table code, as ray queries do:
 *    same values); colour contrast is the only built-in criterion of
 *    rm_dispatch_adaptive (rm_dispatch_adaptive_edges below has the geometric
 *    ones).  RM_ERR_STATE on a context with counters, nshards > 1, a
 *    communicator, ngpus >= 1, RM_OUT_GBUFFER or rm_graph_enable on; no batches,
 *    no graph replay.
 *  - The environment variable RM_AA_REFINE_WAVES (1..65535, read by rm_create)
 *    overrides the refinement's grid size, min(ceil(W H / 16), 128 x compute units)
 *    one-wave workgroups. */
#define RM_HAS_ADAPTIVE_AA 1

/* threshold in 0..255 (else RM_ERR_INVALID).  Asynchronous. */
int rm_dispatch_adaptive(rm_ctx *ctx, int32_t threshold);
/* A host mask: uploaded synchronously (the caller's buffer is free on return),
 * the frame itself is asynchronous.  RM_ERR_INVALID for a null mask or a
 * row_pitch below width. */
int rm_dispatch_refine(rm_ctx *ctx, const uint8_t *mask, size_t row_pitch);
/* A device mask, read on the context's stream.  Asynchronous. */
int rm_dispatch_refine_device(rm_ctx *ctx, const void *mask_dev, size_t row_pitch);
/* Synchronous readback of the 0/1 mask of the last such dispatch; row_pitch
 * (bytes, 0 = width) and flip_y as rm_read_rgba8.  RM_ERR_STATE before the first. */
int rm_read_aa_mask(rm_ctx *ctx, uint8_t *dst, size_t row_pitch, int flip_y);
/* The context's mask image, [height][width] uint8, tight (allocated on first use). */
int rm_get_aa_mask(rm_ctx *ctx, void **device_ptr);
/* Flagged pixels of the last such dispatch; synchronises.  RM_ERR_STATE before the first. */
int rm_aa_refined(rm_ctx *ctx, int64_t *pixels);

/* ---- adaptive supersampling by geometric edges, from pass 1's own G-buffer ------
 * rm_dispatch_adaptive_edges is rm_dispatch_adaptive with another flagging step:
 * pass 1, the refinement and everything under "Afterwards" above are the same,
 * and the frame is again the AA-off frame with every flagged pixel replaced by
 * the AA-on frame's.  The flags are the union of the criteria selected in
 * rm_aa_criteria.edges, evaluated on the device on what pass 1 has just written:
 * its rm_gbuffer_px records (the G-buffer section above) and / or its RGBA8 image.
 *
 *  - Flagging: pixel p is flagged iff some 4-neighbour q (left, right, below,
 *    above) inside the frame satisfies at least one selected criterion for the
 *    pair (p, q):
 *      RM_AA_EDGE_COLOR   max over R, G, B of |p_c - q_c| > color_threshold on pass
 *                         1's RGBA8 values: rm_dispatch_adaptive's rule, word for word;
 *      RM_AA_EDGE_ID      p.id != q.id (a miss has id -1, so a hit beside a miss is
 *                         an edge and two misses are not);
 *      RM_AA_EDGE_DEPTH   both hit and fabsf(p.t - q.t) > depth_rel * fminf(p.t, q.t);
 *      RM_AA_EDGE_NORMAL  both hit and
 *                         (p.normal[0] * q.normal[0] + p.normal[1] * q.normal[1])
 *                           + p.normal[2] * q.normal[2] < normal_cos;
 *      RM_AA_EDGE_ALBEDO  p.albedo[c] != q.albedo[c] for some c (the floor's checker
 *                         edges, and every edge between two colours).
 *    p and q are pass 1's records: the centre ray's hit, the ray rm_pick casts.
 *    "Hit" is t != -1.0f, the GLSL's own test.  Every float operation is one IEEE
 *    single-precision operation in the order written, no FMA: three separate
 *    multiplies and two separate adds in the dot product.  The compares are the
 *    ones written, so a NaN fails > and < and passes !=: a NaN normal is no
 *    NORMAL edge, a NaN albedo is an ALBEDO edge, a NaN t is a hit and no DEPTH
 *    edge.  Every pair test is symmetric in p and q, so the mask is symmetric
 *    like the colour rule's: if q flags p, p flags q.  A 1x1 frame flags nothing.
 *    depth_rel = +inf under DEPTH alone flags nothing (a hit has t >= 0, so
 *    the right-hand side is +inf, or NaN at t = 0); depth_rel = 0 flags
 *    every pair of hits with different t.
 *  - Contexts: ID, DEPTH, NORMAL and ALBEDO read the G-buffer and need
 *    RM_OUT_GBUFFER in rm_config.outputs; without it RM_ERR_STATE.  COLOR alone
 *    works wherever rm_dispatch_adaptive does, and on G-buffer contexts too.  A
 *    context with RM_OUT_GBUFFER and no colour output has nothing to refine:
 *    RM_ERR_STATE.  Otherwise as rm_dispatch_adaptive: RM_ERR_STATE with
 *    counters, nshards > 1, a communicator, ngpus >= 1 or rm_graph_enable on;
 *    the built-in scene and rm_set_scene tables.  rm_dispatch_adaptive,
 *    rm_dispatch_refine and rm_dispatch_refine_device keep refusing G-buffer
 *    contexts; rm_read_aa_mask, rm_get_aa_mask and rm_aa_refined serve them.
 *  - The G-buffer afterwards: rm_read_gbuffer, and the buffer of
 *    rm_set_output_gbuffer (the one classified, when one is set), hold pass 1's
 *    records for every pixel, flagged or not: the G-buffer of an rm_dispatch with
 *    AA off, bit for bit.  The refinement writes colour only.  This differs from
 *    an rm_dispatch with AA on, whose G-buffer holds the first sample's ray: a
 *    refined pixel's colour is the four samples' mean, its record the centre ray's.
 *  - Fields whose bit is clear are not read and not checked.
 *  - The environment variable RM_AA_EDGES_NAIVE (set to anything but "0"; read
 *    by every call) selects the classifier's plain form, which tests all four
 *    neighbours in every lane: the same mask, kept for measurement. */
#define RM_HAS_ADAPTIVE_EDGES 1
#define RM_AA_EDGE_COLOR   1u  /* rm_dispatch_adaptive's rule at color_threshold */
#define RM_AA_EDGE_ID      2u  /* p.id != q.id (a miss has id -1) */
#define RM_AA_EDGE_DEPTH   4u  /* both hit and fabsf(p.t - q.t) > depth_rel * fminf(p.t, q.t) */
#define RM_AA_EDGE_NORMAL  8u  /* both hit and dot(p.normal, q.normal) < normal_cos */
#define RM_AA_EDGE_ALBEDO 16u  /* some albedo component has p.albedo[c] != q.albedo[c] (checker edges) */

typedef struct rm_aa_criteria {   /* 20 bytes */
  uint32_t struct_size;           /* sizeof(rm_aa_criteria); anything else: RM_ERR_INVALID */
  uint32_t edges;                 /* RM_AA_EDGE_* mask, non-zero, no unknown bit */
  int32_t  color_threshold;       /* 0..255, read only under COLOR */
  float    depth_rel;             /* >= 0, +inf allowed, not NaN; read only under DEPTH */
  float    normal_cos;            /* in [-1, 1], not NaN; read only under NORMAL */
} rm_aa_criteria;

/* struct_size, and ID | DEPTH | NORMAL at color_threshold 8, depth_rel 0.05f,
 * normal_cos 0.9f.  RM_ERR_INVALID for NULL. */
int rm_aa_criteria_init(rm_aa_criteria *c);
/* RM_ERR_INVALID for a null context (nothing written), null criteria, or a
 * field outside the ranges above.  Asynchronous. */
int rm_dispatch_adaptive_edges(rm_ctx *ctx, const rm_aa_criteria *criteria);

/* ---- sample patterns: a frame supersampled at caller-chosen offsets --------------
 * An extension.  rm_dispatch_pattern renders the whole frame with n sample rays
 * per pixel at the offsets of an rm_sample_pattern, in pixels from the AA-off
 * frame's ray (the ray rm_pick casts), and stores their mean: a re-centred or
 * rotated grid that registers with the AA-off frame and the G-buffer, 8, 9 or 16
 * samples per pixel, or one jittered sample per frame (n = 1) for temporal
 * accumulation (rm_dispatch_accumulate below keeps the sum).
 *
 * The rule.  Every operation is one IEEE single-precision operation in the order
 * written, with no FMA.
 *
 *  - uv.  x0 = (float)(2 px - W) / (float)W and y0 = (float)(2 py - H) / (float)H
 *    (glsl:301-305).  ox_s = (2.0f * dx[s]) / (float)W and
 *    oy_s = (2.0f * dy[s]) / (float)H.  Without the flag: ux_s = x0 + ox_s.  With
 *    RM_PATTERN_CUMULATIVE: ux_0 = x0 + ox_0 and ux_s = ux_(s-1) + ox_s.  y is
 *    formed the same way.
 *  - Sample.  c_s = render(castRay(ux_s, uy_s)).  This is what a SHADE trace of
 *    that ray returns (rm_trace_rays with RM_TRACE_SHADE).
 *  - Pixel.  sum = c_0; sum = sum + c_s for s = 1..n-1 in order;
 *    out = sum / (float)n; alpha 1.0f.  RGBA8 is the usual quantisation of out
 *    (round(clamp(c, 0, 1) * 255), NaN -> 0).
 *  - Two anchors follow from the rule.  RM_PATTERN_REFERENCE gives the AA-on
 *    rm_dispatch frame bit for bit: 2 * 0.125f is exactly the shader's 0.25.
 *    n = 1, dx = dy = 0 gives the AA-off frame.
 *
 *  - Validation: struct_size is sizeof(rm_sample_pattern), flags has no unknown
 *    bit, n is in 1..RM_MAX_SAMPLES, and every read offset (index < n) is finite
 *    with |d| <= 16; otherwise RM_ERR_INVALID, with the reason in rm_last_error
 *    for rm_dispatch_pattern.  Entries past n are not read.
 *  - u.AA is ignored and the context's uniforms stay as they are; bounceVar,
 *    shadow_mode, iTime, the light and the camera apply as in rm_dispatch.
 *  - Afterwards the context reads as after an rm_dispatch (rm_read_rgba8 /
 *    _rgba32f, rm_get_output_rgba8, rm_set_output_rgba8, rm_wait_output,
 *    rm_set_stream, rm_synchronize).  Nothing is sticky: the next rm_dispatch is
 *    what it always was.  With rm_enable_timing the call is one bracketed launch.
 *    The pattern's uv table is uploaded when the pattern differs from the last
 *    call's; a repeated pattern uploads nothing.
 *  - This version: one-device, whole-frame contexts; the built-in scene and
 *    rm_set_scene tables (with rm_scene_specialize on the generic table code
 *    renders, as the adaptive refinement does: same values).  RM_ERR_STATE on a
 *    context with counters, nshards > 1, a communicator, ngpus >= 1,
 *    RM_OUT_GBUFFER or rm_graph_enable on; no batches, no graph replay.
 *    (Pattern refinement in the adaptive calls: the next section.  A sum kept
 *    across calls: progressive accumulation, the section after it.) */
#define RM_HAS_SAMPLE_PATTERN 1
#define RM_MAX_SAMPLES 16
#define RM_PATTERN_CUMULATIVE 1u      /* flags: offsets are increments, the GLSL's x += o / W */
typedef struct rm_sample_pattern {    /* 140 bytes */
  uint32_t struct_size;               /* sizeof(rm_sample_pattern), else RM_ERR_INVALID */
  uint32_t flags;                     /* 0 or RM_PATTERN_CUMULATIVE; unknown bits: RM_ERR_INVALID */
  int32_t  n;                         /* 1..RM_MAX_SAMPLES */
  float    dx[RM_MAX_SAMPLES];        /* pixels, from the AA-off frame's ray (rm_pick's) */
  float    dy[RM_MAX_SAMPLES];
} rm_sample_pattern;
/* presets: every offset is a dyadic rational, so 2 d is exact */
#define RM_PATTERN_REFERENCE 0  /* n 4, CUMULATIVE, dx {.125,.375,.125,.375}, dy {.125,.125,.375,.375} */
#define RM_PATTERN_GRID2     1  /* n 4,  {-.25,+.25}^2, x fastest */
#define RM_PATTERN_RGSS      2  /* n 4,  (.125,.375) (-.375,.125) (.375,-.125) (-.125,-.375) */
#define RM_PATTERN_GRID3     3  /* n 9,  {-.34375, 0, +.34375}^2 (11/32: the multiple of 1/32 nearest 1/3), x fastest */
#define RM_PATTERN_GRID4     4  /* n 16, {-.375,-.125,+.125,+.375}^2, x fastest */
/* struct_size, flags, n and the offsets of a preset, the entries past n zero.
 * RM_ERR_INVALID for NULL or an unknown preset (nothing written). */
int rm_sample_pattern_init(rm_sample_pattern *p, int32_t preset);
/* The uv of every pixel column and row by the rule above: uvx [width][n], uvy
 * [height][n], either possibly NULL.  Pure: no context, no device.
 * RM_ERR_INVALID for an invalid pattern or a width / height outside 1..65536. */
int rm_pattern_uv_table(const rm_sample_pattern *p, int32_t width, int32_t height,
                        float *uvx, float *uvy);
/* The frame of the pattern.  RM_ERR_INVALID for a null context or pattern
 * (nothing written) or an invalid pattern.  Asynchronous. */
int rm_dispatch_pattern(rm_ctx *ctx, const rm_sample_pattern *p);

/* ---- pattern refinement: the adaptive calls with a sample pattern's samples ------
 * An extension that joins the two above.  The frame of these calls is the AA-off
 * frame with every FLAGGED pixel replaced by that pixel of the frame
 * rm_dispatch_pattern(ctx, pattern) would render with the same uniforms and scene.
 * Every pixel is therefore exactly one of two values defined above: pass 1's
 * pixel (the centre ray), or the sample-pattern rule's pixel (uv from
 * rm_pattern_uv_table, c_s a SHADE trace, sum = c_0, sum = sum + c_s in order,
 * / (float)n, alpha 1, the usual RGBA8 quantisation), bit for bit in RGBA32F and
 * byte for byte in RGBA8.  With a centred pattern a refined pixel registers with
 * the G-buffer record of its centre ray, which the reference's shifted samples of
 * rm_dispatch_adaptive_edges do not.
 *
 *  - Three anchors follow.  RM_PATTERN_REFERENCE gives rm_dispatch_adaptive_edges'
 *    (or rm_dispatch_refine's) frame.  One sample at (0, 0) gives the AA-off frame
 *    whatever is flagged.  An all-ones mask gives the rm_dispatch_pattern frame.
 *  - Flagging, rm_dispatch_adaptive_pattern: rm_dispatch_adaptive_edges' rule, word
 *    for word, with its validation of the criteria, its context requirements (the
 *    geometric criteria need RM_OUT_GBUFFER, the context a colour output) and its
 *    order of checks.  COLOR alone works on plain contexts, so the call covers
 *    rm_dispatch_adaptive's rule too.
 *  - Flagging, rm_dispatch_refine_pattern / _device: rm_dispatch_refine's rule (a
 *    non-zero byte flags, row_pitch 0 = width, the device mask may be the
 *    context's own copy).  Unlike rm_dispatch_refine they admit G-buffer contexts
 *    (a G-buffer criterion of the caller's own); pass 1 then writes the records,
 *    as in rm_dispatch_adaptive_edges.
 *  - Afterwards the context reads as after rm_dispatch_adaptive_edges: on a
 *    G-buffer context the G-buffer holds pass 1's records for every pixel, and
 *    rm_read_aa_mask, rm_get_aa_mask and rm_aa_refined serve the call.  Nothing is
 *    sticky, u.AA is ignored and the uniforms stay.  With rm_enable_timing one
 *    event pair brackets pass 1 through the refinement, one launch of one frame;
 *    the pattern's uv table, which these calls share with rm_dispatch_pattern (a
 *    repeated pattern uploads nothing, across both kinds of call), is uploaded
 *    before the pair.
 *  - Errors: RM_ERR_INVALID for a null context (nothing is touched), for a null or
 *    invalid pattern (the sample patterns' validation, the reason in rm_last_error
 *    after the call's name), and for the criteria or the mask as in the calls
 *    above.  RM_ERR_STATE, naming the call, on a context with counters, nshards >
 *    1, a communicator, ngpus >= 1 or rm_graph_enable on.
 *  - RM_AA_REFINE_WAVES overrides the refinement's grid as above; without it a
 *    pattern of one sample, whose wave takes 64 list entries instead of 16, gets
 *    min(ceil(W H / 64), 128 x compute units) workgroups.
 *  - Out of scope in this version: batches, graph replay, shards,
 *    hiprtc-specialised refine kernels (the generic table code refines, same
 *    values), accumulation across calls in these calls (rm_dispatch_accumulate
 *    sums whole pattern frames; a refined pixel would need a count of its own). */
#define RM_HAS_ADAPTIVE_PATTERN 1
/* rm_dispatch_adaptive_edges with `pattern`'s samples on the flagged pixels.  Asynchronous. */
int rm_dispatch_adaptive_pattern(rm_ctx *ctx, const rm_aa_criteria *criteria, const rm_sample_pattern *pattern);
/* rm_dispatch_refine / _device with `pattern`'s samples on the flagged pixels; the
 * host mask is uploaded synchronously, the frame is asynchronous. */
int rm_dispatch_refine_pattern(rm_ctx *ctx, const uint8_t *mask, size_t row_pitch, const rm_sample_pattern *pattern);
int rm_dispatch_refine_pattern_device(rm_ctx *ctx, const void *mask_dev, size_t row_pitch,
                                      const rm_sample_pattern *pattern);

/* ---- progressive accumulation: sample sums kept across dispatches -----------------
 * An extension to the sample patterns.  rm_dispatch_accumulate renders a pattern's
 * samples and adds them onto a sum the context keeps, so that a frame is the mean
 * of every sample since the sum was last restarted: more than RM_MAX_SAMPLES
 * samples per pixel for a converging still image, and, with a uniform changed
 * between calls, soft shadows from a moved light, motion blur over iTime or depth
 * of field from a moved camera.
 *
 * The rule.  A context gets two new pieces of state.
 *
 *  - The sum image.  [height][width] float4, 16-byte aligned.  It is allocated on
 *    the first accumulating call.
 *  - A host-side sample count N.  int64, 0 after rm_create.
 *
 * rm_dispatch_accumulate(ctx, pattern, flags) renders the pattern's n samples of
 * every pixel exactly as rm_dispatch_pattern does.  The uv comes from
 * rm_pattern_uv_table.  c_s is the SHADE trace of that ray.  The call uses the
 * context's current uniforms and scene.  Then, per pixel and per channel, it
 * performs these steps.  Each one is a single IEEE single-precision operation in
 * this order, with no FMA.
 *
 *  - If N == 0:
 *     - S = c_0;
 *     - then S = S + c_s for s = 1..n-1.
 *  - Otherwise S = S + c_s for s = 0..n-1.
 *     - The stored sum is added first, then the samples in pattern order.
 *  - N = N + n.
 *  - out = S / (float)N, alpha 1.0f.
 *     - RGBA8 is the usual quantisation of out.
 *     - (float)N is the int64-to-float conversion, round to nearest even.  It is
 *       formed on the host.
 *  - The sum image's pixel becomes (S.r, S.g, S.b, (float)N).
 *     - A caller's own shader can therefore resolve it as rgb / w.
 *
 * Three anchors follow from the rule, and the tests rest on them.
 *
 *  1. With N == 0, one call gives the rm_dispatch_pattern(pattern) frame bit for
 *     bit.
 *     - S = c_0, not 0 + c_0, so a -0.0f sample stays -0.0f.
 *  2. Take calls with absolute (non-cumulative) patterns p1, p2, ... whose
 *     concatenation is a valid pattern p (total <= 16).  They give the
 *     rm_dispatch_pattern(p) frame bit for bit.
 *     - This holds however the samples are split, including sixteen n = 1 calls.
 *  3. Past 16 samples the frame is a numpy float32 running sum of SHADE traces,
 *     taken in call order and then sample order.
 *
 * Nothing resets the sum but the caller.
 *
 *  - The uniforms and the scene may change between calls, and each call adds what
 *    it renders under them.
 *  - This is how motion blur, lens blur and area lights are obtained, and it is
 *    documented behaviour, not an accident.
 *  - The sum is touched only by rm_dispatch_accumulate and rm_accum_reset.
 *     - rm_dispatch, rm_dispatch_frames, rm_dispatch_pattern and the adaptive calls
 *       overwrite the colour images as always and leave S and N alone.
 *     - The next accumulating call continues and rewrites the colour images from
 *       S / N.
 *  - Every accumulating call reads the sum the one before it wrote, on the
 *    context's stream.  rm_set_stream waits only when it leaves the context's
 *    own stream: a caller who moves the context from one stream of theirs to
 *    another (or back to its own) between accumulating calls orders the new
 *    stream behind the old one first, for example with rm_wait_output on the
 *    new stream before rm_set_stream.
 *
 * Contexts and errors of rm_dispatch_accumulate are rm_dispatch_pattern's:
 * RM_ERR_STATE, naming the call, on a context with counters, nshards > 1, a
 * communicator, ngpus >= 1, RM_OUT_GBUFFER or rm_graph_enable on; RM_ERR_INVALID
 * for a null context or pattern (nothing is touched), for an invalid pattern (the
 * sample patterns' validation, the reason in rm_last_error after the call's name)
 * and for an unknown flag bit.  A call that fails leaves S and N as they were.
 * Afterwards the context reads as after rm_dispatch_pattern (the readbacks,
 * rm_get_output_rgba8 / rm_set_output_rgba8, rm_wait_output, rm_set_stream,
 * rm_synchronize); u.AA is ignored and the uniforms stay; with rm_enable_timing the
 * call is one bracketed launch; the pattern's uv table is the one
 * rm_dispatch_pattern and the pattern refinements share, so a repeated pattern
 * uploads nothing.  The built-in scene and rm_set_scene tables are served; with
 * rm_scene_specialize on the generic table code renders, with the same values.
 *
 * Out of scope in this version: accumulation in the adaptive and refine calls (it
 * needs per-pixel counts; the w channel is where they would go), batches, graph
 * replay, shards and G-buffer contexts, a hiprtc-specialised accumulation kernel,
 * exponential blends and per-sample weights, variance or convergence estimates,
 * loading a saved sum back into a context. */
#define RM_HAS_ACCUMULATION 1
#define RM_ACCUM_RESTART 1u   /* flags: N = 0 first, so the call's samples replace the sum */
/* The pattern's samples added onto the sum, and the frame S / N.  Asynchronous. */
int rm_dispatch_accumulate(rm_ctx *ctx, const rm_sample_pattern *pattern, uint32_t flags);
/* N = 0; no device work; the old sum is never read again.  RM_ERR_INVALID for a null context. */
int rm_accum_reset(rm_ctx *ctx);
/* N; no synchronisation.  RM_ERR_INVALID for a null context or output (nothing written). */
int rm_accum_samples(const rm_ctx *ctx, int64_t *samples);
/* The sum image, by the layout rules of rm_read_rgba32f (row_pitch in bytes, 0 = a
 * row; flip_y).  Synchronous.  RM_ERR_STATE while N == 0. */
int rm_read_accum(rm_ctx *ctx, float *dst, size_t row_pitch, int flip_y);
/* The sum image on the device, allocated on first use, whatever N is; its contents
 * are undefined while N == 0.  Order reads after the context's stream
 * (rm_wait_output).  RM_ERR_STATE on the contexts rm_dispatch_accumulate refuses. */
int rm_get_accum(rm_ctx *ctx, void **device_ptr);
/* A pattern of n points of the Halton sequence in bases 2 and 3, re-centred on the
 * pixel, so that callers do not each invent a sequence: struct_size, flags = 0, n,
 * the entries past n zero, and for sample s, with index i = first + s + 1,
 *   dx[s] = (float)(R(i, 2) - 0.5),  dy[s] = (float)(R(i, 3) - 0.5).
 * R(i, b) is computed in double, each operation one IEEE double operation in the
 * order written:
 *   f = 1.0 / b; r = 0.0; while (i > 0) { r = r + (double)(i % b) * f; i = i / b; f = f / (double)b; }
 * (the product and the sum are separate operations).  Pure host: no context, no
 * device.  RM_ERR_INVALID, with nothing written, for NULL, n outside
 * 1..RM_MAX_SAMPLES or first outside 0..2^40. */
int rm_sample_pattern_halton(rm_sample_pattern *p, int64_t first, int32_t n);

/* ---- one rank per process: RCCL-gathered frames -------------
 * The multi-process form of rm_config.ngpus, for hosts that run one process
 * per GPU (torch.distributed.run, MPI).  Rank 0 creates an id and broadcasts it
 * over the host's own channel; every rank then joins its sharded context
 * (cfg.nshards = nranks, cfg.shard = rank) to the communicator
 * (ncclCommInitRank: collective, every rank must call it).  From then on
 * rm_dispatch renders this rank's shard, gathers all shards on rank 0
 * (ncclGather into rank 0's [nranks][rows_cap][width] buffer; rank 0 renders
 * its own shard in place) and, on rank 0, assembles the frame (k_unshard), all
 * on the context's stream.  Rank 0's rm_read_rgba8 / rm_read_rgba32f /
 * rm_get_output_rgba8 / rm_set_output_rgba8 then refer to the full height x
 * width frame, the other ranks' to their packed shard; an output buffer set on
 * rank 0 before rm_comm_init (shard-sized) is dropped, so set or re-query output
 * pointers after it.  rm_dispatch and rm_graph_dispatch are collective: every
 * rank issues the same sequence.  rm_graph_dispatch captures render + gather +
 * assembly into one hipGraph per rank (cfg 5).  RGBA8 and/or RGBA32F (16 B/px
 * shards gathered as ncclFloat32), no counters.
 *
 * Failure detection: communicators are non-blocking; rm_comm_init, and every
 * wait on the context afterwards, polls progress and ncclCommGetAsyncError
 * against a deadline (rm_comm_set_timeout; default 120000 ms or the
 * RM_COMM_TIMEOUT_MS environment variable; 0 = none).  A rank that never
 * joins, an RCCL error or a frame that misses the deadline aborts the
 * communicator (ncclCommAbort) and returns RM_ERR_COMM with the reason in
 * rm_last_error; the process and its other contexts stay usable. */
#define RM_COMM_ID_BYTES 128 /* == NCCL_UNIQUE_ID_BYTES */
int rm_comm_unique_id(void *id, size_t size);
int rm_comm_init(rm_ctx *ctx, const void *id, int32_t nranks, int32_t rank);
/* Deadline in ms of rm_comm_init and of every later wait on the context. */
int rm_comm_set_timeout(rm_ctx *ctx, int32_t timeout_ms);
/* Non-blocking health check: RM_OK, or RM_ERR_COMM when the communicator has
 * an asynchronous error (it is then aborted) or was aborted before. */
int rm_comm_check(rm_ctx *ctx);
/* The context's communicator: rank / size (0 / 1 without one), and the devices
 * a multi-GPU context drives (*ngpus = 1 for a one-GPU context). */
int rm_comm_info(const rm_ctx *ctx, int32_t *rank, int32_t *nranks, int32_t *ngpus);
/* What RCCL itself reports for the context's communicator (API version 4):
 * ncclCommCount, ncclCommUserRank and ncclCommCuDevice of the communicator
 * (device 0's for a multi-GPU context, whose every device is checked to be user
 * rank i of ngpus on its own device) and ncclGetVersion.  RM_ERR_COMM when RCCL's
 * view differs from the context's (rank, nranks, device).  Without a
 * communicator: *count = 0, *user_rank = *hip_device = -1, *version = 0.  Any
 * pointer may be NULL. */
int rm_comm_rccl_info(rm_ctx *ctx, int32_t *count, int32_t *user_rank, int32_t *hip_device,
                      int32_t *version);

/* ---- row sharding helpers (pure functions) ------------------------------- */
/* The weighted interleave (API version 5).  Rows go in rounds of
 * P = rank0_rows + (nshards - 1) row_block rows: shard 0 owns rows
 * [kP, kP + rank0_rows) of round k, shard s >= 1 the row_block rows after
 * rank0_rows + (s - 1) row_block.  Shard s's rows are packed in round order into
 * a [rows_cap][width] image; rows_cap (the same for every shard, so one
 * ncclGather moves them) is the largest shard's rounds times its rows per round,
 * and *rows is shard s's own count of real rows.  rank0_rows = 0 means
 * row_block (the plain interleave: block b belongs to shard b % nshards).
 * nshards <= 1: the whole image (rows = rows_cap = height).
 * Every function below takes (height, row_block, rank0_rows, nshards, ...) in
 * this order (API version 6; version 5's rm_shard_row took shard before nshards,
 * and version 1's rm_shard_rows_cap / rm_shard_global_row knew only the plain
 * interleave: all three are gone, so a stale caller fails to bind instead of
 * reading the wrong rows). */
int rm_shard_rows(int32_t height, int32_t row_block, int32_t rank0_rows, int32_t nshards, int32_t shard,
                  int32_t *rows, int32_t *rows_cap);
/* Global row (py) of local row `local_row` of shard `shard`; -1 if padding or
 * out of range (including invalid arguments). */
int32_t rm_shard_to_global(int32_t height, int32_t row_block, int32_t rank0_rows, int32_t nshards, int32_t shard,
                           int32_t local_row);
/* The inverse: the shard and local row that own global row `row`. */
int rm_shard_owner(int32_t height, int32_t row_block, int32_t rank0_rows, int32_t nshards, int32_t row,
                   int32_t *shard, int32_t *local_row);

/* ---- Camera (source/camera.{hpp,cpp}), glm-free, same formulas ----------- */
typedef struct rm_camera_state { /* members of camera.hpp:14-27 */
  int32_t width, height;
  float angleY, angleX;
  float mouseSensitivity, keyboardSpeed;
  float xpos, ypos;
  float cameraPos[3];
  float forward[3];
  float up[3];
  float right[3];
} rm_camera_state;

/* Camera::Camera(w,h,sens,speed,pos,lookAt,up)  camera.cpp:8-14 */
int rm_camera_init(rm_camera_state *c, int32_t width, int32_t height, float mouseSensitivity,
                   float keyboardSpeed, const float pos[3], const float lookAt[3],
                   const float up[3]);
/* Camera::setMouse                              camera.cpp:16-20 */
int rm_camera_set_mouse(rm_camera_state *c, float x, float y);
/* Camera::lookAt                                camera.cpp:22-51 */
int rm_camera_look_at(rm_camera_state *c, int zN, int zP, int xN, int xP, int halfSpeed,
                      float deltaTime);
/* The four setVec4 calls of main.cpp:103-106 (w = 0). */
int rm_camera_to_uniform(const rm_camera_state *c, rm_camera *out);

/* ---- interactive input mapping ------------------------
 * The reference's GLFW input globals and callbacks (main.cpp:20-39, 93-95,
 * 155-234; source/MousePosition.cpp:4-22) as a state struct and four event
 * functions, so any windowing front-end can feed its key/mouse events and get
 * the reference's camera motion, bounce/AA toggles and uniforms.  Key and
 * action codes are GLFW's (glfw3.h) so a GLFW front-end passes them through. */
#define RM_KEY_A 65
#define RM_KEY_D 68
#define RM_KEY_L 76
#define RM_KEY_S 83
#define RM_KEY_W 87
#define RM_KEY_ESCAPE 256
#define RM_KEY_DOWN 264
#define RM_KEY_UP 265
#define RM_KEY_F1 290
#define RM_RELEASE 0
#define RM_PRESS 1
#define RM_REPEAT 2
/* keys held this frame (glfwGetKey(...) == GLFW_PRESS), for rm_input_process */
#define RM_HELD_W 1u
#define RM_HELD_A 2u
#define RM_HELD_S 4u
#define RM_HELD_D 8u
#define RM_HELD_ESCAPE 16u

typedef struct rm_input_state {
  int32_t zaxisPos, zaxisNeg, xaxisPos, xaxisNeg; /* main.cpp:23-26 */
  int32_t AA;                                     /* main.cpp:27 (true) */
  int32_t showQuad;                               /* main.cpp:28 wireframe toggle (display only) */
  float halfSpeed;                                /* main.cpp:29 (a float in the reference) */
  int32_t bounce;                                 /* main.cpp:30, 0..5 */
  float deltaTime, lastFrame;                     /* main.cpp:32-33 */
  float lastX, lastY;                             /* main.cpp:35-36 (screen centre) */
  int32_t firstMouse;                             /* main.cpp:37 */
  float pitch, yaw;                               /* MouseInput mouse, main.cpp:39 */
  float mouseSensitivity;                         /* MouseSensitivity, MousePosition.hpp:8 */
  int32_t shouldClose;                            /* glfwSetWindowShouldClose (main.cpp:157) */
} rm_input_state;

/* The globals' initial values for a screen_width x screen_height window. */
int rm_input_init(rm_input_state *s, int32_t screen_width, int32_t screen_height);
/* main.cpp:93-95: currentFrame = (float)now; deltaTime = currentFrame - lastFrame. */
int rm_input_begin_frame(rm_input_state *s, double now_seconds);
/* processInput  main.cpp:155-195: axis flags and halfSpeed from the held keys
 * (RM_HELD_*), ESC -> shouldClose, then camera.lookAt(..., deltaTime). */
int rm_input_process(rm_input_state *s, uint32_t held, rm_camera_state *cam);
/* key_callback  main.cpp:197-217: UP/DOWN bounce within 0..5, F1 toggles AA,
 * L toggles showQuad; only RM_PRESS acts (repeats are ignored). */
int rm_input_key(rm_input_state *s, int32_t key, int32_t action);
/* mouse_callback  main.cpp:219-234: MouseInput offsets, camera.setMouse(-x, -y). */
int rm_input_mouse(rm_input_state *s, double xpos, double ypos, rm_camera_state *cam);
/* MouseInput::EulerAngles  MousePosition.cpp:24-33 (the "mouse" uniform). */
int rm_input_euler_angles(const rm_input_state *s, float out[3]);
/* The per-frame uploads of main.cpp:101-120 that input drives: camera block,
 * AA, bounceVar, mouse = EulerAngles(), iMouse = (yaw, pitch), and
 * iTime = the frame's clock sample (lastFrame).  Other fields are untouched. */
int rm_input_to_uniforms(const rm_input_state *s, const rm_camera_state *cam, rm_uniforms *u);

/* ---- synthetic frames -------------------------------------- */
/* Sweep S(F): camera at (0,0,15), yaw -20..+20 deg over F frames, pitch -5 deg,
 * iTime = f/60; lights of main.cpp:108-114. frame < 0 selects the default
 * frame D (start-up view: pos 0, yaw = pitch = 0, iTime = 0). */
int rm_sweep_uniforms(int32_t frame, int32_t nframes, int32_t bounceVar, int32_t AA,
                      int32_t shadow_mode, rm_uniforms *out);

#ifdef __cplusplus
}
#endif

#endif /* RM_API_H */
