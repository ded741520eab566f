// rm_api_comm.hip — librm's RCCL-gathered frames: everything that touches a
// communicator.  The bounded waits and the abort, a multi-GPU context
// (rm_config.ngpus) and one rank per process (rm_comm_init), the gather and
// rank 0's assembly, the two-slot batch pipeline, and the rm_comm_* entry points.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdlib>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "rm_ctx.hpp"

using namespace rm;

namespace {

int nccl_fail(rm_ctx* c, const rm::Rccl* r, ncclResult_t e, const char* what) {
  return fail(c, RM_ERR_COMM, std::string(what) + ": " + (r ? r->GetErrorString(e) : "RCCL"));
}

// The contexts whose communicators one frame uses: a multi-GPU context's devices,
// or the context itself.
std::vector<rm_ctx*> comm_members(rm_ctx* c) {
  if (!c->subs.empty()) return c->subs;
  return {c};
}

int comm_abort(rm_ctx* c, const std::string& why) {
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  for (rm_ctx* m : comm_members(c)) {
    if (m->comm && r) {
      (void)hipSetDevice(m->device);
      (void)r->CommAbort(m->comm);  // pending collectives see the abort flag and quit
    }
    m->comm = nullptr;
    m->comm_failed = true;
    m->comm_why = why;
  }
  c->comm_failed = true;
  c->comm_why = why;
  return fail(c, RM_ERR_COMM, why);
}

}  // namespace

namespace rm {

// ---- communicator failure detection --------------------------------------
// Every wait on a communicator context is a bounded poll: the stream's progress
// (hipStreamQuery) and the communicator's asynchronous error
// (ncclCommGetAsyncError), against c->comm_timeout_ms.  An RCCL error or a missed
// deadline (a peer that died, stalled or never joined) aborts the communicator
// (ncclCommAbort: the pending collectives quit) and the context reports
// RM_ERR_COMM from then on; it can still be read for its error and destroyed.
long default_comm_timeout_ms() {
  const char* s = std::getenv("RM_COMM_TIMEOUT_MS");
  if (s && *s) {
    char* end = nullptr;
    const long v = std::strtol(s, &end, 10);
    if (end && *end == '\0' && v >= 0) return v;
  }
  return 120000;
}

// A communicator context whose communicator was aborted.
int comm_dead(rm_ctx* c) {
  return fail(c, RM_ERR_COMM, "the communicator was aborted: " + c->comm_why);
}

// Waits until every stream of the frame's contexts has drained, polling the
// communicators' asynchronous errors, within the context's deadline.
// (the caller's current device is restored: a multi-GPU context's wait visits
// every device)
int comm_wait(rm_ctx* c) {
  const KeepDevice keep;
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, err);
  const std::vector<rm_ctx*> ms = comm_members(c);
  const long tmo = c->comm_timeout_ms;
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<bool> done(ms.size(), false);
  for (int spins = 0;; ++spins) {
    bool all = true;
    for (size_t i = 0; i < ms.size(); ++i) {
      if (done[i]) continue;
      rm_ctx* m = ms[i];
      (void)hipSetDevice(m->device);
      // the render stream and, after a batch, the gather stream
      hipError_t q = hipStreamQuery(m->stream);
      if (q == hipSuccess && m->gstream) q = hipStreamQuery(m->gstream);
      if (q == hipSuccess) {
        done[i] = true;
        continue;
      }
      if (q != hipErrorNotReady) return hip_fail(c, q, "hipStreamQuery");
      all = false;
      if (m->comm) {
        ncclResult_t st = ncclSuccess;
        const ncclResult_t e = r->CommGetAsyncError(m->comm, &st);
        if (e != ncclSuccess || (st != ncclSuccess && st != ncclInProgress))
          return comm_abort(c, std::string("RCCL asynchronous error on device ") + std::to_string(m->device) +
                                   ": " + r->GetErrorString(e != ncclSuccess ? e : st));
      }
    }
    if (all) return RM_OK;
    if (tmo > 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(tmo))
      return comm_abort(c, "the frame did not complete within " + std::to_string(tmo) +
                               " ms (rm_comm_set_timeout): a peer rank stalled, failed or never issued "
                               "its gather");
    rm::poll_pause(spins);
  }
}

// The communicators of a context being freed (its own, or its devices'), torn
// down together and within the deadline (rm_comm.cpp teardown).
void comm_teardown(rm_ctx* c) {
  std::vector<ncclComm_t> cs;
  for (rm_ctx* m : comm_members(c))
    if (m->own_comm && m->comm) {
      cs.push_back(m->comm);
      m->comm = nullptr;
    }
  std::string err;
  const rm::Rccl* r = cs.empty() ? nullptr : rm::rccl(&err);
  if (r) {
    const KeepDevice keep;
    rm::teardown(r, cs.data(), (int)cs.size(), c->comm_timeout_ms);
  }
}

}  // namespace rm

namespace {

// Waits for an RCCL call that returned ncclInProgress (non-blocking communicator).
int comm_enqueued(rm_ctx* c, const rm::Rccl* r, ncclResult_t e, const char* what) {
  if (e == ncclSuccess) return RM_OK;
  // an enqueue error aborts the communicator (rm_api.h: RM_ERR_COMM means aborted);
  // a partial group may already have launched gathers that would wait forever
  if (e != ncclInProgress) return comm_abort(c, std::string(what) + ": " + r->GetErrorString(e));
  std::vector<ncclComm_t> cs;
  for (rm_ctx* m : comm_members(c))
    if (m->comm) cs.push_back(m->comm);
  const ncclResult_t w = rm::wait_ready(r, cs.data(), (int)cs.size(), c->comm_timeout_ms);
  if (w == ncclSuccess) return RM_OK;
  if (w == ncclInProgress)
    return comm_abort(c, std::string(what) + ": not enqueued within " + std::to_string(c->comm_timeout_ms) + " ms");
  return comm_abort(c, std::string(what) + ": " + r->GetErrorString(w));
}

// Joins a sharded context to a communicator as `rank` of `n`: rank 0 gets the
// gather buffers (its shard renders into slot 0, so ncclGather runs in place) and
// the assembled frames, one pair per enabled output format.  Rank 0's readable
// image changes from its shard to the full frame, so a caller-set RGBA8 output
// (sized for the shard) is dropped: output pointers are set, or re-queried, after
// rm_comm_init (include/rm_api.h).
int comm_attach(rm_ctx* c, ncclComm_t comm, int rank, int n, bool own, bool member) {
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  c->comm = comm;
  c->own_comm = own;
  c->group_member = member;
  c->crank = rank;
  c->cranks = n;
  c->comm_failed = false;
  // the gathered shards travel as packed RGB unless the config asks for RGBA8
  if ((c->cfg.outputs & RM_OUT_RGBA8) && c->cfg.shard_format == RM_SHARD_AUTO) c->rgb3 = true;
  if (rank == 0) {
    const size_t px_shard = (size_t)c->rows * c->cfg.width, px_frame = (size_t)c->cfg.height * c->cfg.width;
    if (c->cfg.outputs & RM_OUT_RGBA8) {
      RM_HIP(c, hipMalloc(&c->d_gathered, px_shard * 4 * n));
      RM_HIP(c, hipMalloc(&c->d_frame, px_frame * 4));
      RM_HIP(c, hipMemsetAsync(c->d_gathered, 0, px_shard * 4 * n, c->stream));
      RM_HIP(c, hipMemsetAsync(c->d_frame, 0, px_frame * 4, c->stream));
    }
    if (c->cfg.outputs & RM_OUT_RGBA32F) {
      RM_HIP(c, hipMalloc(&c->d_gathered32, px_shard * 16 * n));
      RM_HIP(c, hipMalloc(&c->d_frame32, px_frame * 16));
      RM_HIP(c, hipMemsetAsync(c->d_gathered32, 0, px_shard * 16 * n, c->stream));
      RM_HIP(c, hipMemsetAsync(c->d_frame32, 0, px_frame * 16, c->stream));
    }
    RM_HIP(c, hipStreamSynchronize(c->stream));
    // rank 0 renders into the gather buffers
    if (c->d_rgba8) (void)hipFree(c->d_rgba8);
    if (c->d_rgba32f) (void)hipFree(c->d_rgba32f);
    c->d_rgba8 = nullptr;
    c->d_rgba32f = nullptr;
    c->ext_rgba8 = nullptr;  // a shard-sized caller buffer cannot hold the frame
  }
  graph_release(c);
  return RM_OK;
}

int check_comm_config(const rm_config& cfg, const char* who) {
  if (cfg.outputs & RM_OUT_GBUFFER)
    return fail(nullptr, RM_ERR_INVALID, std::string(who) + ": RM_OUT_GBUFFER is not available for "
                                         "RCCL-gathered frames (a one-device context only)");
  if ((cfg.outputs & ~(RM_OUT_RGBA8 | RM_OUT_RGBA32F)) != 0 || cfg.counters)
    return fail(nullptr, RM_ERR_INVALID, std::string(who) + ": RCCL-gathered frames are RGBA8 and/or "
                                         "RGBA32F, without counters");
  return RM_OK;
}

}  // namespace

namespace rm {

// rm_config.ngpus >= 1: one shard context per device plus a single-process
// communicator over the devices (one ncclCommInitRankConfig per device inside a
// group, non-blocking, waited for within the deadline).
int create_multi(rm_ctx** out, const rm_config* cfg) {
  const int n = cfg->ngpus;
  int rc = check_comm_config(*cfg, "rm_create");
  if (rc != RM_OK) return rc;
  if (cfg->nshards > 1 || cfg->shard != 0)
    return fail(nullptr, RM_ERR_INVALID, "rm_create: ngpus shards by itself (shard/nshards must be 0)");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    return fail(nullptr, RM_ERR_NO_DEVICE, "rm_create: no HIP device (librm has no CPU fallback)");
  std::vector<int> devs(n);
  int d0 = cfg->device;
  if (d0 < 0 && hipGetDevice(&d0) != hipSuccess) d0 = 0;
  for (int i = 0; i < n; ++i) {
    devs[i] = cfg->devices ? cfg->devices[i] : d0 + i;
    if (devs[i] < 0 || devs[i] >= ndev)
      return fail(nullptr, RM_ERR_INVALID, "rm_create: device " + std::to_string(devs[i]) +
                                               " out of range (" + std::to_string(ndev) + " devices)");
    for (int j = 0; j < i; ++j)
      if (devs[j] == devs[i])
        return fail(nullptr, RM_ERR_INVALID, "rm_create: devices must be distinct (one shard per GPU)");
  }
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(nullptr, RM_ERR_COMM, "rm_create: " + err);
  rm_ctx* c = new (std::nothrow) rm_ctx();
  if (!c) return fail(nullptr, RM_ERR_NOMEM, "rm_create: out of host memory");
  c->cfg = *cfg;
  if (c->cfg.outputs == 0) c->cfg.outputs = RM_OUT_RGBA8;
  c->cfg.row_block = cfg->row_block > 0 ? cfg->row_block : 8;
  c->cfg.nshards = n;
  c->cfg.shard = 0;
  c->cfg.devices = nullptr;  // not kept: the caller owns the array
  c->device = devs[0];
  c->rows = c->cfg.height;
  c->comm_timeout_ms = default_comm_timeout_ms();
  rm_default_uniforms(&c->u);
  for (int i = 0; i < n; ++i) {
    rm_config sc = c->cfg;
    sc.ngpus = 0;
    sc.device = devs[i];
    sc.shard = i;
    rm_ctx* sub = nullptr;
    if ((rc = rm_create(&sub, &sc)) != RM_OK) {
      c->err = "rm_create (device " + std::to_string(devs[i]) + "): " + rm_last_error(nullptr);
      return create_fail(c, rc);
    }
    c->subs.push_back(sub);
  }
  ncclUniqueId id;
  ncclResult_t e = r->GetUniqueId(&id);
  if (e != ncclSuccess) return create_fail(c, nccl_fail(c, r, e, "ncclGetUniqueId"));
  std::vector<ncclComm_t> comms(n, nullptr);
  e = r->GroupStart();
  for (int i = 0; i < n && (e == ncclSuccess || e == ncclInProgress); ++i) {
    ncclConfig_t nb = rm::nonblocking_config();
    (void)hipSetDevice(devs[i]);
    e = r->CommInitRankConfig(&comms[i], n, id, i, &nb);
  }
  const ncclResult_t eg = r->GroupEnd();
  if (e == ncclSuccess || e == ncclInProgress) e = eg;
  if (e == ncclSuccess || e == ncclInProgress) e = rm::wait_ready(r, comms.data(), n, c->comm_timeout_ms);
  if (e != ncclSuccess) {
    for (int i = 0; i < n; ++i)
      if (comms[i]) (void)r->CommAbort(comms[i]);
    c->err = e == ncclInProgress
                 ? "rm_create: the communicator was not ready within " + std::to_string(c->comm_timeout_ms) + " ms"
                 : std::string("rm_create: ncclCommInitRankConfig: ") + r->GetErrorString(e);
    return create_fail(c, RM_ERR_COMM);
  }
  for (int i = 0; i < n; ++i) {
    if ((rc = comm_attach(c->subs[i], comms[i], i, n, true, true)) != RM_OK) {
      //  abort every member, attached or not, and detach them, so the
      // teardown below neither finalizes a half-aborted group (and waits out the
      // deadline) nor leaks comms[i]
      c->err = c->subs[i]->err;
      for (int j = 0; j < n; ++j) {
        (void)hipSetDevice(devs[j]);
        (void)r->CommAbort(comms[j]);
        c->subs[j]->comm = nullptr;
        c->subs[j]->own_comm = false;
      }
      return create_fail(c, rc);
    }
    c->subs[i]->comm_timeout_ms = c->comm_timeout_ms;
  }
  c->stream = c->subs[0]->stream;  // the frame's stream (not owned)
  *out = c;
  return RM_OK;
}

// The gather of one rank (ncclGather to rank 0, in place on rank 0): the RGBA8
// and RGBA32F shards in one group.
int comm_gather(rm_ctx* c) {
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, err);
  const size_t px = (size_t)c->rows * c->cfg.width;
  const bool root = comm_root(c);
  ncclResult_t e = r->GroupStart();
  if (e == ncclSuccess && (c->cfg.outputs & RM_OUT_RGBA8))
    e = r->Gather(render_dst(c), root ? c->d_gathered : nullptr, px * bpp8(c), ncclUint8, 0, c->comm, c->stream);
  if ((e == ncclSuccess || e == ncclInProgress) && (c->cfg.outputs & RM_OUT_RGBA32F))
    e = r->Gather(render_dst32(c), root ? c->d_gathered32 : nullptr, px * 4, ncclFloat32, 0, c->comm,
                  c->stream);
  const ncclResult_t eg = r->GroupEnd();
  if (e == ncclSuccess || e == ncclInProgress) e = eg;
  const int rc = comm_enqueued(c, r, e, "ncclGather");
  if (rc != RM_OK) return rc;
  c->comm_warm = true;
  return RM_OK;
}

// Rank 0: the gathered shards -> the frame (k_unshard), on the same stream.  An
// RGBA32F row is 4 x width 32-bit words: the same row permutation as an RGBA8
// image 4 x as wide.
int comm_assemble(rm_ctx* c) {
  if (!comm_root(c)) return RM_OK;
  if (c->cfg.outputs & RM_OUT_RGBA8) {
    const hipError_t e = rm::launch_unshard(c->d_gathered, image_rgba8(c), c->cfg.width, c->cfg.height,
                                            c->cfg.row_block, row_block0(c), c->cranks, c->rows, c->stream, 0,
                                            c->rgb3);
    if (e != hipSuccess) return hip_fail(c, e, "unshard launch");
  }
  if (c->cfg.outputs & RM_OUT_RGBA32F) {
    const hipError_t e = rm::launch_unshard(c->d_gathered32, c->d_frame32, c->cfg.width * 4, c->cfg.height,
                                            c->cfg.row_block, row_block0(c), c->cranks, c->rows, c->stream);
    if (e != hipSuccess) return hip_fail(c, e, "unshard launch (RGBA32F)");
  }
  return RM_OK;
}

// A multi-GPU context's frame: every device renders its shard (plainly or from
// its render-only graph), one grouped ncclGather collects the shards on device
// 0 (a single-process communicator needs the group), device 0 assembles.
int multi_frame(rm_ctx* c, bool graph) {
  if (c->comm_failed) return comm_dead(c);
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, err);
  const bool timed = !graph && c->subs[0]->timing;
  int rc = RM_OK;
  for (rm_ctx* s : c->subs) {
    s->u = c->u;
    if (timed && (rc = phase(s, 0)) != RM_OK) return fail(c, rc, s->err);
    rc = graph ? graph_frame(s) : render_launch(s);
    if (rc != RM_OK) return fail(c, rc, s->err);
    if (timed && (rc = phase(s, 1)) != RM_OK) return fail(c, rc, s->err);
  }
  ncclResult_t e = r->GroupStart();
  if (e != ncclSuccess) return comm_abort(c, std::string("ncclGroupStart: ") + r->GetErrorString(e));
  std::string why;
  for (rm_ctx* s : c->subs) {
    if ((rc = set_device(s)) != RM_OK || (rc = comm_gather(s)) != RM_OK) {
      why = s->err;
      break;
    }
  }
  e = r->GroupEnd();
  // a partial group: the gathers already queued on some devices can never
  // complete, so the communicator is aborted (not left to the deadline)
  if (rc != RM_OK) return comm_abort(c, "gather (partial group): " + why);
  if ((rc = comm_enqueued(c, r, e, "ncclGroupEnd (gather)")) != RM_OK) return rc;
  rm_ctx* s0 = c->subs[0];
  if ((rc = set_device(s0)) != RM_OK) return fail(c, rc, s0->err);
  if (timed && (rc = phase(s0, 2)) != RM_OK) return fail(c, rc, s0->err);
  if ((rc = comm_assemble(s0)) != RM_OK) return fail(c, rc, s0->err);
  if (timed && (rc = phase(s0, 3)) != RM_OK) return fail(c, rc, s0->err);
  s0->ph_recorded = timed || s0->ph_recorded;
  s0->ph_comm = true;
  c->dispatched = true;
  return RM_OK;
}

}  // namespace rm

// ---- frame batches on a communicator (rm_dispatch_frames) --------------------------
// The n shards of one rank go to a batch slot and move in ONE ncclGather on the
// gather stream; rank 0 assembles the n frames there.  Two slots alternate, so
// batch j + 1 renders while batch j gathers, and all of a communicator's
// collectives stay on one stream in issue order.
namespace {

// A communicator context's batch slot holding n frames: this rank's shards
// ([n][rows][width]), or on rank 0 the whole gather buffer ([nranks][n][rows]
// [width]).  Re-allocated only for a longer batch, after the slot's last
// gather has read it.
int slot_alloc(rm_ctx* c, rm_ctx::BatchSlot& b, int n) {
  if (!b.rendered) RM_HIP(c, hipEventCreateWithFlags(&b.rendered, hipEventDisableTiming));
  if (!b.freed) RM_HIP(c, hipEventCreateWithFlags(&b.freed, hipEventDisableTiming));
  if (b.cap >= n) return RM_OK;
  // the slot's last gather (gstream) and this rank's renders (stream) must be done
  // before its buffers go: on a communicator context that wait is the bounded poll
  // of every other communicator wait (a stalled peer is RM_ERR_COMM at the deadline,
  // ADVICE r04), not an unbounded event / stream synchronise
  if (c->comm) {
    const int rc = comm_wait(c);
    if (rc != RM_OK) return rc;
  } else {
    if (b.pending) RM_HIP(c, hipEventSynchronize(b.freed));
    RM_HIP(c, hipStreamSynchronize(c->stream));
  }
  if (b.send8) (void)hipFree(b.send8);
  if (b.send32) (void)hipFree(b.send32);
  b.send8 = nullptr;
  b.send32 = nullptr;
  b.cap = 0;
  const size_t px = (size_t)c->rows * (size_t)c->cfg.width * (size_t)n * (comm_root(c) ? c->cranks : 1);
  if (c->cfg.outputs & RM_OUT_RGBA8) RM_HIP(c, hipMalloc(&b.send8, px * 4));
  if (c->cfg.outputs & RM_OUT_RGBA32F) RM_HIP(c, hipMalloc(&b.send32, px * 16));
  b.cap = n;
  return RM_OK;
}

// Step 1 of a communicator batch: this rank's n shards in one launch, on the
// context's stream, into the next slot.
int batch_render(rm_ctx* c, const rm_uniforms* u, int n) {
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  if ((rc = order_after_batch(c)) != RM_OK) return rc;
  if (!c->gstream) {
    RM_HIP(c, hipStreamCreateWithFlags(&c->gstream, hipStreamNonBlocking));
    RM_HIP(c, hipEventCreateWithFlags(&c->gdone, hipEventDisableTiming));
  }
  rm_ctx::BatchSlot& b = c->bslot[c->bnext];
  if ((rc = slot_alloc(c, b, n)) != RM_OK) return rc;
  if (comm_root(c) && (rc = ensure_ring(c, n, c->cfg.height)) != RM_OK) return rc;
  // the slot's previous batch (two batches ago) has been gathered and assembled
  if (b.pending) RM_HIP(c, hipStreamWaitEvent(c->stream, b.freed, 0));
  const size_t px = (size_t)c->rows * (size_t)c->cfg.width;
  Timed t;
  if ((rc = t.begin(c)) != RM_OK) return rc;
  if ((rc = phase(c, 0)) != RM_OK) return rc;
  uint8_t* out8[RM_MAX_BATCH];
  float* out32[RM_MAX_BATCH];
  for (int k = 0; k < n; ++k) {
    out8[k] = b.send8 ? b.send8 + (size_t)k * px * bpp8(c) : nullptr;
    out32[k] = b.send32 ? b.send32 + (size_t)k * px * 4 : nullptr;
  }
  if ((rc = launch_batch(c, u, n, out8, out32)) != RM_OK) return rc;
  if ((rc = phase(c, 1)) != RM_OK) return rc;
  if ((rc = t.end(c, n)) != RM_OK) return rc;
  RM_HIP(c, hipEventRecord(b.rendered, c->stream));
  return RM_OK;
}

// Step 2 (inside an RCCL group): the slot's n shards to rank 0 in one gather
// per format, on the gather stream once the render is done.
ncclResult_t batch_gather(rm_ctx* c, const rm::Rccl* r, int n) {
  if (set_device(c) != RM_OK) return ncclUnhandledCudaError;
  rm_ctx::BatchSlot& b = c->bslot[c->bnext];
  if (hipStreamWaitEvent(c->gstream, b.rendered, 0) != hipSuccess) return ncclUnhandledCudaError;
  const size_t px = (size_t)c->rows * (size_t)c->cfg.width * (size_t)n;
  const size_t count = px * 4;  // 4 floats per px
  const bool root = comm_root(c);
  ncclResult_t e = ncclSuccess;
  if (b.send8) e = r->Gather(b.send8, root ? b.send8 : nullptr, px * bpp8(c), ncclUint8, 0, c->comm, c->gstream);
  if ((e == ncclSuccess || e == ncclInProgress) && b.send32)
    e = r->Gather(b.send32, root ? b.send32 : nullptr, count, ncclFloat32, 0, c->comm, c->gstream);
  return e;
}

// Step 3, on the gather stream: rank 0 assembles the n frames (frames 0..n-2
// into its ring, frame n-1 into its image); another rank copies its last shard
// into its image, so the context reads as after n rm_dispatch calls.
int batch_finish(rm_ctx* c, int n) {
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  rm_ctx::BatchSlot& b = c->bslot[c->bnext];
  const size_t px = (size_t)c->rows * (size_t)c->cfg.width;
  if ((rc = phase(c, 2, c->gstream)) != RM_OK) return rc;
  if (comm_root(c)) {
    const int W = c->cfg.width, H = c->cfg.height, rb = c->cfg.row_block, rb0 = row_block0(c);
    const size_t stride = (size_t)n * (size_t)c->rows;  // rows between two ranks' blocks
    for (int k = 0; k < n; ++k) {
      if (b.send8) {
        void* dst = k < n - 1 ? (void*)c->ring8[k] : (void*)image_rgba8(c);
        const hipError_t e = rm::launch_unshard(b.send8 + (size_t)k * px * bpp8(c), dst, W, H, rb, rb0, c->cranks,
                                                c->rows, c->gstream, stride, c->rgb3);
        if (e != hipSuccess) return hip_fail(c, e, "unshard launch (batch)");
      }
      if (b.send32) {
        void* dst = k < n - 1 ? (void*)c->ring32[k] : (void*)c->d_frame32;
        const hipError_t e = rm::launch_unshard(b.send32 + (size_t)k * px * 4, dst, W * 4, H, rb, rb0,
                                                c->cranks, c->rows, c->gstream, stride);
        if (e != hipSuccess) return hip_fail(c, e, "unshard launch (batch, RGBA32F)");
      }
    }
  } else {
    if (b.send8 && render_dst(c))
      RM_HIP(c, hipMemcpyAsync(render_dst(c), b.send8 + (size_t)(n - 1) * px * bpp8(c), px * bpp8(c),
                               hipMemcpyDeviceToDevice, c->gstream));
    if (b.send32 && render_dst32(c))
      RM_HIP(c, hipMemcpyAsync(render_dst32(c), b.send32 + (size_t)(n - 1) * px * 4, px * 16,
                               hipMemcpyDeviceToDevice, c->gstream));
  }
  if ((rc = phase(c, 3, c->gstream)) != RM_OK) return rc;
  RM_HIP(c, hipEventRecord(b.freed, c->gstream));
  b.pending = true;
  RM_HIP(c, hipEventRecord(c->gdone, c->gstream));
  c->gdone_pending = true;
  if (c->timing) {
    c->ph_recorded = true;
    c->ph_comm = true;
  }
  c->blast = c->bnext;
  c->bnext ^= 1;
  c->batch_n = n;
  c->comm_warm = true;
  c->dispatched = true;
  return RM_OK;
}

}  // namespace

// One rank's batch (rm_comm_init), or a multi-GPU context's (every device
// renders, one group gathers, device 0 assembles).
int rm::comm_batch(rm_ctx* c, const rm_uniforms* u, int n) {
  if (c->comm_failed) return comm_dead(c);
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, err);
  const std::vector<rm_ctx*> ms = comm_members(c);
  int rc = RM_OK;
  for (rm_ctx* m : ms)
    if ((rc = batch_render(m, u, n)) != RM_OK) {
      if (m == c) return rc;
      // a member's communicator failed (its bounded slot wait): the frame's whole
      // group is aborted, as for any other member failure
      return rc == RM_ERR_COMM ? comm_abort(c, m->err) : fail(c, rc, m->err);
    }
  ncclResult_t e = r->GroupStart();
  if (e != ncclSuccess) return comm_abort(c, std::string("ncclGroupStart: ") + r->GetErrorString(e));
  for (rm_ctx* m : ms) {
    e = batch_gather(m, r, n);
    if (e != ncclSuccess && e != ncclInProgress) break;
  }
  const ncclResult_t eg = r->GroupEnd();
  if (e == ncclSuccess || e == ncclInProgress) e = eg;
  if ((rc = comm_enqueued(c, r, e, "ncclGather (batch)")) != RM_OK) return rc;
  for (rm_ctx* m : ms)
    if ((rc = batch_finish(m, n)) != RM_OK) return m == c ? rc : fail(c, rc, m->err);
  c->batch_n = n;
  c->dispatched = true;
  return RM_OK;
}

namespace {
//  Every rank of a communicator must cut the frame the same way, or
// the gather's counts differ (a stall until the deadline) or k_unshard puts rows
// in the wrong places: the ranks exchange (width, height, row_block, rank 0's
// rows per round, outputs, shard format) with one ncclAllGather on the new
// communicator, and a rank that sees a difference aborts it (every rank sees the
// same table, so every rank fails the same way) with RM_ERR_INVALID.
int comm_check_layout(rm_ctx* c, const rm::Rccl* r) {
  constexpr int K = 6;
  const int32_t mine[K] = {c->cfg.width, c->cfg.height, c->cfg.row_block, row_block0(c), c->cfg.outputs,
                           c->rgb3 ? RM_SHARD_RGB8 : RM_SHARD_RGBA8};
  int32_t* d = nullptr;
  RM_HIP(c, hipMalloc(&d, sizeof(mine) * (size_t)c->cranks));
  std::vector<int32_t> all((size_t)K * c->cranks, 0);
  hipError_t he = hipMemcpyAsync(d + (size_t)K * c->crank, mine, sizeof mine, hipMemcpyHostToDevice, c->stream);
  ncclResult_t e = ncclSuccess;
  if (he == hipSuccess) e = r->AllGather(d + (size_t)K * c->crank, d, K, ncclInt32, c->comm, c->stream);
  int rc = he != hipSuccess ? hip_fail(c, he, "hipMemcpyAsync (layout)")
                            : comm_enqueued(c, r, e, "ncclAllGather (rm_comm_init layout check)");
  if (rc == RM_OK) rc = comm_wait(c);  // bounded: a rank that dies here is RM_ERR_COMM
  if (rc == RM_OK && (he = hipMemcpy(all.data(), d, all.size() * sizeof(int32_t), hipMemcpyDeviceToHost)) != hipSuccess)
    rc = hip_fail(c, he, "hipMemcpy (layout)");
  (void)hipFree(d);
  if (rc != RM_OK) return rc;
  static const char* names[K] = {"width", "height", "row_block", "rank0_rows", "outputs", "shard_format"};
  for (int q = 0; q < c->cranks; ++q)
    for (int k = 0; k < K; ++k)
      if (all[(size_t)K * q + k] != all[k]) {
        const std::string why = std::string("rm_comm_init: ranks 0 and ") + std::to_string(q) + " disagree on " +
                                names[k] + " (" + std::to_string(all[k]) + " vs " +
                                std::to_string(all[(size_t)K * q + k]) + "): every rank must shard the frame alike";
        (void)comm_abort(c, why);
        return fail(c, RM_ERR_INVALID, why);
      }
  return RM_OK;
}
}  // namespace

extern "C" {

// ---- one rank per process -------------------------------------------------------------
int rm_comm_unique_id(void* id, size_t size) {
  if (!id || size < sizeof(ncclUniqueId)) return fail(nullptr, RM_ERR_INVALID, "rm_comm_unique_id: buffer < 128 bytes");
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(nullptr, RM_ERR_HIP, "rm_comm_unique_id: " + err);
  ncclUniqueId u;
  const ncclResult_t e = r->GetUniqueId(&u);
  if (e != ncclSuccess) return fail(nullptr, RM_ERR_HIP, std::string("ncclGetUniqueId: ") + r->GetErrorString(e));
  std::memcpy(id, &u, sizeof u);
  return RM_OK;
}

int rm_comm_init(rm_ctx* c, const void* id, int32_t nranks, int32_t rank) {
  if (!c || !id) return RM_ERR_INVALID;
  if (!c->subs.empty()) return fail(c, RM_ERR_STATE, "a multi-GPU context has its own communicator");
  if (c->comm) return fail(c, RM_ERR_STATE, "the context already has a communicator");
  if (has_gbuf(c)) return fail(c, RM_ERR_STATE, "rm_comm_init: not available on a G-buffer context (RM_OUT_GBUFFER)");
  // an aborted context can only be destroyed (rm_api.h); a second init would
  // re-attach without freeing its gather buffers
  if (c->comm_failed) return comm_dead(c);
  if (nranks < 1 || rank < 0 || rank >= nranks)
    return fail(c, RM_ERR_INVALID, "rm_comm_init: rank must be in 0..nranks-1");
  const int ns = c->cfg.nshards > 1 ? c->cfg.nshards : 1;
  if (ns != nranks || c->cfg.shard != rank)
    return fail(c, RM_ERR_INVALID, "rm_comm_init: the context must render shard `rank` of `nranks` "
                                   "(rm_config.shard / nshards)");
  if (check_comm_config(c->cfg, "rm_comm_init") != RM_OK) return fail(c, RM_ERR_INVALID, rm_last_error(nullptr));
  int rc = set_device(c);
  if (rc != RM_OK) return rc;
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, "rm_comm_init: " + err);
  ncclUniqueId u;
  std::memcpy(&u, id, sizeof u);
  ncclComm_t comm = nullptr;
  // non-blocking init, polled against the deadline: a rank that never joins is
  // RM_ERR_COMM after comm_timeout_ms, not a host thread blocked forever
  ncclConfig_t nb = rm::nonblocking_config();
  ncclResult_t e = r->CommInitRankConfig(&comm, nranks, u, rank, &nb);
  if ((e == ncclSuccess || e == ncclInProgress) && comm) e = rm::wait_ready(r, &comm, 1, c->comm_timeout_ms);
  if (e != ncclSuccess) {
    if (comm) (void)r->CommAbort(comm);
    if (e == ncclInProgress)
      return fail(c, RM_ERR_COMM, "rm_comm_init: the communicator was not ready within " +
                                      std::to_string(c->comm_timeout_ms) +
                                      " ms (rm_comm_set_timeout): a rank never joined");
    return nccl_fail(c, r, e, "ncclCommInitRankConfig");
  }
  RM_HIP(c, hipStreamSynchronize(c->stream));  // frames already queued keep their buffers
  if ((rc = comm_attach(c, comm, rank, nranks, true, false)) != RM_OK) {
    (void)r->CommAbort(comm);  // this rank leaves: its peers see the abort
    c->comm = nullptr;
    return rc;
  }
  return comm_check_layout(c, r);
}

int rm_comm_set_timeout(rm_ctx* c, int32_t timeout_ms) {
  if (!c) return RM_ERR_INVALID;
  if (timeout_ms < 0) return fail(c, RM_ERR_INVALID, "rm_comm_set_timeout: timeout_ms must be >= 0");
  c->comm_timeout_ms = timeout_ms;
  for (rm_ctx* s : c->subs) s->comm_timeout_ms = timeout_ms;
  return RM_OK;
}

int rm_comm_check(rm_ctx* c) {
  if (!c) return RM_ERR_INVALID;
  if (c->comm_failed) return comm_dead(c);
  if (!has_comm(c)) return RM_OK;
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, err);
  for (rm_ctx* m : comm_members(c)) {
    ncclResult_t st = ncclSuccess;
    const ncclResult_t e = r->CommGetAsyncError(m->comm, &st);
    if (e != ncclSuccess || (st != ncclSuccess && st != ncclInProgress))
      return comm_abort(c, std::string("RCCL asynchronous error on device ") + std::to_string(m->device) + ": " +
                               r->GetErrorString(e != ncclSuccess ? e : st));
  }
  return RM_OK;
}

int rm_comm_info(const rm_ctx* c, int32_t* rank, int32_t* nranks, int32_t* ngpus) {
  if (!c) return RM_ERR_INVALID;
  if (rank) *rank = c->crank;
  if (nranks) *nranks = c->subs.empty() ? c->cranks : (int32_t)c->subs.size();
  if (ngpus) *ngpus = c->subs.empty() ? 1 : (int32_t)c->subs.size();
  return RM_OK;
}

int rm_comm_rccl_info(rm_ctx* c, int32_t* count, int32_t* user_rank, int32_t* hip_device, int32_t* version) {
  if (!c) return RM_ERR_INVALID;
  if (count) *count = 0;
  if (user_rank) *user_rank = -1;
  if (hip_device) *hip_device = -1;
  if (version) *version = 0;
  if (c->comm_failed) return comm_dead(c);
  if (!has_comm(c)) return RM_OK;
  std::string err;
  const rm::Rccl* r = rm::rccl(&err);
  if (!r) return fail(c, RM_ERR_COMM, err);
  int v = 0;
  if (version && r->GetVersion(&v) == ncclSuccess) *version = v;
  // every member communicator as RCCL formed it: a multi-GPU context's device i
  // must be user rank i of ngpus, a rank's communicator rank crank of cranks
  const std::vector<rm_ctx*> ms = comm_members(c);
  for (size_t i = 0; i < ms.size(); ++i) {
    int n = 0, ur = -1, dev = -1;
    ncclResult_t e = r->CommCount(ms[i]->comm, &n);
    if (e == ncclSuccess) e = r->CommUserRank(ms[i]->comm, &ur);
    if (e == ncclSuccess) e = r->CommCuDevice(ms[i]->comm, &dev);
    if (e != ncclSuccess) return nccl_fail(c, r, e, "ncclCommCount / ncclCommUserRank / ncclCommCuDevice");
    const int want_n = c->subs.empty() ? c->cranks : (int)ms.size();
    const int want_r = c->subs.empty() ? c->crank : (int)i;
    if (n != want_n || ur != want_r || dev != ms[i]->device)
      return fail(c, RM_ERR_COMM, "RCCL reports rank " + std::to_string(ur) + " of " + std::to_string(n) +
                                      " on device " + std::to_string(dev) + " for a member set up as rank " +
                                      std::to_string(want_r) + " of " + std::to_string(want_n) + " on device " +
                                      std::to_string(ms[i]->device));
    if (i == 0) {
      if (count) *count = n;
      if (user_rank) *user_rank = ur;
      if (hip_device) *hip_device = dev;
    }
  }
  return RM_OK;
}

}  // extern "C"
