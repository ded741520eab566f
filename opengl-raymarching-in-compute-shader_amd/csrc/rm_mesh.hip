// rm_mesh.hip — SDF mesh extraction: a surface-nets mesh of a distance volume
// (rm_sdf_mesh / rm_sdf_mesh_device, include/rm_api.h).
//
// A translation unit of its own: every existing object is what it was without
// it.  The kernels are scene independent: the volume is written by the existing
// grid kernels (k_sdf_grid / k_table_sdf_grid), the attributes by the existing
// point kernels, both launched by the host around these:
//   k_mesh_classify  one lane per grid point, a wave-task 64 consecutive points of
//                    one x-row (rm_mesh_args.hpp), four tasks per wave and round, their
//                    loads issued together: the inside bits of the cell's 8
//                    corners, the cell's active flag and the flags of the up to 3
//                    quads the point's edges own; per wave five ballots (active, x,
//                    y, z edges, point inside) and two byte counts;
//   k_mesh_scan      exclusive scans of the two counts within chunks of 16,384
//                    wave-tasks, one workgroup per chunk, and the chunks' sums;
//   k_mesh_scan_chunks  the exclusive scan of those sums, and the totals (the
//                    mesh's counts): one workgroup;
//   k_mesh_vertices  the active cells' crossings again, the mean stored at the
//                    wave's offset + the lane's rank in the active mask (v_mbcnt);
//                    a launched wave visits those of 16 wave-tasks that hold a vertex;
//   k_mesh_quads     the owner points' quads from the ballots alone (no volume
//                    read); a neighbour cell's vertex index is its wave's offset +
//                    the popcount of its wave's mask below its lane;
//   k_mesh_attr_copy the device call's attribute records, from the context's
//                    staging copy, below the device-side count.
// No atomics: every output index follows from the grid order.  The vertex rule is
// written as single IEEE operations in the contract's order (no contraction:
// Makefile), so tests/sdf_mesh_model.py restates it bit for bit.
#include <hip/hip_runtime.h>

#include "rm_mesh_args.hpp"
#include "rm_scene.hpp"  // lane_rank

namespace rmd {

// Grid coordinate idx of one axis, as rm_sdf.hpp sdf_grid_coord: one IEEE
// multiply, then one IEEE add.
__device__ __forceinline__ float mesh_coord(float origin, float step, int idx) {
  const float m = (float)idx * step;
  return origin + m;
}

// Wave b's row and point: false for a lane past the row's end.
__device__ __forceinline__ bool mesh_point(const MeshArgs& M, uint32_t b, uint32_t& row, int& ix, int& iy, int& iz) {
  row = b / M.bpr;
  const uint32_t xb = b - row * M.bpr;
  iz = (int)(row / (uint32_t)M.ny);
  iy = (int)(row - (uint32_t)iz * (uint32_t)M.ny);
  ix = (int)(xb * 64u + (threadIdx.x & 63u));
  return ix < M.nx;
}

// The cell's 8 corner distances, corner c = dx + 2 dy + 4 dz; a corner outside the
// grid (in / hx / hy / hz false) reads as +0: outside.  Every load is made, at an
// address clamped into the grid (mesh_load), and its value dropped by a select
// afterwards (mesh_mask): no branch stands between the loads, so all of them, and
// those of the next wave-task, are in flight together.
struct MeshCorners {
  float d[8];
};
__device__ __forceinline__ MeshCorners mesh_load(const MeshArgs& M, uint32_t row, int ix, bool in, bool hx, bool hy,
                                                 bool hz) {
  const size_t nx = (size_t)M.nx, last = nx - 1;
  const size_t x0 = in ? (size_t)ix : last, x1 = hx ? (size_t)ix + 1 : last;
  const size_t r0 = (size_t)row * nx;  // row nx + x < 2^31
  const size_t r1 = hy ? r0 + nx : r0, r2 = hz ? r0 + nx * (size_t)M.ny : r0, r3 = hy ? r2 + nx : r2;
  const float v0 = M.vol[r0 + x0], v1 = M.vol[r0 + x1], v2 = M.vol[r1 + x0], v3 = M.vol[r1 + x1];
  const float v4 = M.vol[r2 + x0], v5 = M.vol[r2 + x1], v6 = M.vol[r3 + x0], v7 = M.vol[r3 + x1];
  return MeshCorners{{v0, v1, v2, v3, v4, v5, v6, v7}};
}
__device__ __forceinline__ MeshCorners mesh_mask(const MeshCorners& v, bool in, bool hx, bool hy, bool hz) {
  MeshCorners c;
  c.d[0] = in ? v.d[0] : 0.0f;
  c.d[1] = hx ? v.d[1] : 0.0f;
  c.d[2] = in && hy ? v.d[2] : 0.0f;
  c.d[3] = hx && hy ? v.d[3] : 0.0f;
  c.d[4] = in && hz ? v.d[4] : 0.0f;
  c.d[5] = hx && hz ? v.d[5] : 0.0f;
  c.d[6] = in && hy && hz ? v.d[6] : 0.0f;
  c.d[7] = hx && hy && hz ? v.d[7] : 0.0f;
  return c;
}

// A wave takes kMeshClassify consecutive wave-tasks a round and loads the corners
// of all of them before it looks at any: the kernel waits for memory, and a wave
// with one task's 8 loads in flight lives as long as one with 32.
constexpr uint32_t kMeshClassify = 4;

__global__ __launch_bounds__(64) void k_mesh_classify(MeshArgs M) {
  const uint32_t ngroups = (M.nw + kMeshClassify - 1u) / kMeshClassify;
  for (uint32_t g = blockIdx.x; g < ngroups; g += gridDim.x) {
    MeshCorners raw[kMeshClassify];
    int ix[kMeshClassify], iy[kMeshClassify], iz[kMeshClassify];
#pragma unroll
    for (uint32_t k = 0; k < kMeshClassify; ++k) {
      // (a task past the last loads the last one's corners, and drops them below)
      const uint32_t b = g * kMeshClassify + k, bb = b < M.nw ? b : M.nw - 1u;
      uint32_t row;
      const bool in = mesh_point(M, bb, row, ix[k], iy[k], iz[k]);
      raw[k] = mesh_load(M, row, ix[k], in, ix[k] + 1 < M.nx, iy[k] + 1 < M.ny, iz[k] + 1 < M.nz);
    }
#pragma unroll
    for (uint32_t k = 0; k < kMeshClassify; ++k) {
      const uint32_t b = g * kMeshClassify + k;
      if (b < M.nw) {
        const int x = ix[k], y = iy[k], z = iz[k];
        const bool in = x < M.nx, hx = x + 1 < M.nx, hy = y + 1 < M.ny, hz = z + 1 < M.nz;
        const MeshCorners ck = mesh_mask(raw[k], in, hx, hy, hz);
        int n = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) n += ck.d[j] < 0.0f ? 1 : 0;
        const bool active = hx && hy && hz && n > 0 && n < 8;
        // the point's own edges: they exist, their ends differ, and they are interior
        const bool a_in = ck.d[0] < 0.0f;
        const bool mx = x >= 1 && x + 2 <= M.nx, my = y >= 1 && y + 2 <= M.ny, mz = z >= 1 && z + 2 <= M.nz;
        const bool ex = hx && my && mz && a_in != (ck.d[1] < 0.0f);
        const bool ey = in && hy && mz && mx && a_in != (ck.d[2] < 0.0f);
        const bool ez = in && hz && mx && my && a_in != (ck.d[4] < 0.0f);
        const unsigned long long ba = __ballot(active), bx = __ballot(ex), by = __ballot(ey), bz = __ballot(ez),
                                 bi = __ballot(a_in);
        if ((threadIdx.x & 63u) == 0) {
          M.active[b] = ba;
          ulonglong2* e = reinterpret_cast<ulonglong2*>(M.edges + (size_t)b * 4);
          e[0] = make_ulonglong2(bx, by);
          e[1] = make_ulonglong2(bz, bi);
          M.vcnt[b] = (uint8_t)__popcll(ba);
          M.qcnt[b] = (uint8_t)(__popcll(bx) + __popcll(by) + __popcll(bz));
        }
      }
    }
  }
}

// One chunk's counts of a lane, 16 adjacent bytes as loaded; a count past the last
// wave is 0.  Returns their sum.
__device__ __forceinline__ uint32_t mesh_scan_unpack(uint4 v, size_t i0, uint32_t nw, uint32_t (&c)[kMeshScanPer]) {
  const uint32_t words[4] = {v.x, v.y, v.z, v.w};
  uint32_t sum = 0;
#pragma unroll
  for (int j = 0; j < kMeshScanPer; ++j) {
    c[j] = i0 + (size_t)j < (size_t)nw ? (words[j >> 2] >> (8 * (j & 3))) & 255u : 0u;
    sum += c[j];
  }
  return sum;
}

// Inclusive scan of v over the wave's lanes.
__device__ __forceinline__ uint32_t mesh_scan_wave(uint32_t v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// Exclusive scans of vcnt and qcnt within scan chunk blockIdx.x into voff / qoff,
// the chunk's sums into chunks[chunk][0 / 1]: one workgroup per chunk, both scans
// behind the same two barriers.  A chunk's sums fit a word (16,384 x 192 < 2^22).
__global__ __launch_bounds__(kMeshScanLanes) void k_mesh_scan(MeshArgs M) {
  constexpr int kWaves = kMeshScanLanes / 64;
  __shared__ uint32_t ws[2][kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const size_t i0 = (size_t)blockIdx.x * kMeshScanChunk + (size_t)t * kMeshScanPer;
  uint32_t cv[kMeshScanPer], cq[kMeshScanPer];
  const uint32_t vsum = mesh_scan_unpack(*reinterpret_cast<const uint4*>(M.vcnt + i0), i0, M.nw, cv);
  const uint32_t qsum = mesh_scan_unpack(*reinterpret_cast<const uint4*>(M.qcnt + i0), i0, M.nw, cq);
  const uint32_t vinc = mesh_scan_wave(vsum), qinc = mesh_scan_wave(qsum);
  if (lane == 63) {
    ws[0][w] = vinc;
    ws[1][w] = qinc;
  }
  __syncthreads();
  uint32_t vrun = vinc - vsum, qrun = qinc - qsum, vall = 0, qall = 0;
#pragma unroll
  for (int k = 0; k < kWaves; ++k) {
    const uint32_t sv = ws[0][k], sq = ws[1][k];
    vrun += k < w ? sv : 0u;
    qrun += k < w ? sq : 0u;
    vall += sv;
    qall += sq;
  }
  uint32_t vo[kMeshScanPer], qo[kMeshScanPer];
#pragma unroll
  for (int j = 0; j < kMeshScanPer; ++j) {
    vo[j] = vrun;
    qo[j] = qrun;
    vrun += cv[j];
    qrun += cq[j];
  }
  uint4* vd = reinterpret_cast<uint4*>(M.voff + i0);
  uint4* qd = reinterpret_cast<uint4*>(M.qoff + i0);
#pragma unroll
  for (int j = 0; j < kMeshScanPer / 4; ++j) {
    vd[j] = make_uint4(vo[4 * j], vo[4 * j + 1], vo[4 * j + 2], vo[4 * j + 3]);
    qd[j] = make_uint4(qo[4 * j], qo[4 * j + 1], qo[4 * j + 2], qo[4 * j + 3]);
  }
  if (t == 0) *reinterpret_cast<ulonglong2*>(M.chunks + (size_t)blockIdx.x * 2) = make_ulonglong2(vall, qall);
}

// Inclusive scan of v over the wave's lanes, 64-bit.
__device__ __forceinline__ unsigned long long mesh_scan_wave64(unsigned long long v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// The chunks' sums to their exclusive scans, in place, and the totals into
// counts[0] / counts[1]: one workgroup, 1024 chunks a round (a 256^3 grid has 16).
__global__ __launch_bounds__(kMeshScanLanes) void k_mesh_scan_chunks(MeshArgs M, uint32_t nchunks) {
  constexpr int kWaves = kMeshScanLanes / 64;
  __shared__ unsigned long long ws[2][kWaves];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  unsigned long long vbase = 0, qbase = 0;  // uniform
  for (uint32_t c0 = 0; c0 < nchunks; c0 += kMeshScanLanes) {
    const uint32_t ch = c0 + (uint32_t)t;
    ulonglong2 own = make_ulonglong2(0ull, 0ull);
    if (ch < nchunks) own = *reinterpret_cast<const ulonglong2*>(M.chunks + (size_t)ch * 2);
    const unsigned long long vinc = mesh_scan_wave64(own.x), qinc = mesh_scan_wave64(own.y);
    if (lane == 63) {
      ws[0][w] = vinc;
      ws[1][w] = qinc;
    }
    __syncthreads();
    unsigned long long vrun = vbase + (vinc - own.x), qrun = qbase + (qinc - own.y);
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
      const unsigned long long sv = ws[0][k], sq = ws[1][k];
      vrun += k < w ? sv : 0ull;
      qrun += k < w ? sq : 0ull;
      vbase += sv;
      qbase += sq;
    }
    __syncthreads();  // ws is rewritten next round
    if (ch < nchunks) *reinterpret_cast<ulonglong2*>(M.chunks + (size_t)ch * 2) = make_ulonglong2(vrun, qrun);
  }
  if (t == 0) {
    M.counts[0] = vbase;
    M.counts[1] = qbase;
  }
}

// One edge of the cell, from corner A (distance dA, coordinate cA on the edge's
// axis) to B: where its ends differ in "inside", the crossing joins the sums.
// pa / pu / pv: the sums' components on the edge's axis and on the two others.
__device__ __forceinline__ void mesh_edge(float dA, float dB, float cA, float cB, float cu, float cv, float& pa,
                                          float& pu, float& pv, int& n) {
  if ((dA < 0.0f) != (dB < 0.0f)) {
    const float t = dA / (dA - dB);
    const float w = cB - cA;
    const float m = t * w;
    pa = pa + (cA + m);
    pu = pu + cu;
    pv = pv + cv;
    n += 1;
  }
}

// Most waves of a grid hold no surface.  The two emitting kernels therefore do not
// give every wave-task a wave of its own: a wave looks at kMeshTasks consecutive
// tasks' counts, one per lane, and visits only those with work, in order.
constexpr uint32_t kMeshTasks = 16;

// The vertices of wave-task b: one lane per active cell.
__device__ __forceinline__ void mesh_task_vertices(const MeshArgs& M, uint32_t b) {
  const unsigned long long m = M.active[b];
  const long long v0 = (long long)(M.chunks[(size_t)(b >> kMeshScanShift) * 2] + M.voff[b]);
  if (v0 >= M.vcap) return;
  const long long v = v0 + (long long)lane_rank(m);
  if (!((m >> (threadIdx.x & 63u)) & 1ull) || v >= M.vcap) return;
  uint32_t row;
  int ix, iy, iz;
  (void)mesh_point(M, b, row, ix, iy, iz);
  const MeshCorners c = mesh_load(M, row, ix, true, true, true, true);  // an active cell: all 8 exist
  const float x0 = mesh_coord(M.origin[0], M.step[0], ix), x1 = mesh_coord(M.origin[0], M.step[0], ix + 1);
  const float y0 = mesh_coord(M.origin[1], M.step[1], iy), y1 = mesh_coord(M.origin[1], M.step[1], iy + 1);
  const float z0 = mesh_coord(M.origin[2], M.step[2], iz), z1 = mesh_coord(M.origin[2], M.step[2], iz + 1);
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  int n = 0;
  // axis x: u = y, v = z; starts (du, dv) = (0,0), (1,0), (0,1), (1,1)
  mesh_edge(c.d[0], c.d[1], x0, x1, y0, z0, ax, ay, az, n);
  mesh_edge(c.d[2], c.d[3], x0, x1, y1, z0, ax, ay, az, n);
  mesh_edge(c.d[4], c.d[5], x0, x1, y0, z1, ax, ay, az, n);
  mesh_edge(c.d[6], c.d[7], x0, x1, y1, z1, ax, ay, az, n);
  // axis y: u = z, v = x
  mesh_edge(c.d[0], c.d[2], y0, y1, z0, x0, ay, az, ax, n);
  mesh_edge(c.d[4], c.d[6], y0, y1, z1, x0, ay, az, ax, n);
  mesh_edge(c.d[1], c.d[3], y0, y1, z0, x1, ay, az, ax, n);
  mesh_edge(c.d[5], c.d[7], y0, y1, z1, x1, ay, az, ax, n);
  // axis z: u = x, v = y
  mesh_edge(c.d[0], c.d[4], z0, z1, x0, y0, az, ax, ay, n);
  mesh_edge(c.d[1], c.d[5], z0, z1, x1, y0, az, ax, ay, n);
  mesh_edge(c.d[2], c.d[6], z0, z1, x0, y1, az, ax, ay, n);
  mesh_edge(c.d[3], c.d[7], z0, z1, x1, y1, az, ax, ay, n);
  const float fn = (float)n;
  float* p = M.pos + (size_t)v * 3;
  p[0] = ax / fn;
  p[1] = ay / fn;
  p[2] = az / fn;
}

__global__ __launch_bounds__(64) void k_mesh_vertices(MeshArgs M) {
  const uint32_t lane = threadIdx.x & 63u, nblk = (M.nw + kMeshTasks - 1u) / kMeshTasks;
  for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint32_t mine = blk * kMeshTasks + lane;  // < 2^31 + 64
    unsigned long long todo = __ballot(lane < kMeshTasks && mine < M.nw && M.vcnt[mine] != 0);
    while (todo != 0ull) {
      mesh_task_vertices(M, blk * kMeshTasks + (uint32_t)__builtin_ctzll(todo));
      todo &= todo - 1ull;
    }
  }
}

// The vertex index of cell (ci, cj, ck): its wave's offset + the active lanes below its own.
__device__ __forceinline__ uint32_t mesh_vertex_of(const MeshArgs& M, int ci, int cj, int ck) {
  const uint32_t w = ((uint32_t)ck * (uint32_t)M.ny + (uint32_t)cj) * M.bpr + ((uint32_t)ci >> 6);
  const unsigned long long below = (1ull << ((uint32_t)ci & 63u)) - 1ull;
  return (uint32_t)M.chunks[(size_t)(w >> kMeshScanShift) * 2] + M.voff[w] + (uint32_t)__popcll(M.active[w] & below);
}

// Quad q of corners c0..c3 (counter-clockwise seen from +a when A is inside,
// else 0, 3, 2, 1): one 16-byte record, or under TRIANGLES 24 bytes at 24 q (8-byte
// aligned: an 8- and a 16-byte store, the 16-byte one on its boundary).
__device__ __forceinline__ void mesh_emit(const MeshArgs& M, unsigned long long q, bool a_in, uint32_t c0, uint32_t c1,
                                          uint32_t c2, uint32_t c3) {
  const uint32_t q1 = a_in ? c1 : c3, q3 = a_in ? c3 : c1;
  if (!M.triangles) {
    *reinterpret_cast<uint4*>(M.indices + q * 4ull) = make_uint4(c0, q1, c2, q3);
    return;
  }
  uint32_t* t = M.indices + q * 6ull;  // (q0, q1, q2), (q0, q2, q3)
  if (q & 1ull) {
    *reinterpret_cast<uint2*>(t) = make_uint2(c0, q1);
    *reinterpret_cast<uint4*>(t + 2) = make_uint4(c2, c0, c2, q3);
  } else {
    *reinterpret_cast<uint4*>(t) = make_uint4(c0, q1, c2, c0);
    *reinterpret_cast<uint2*>(t + 4) = make_uint2(c2, q3);
  }
}

// The quads of wave-task b: one lane per owner point.
__device__ __forceinline__ void mesh_task_quads(const MeshArgs& M, uint32_t b) {
  const unsigned long long q0 = M.chunks[(size_t)(b >> kMeshScanShift) * 2 + 1] + M.qoff[b];
  if (q0 >= (unsigned long long)M.qcap) return;
  const ulonglong2* e = reinterpret_cast<const ulonglong2*>(M.edges + (size_t)b * 4);
  const ulonglong2 e0 = e[0], e1 = e[1];
  const unsigned long long bx = e0.x, by = e0.y, bz = e1.x, bi = e1.y;
  const uint32_t lane = threadIdx.x & 63u;
  const bool ex = (bx >> lane) & 1ull, ey = (by >> lane) & 1ull, ez = (bz >> lane) & 1ull, a_in = (bi >> lane) & 1ull;
  if (!(ex || ey || ez)) return;
  // the quads of the lanes below come first, then the lane's own in axis order
  unsigned long long q = q0 + (unsigned long long)(lane_rank(bx) + lane_rank(by) + lane_rank(bz));
  uint32_t row;
  int i, j, k;
  (void)mesh_point(M, b, row, i, j, k);
  const unsigned long long cap = (unsigned long long)M.qcap;
  // the cell of the point itself is in all three rings
  const uint32_t own = mesh_vertex_of(M, i, j, k);
  if (ex) {  // u = y, v = z: cells (j-1, k-1), (j, k-1), (j, k), (j-1, k)
    if (q < cap)
      mesh_emit(M, q, a_in, mesh_vertex_of(M, i, j - 1, k - 1), mesh_vertex_of(M, i, j, k - 1), own,
                mesh_vertex_of(M, i, j - 1, k));
    q += 1;
  }
  if (ey) {  // u = z, v = x: cells (k-1, i-1), (k, i-1), (k, i), (k-1, i)
    if (q < cap)
      mesh_emit(M, q, a_in, mesh_vertex_of(M, i - 1, j, k - 1), mesh_vertex_of(M, i - 1, j, k), own,
                mesh_vertex_of(M, i, j, k - 1));
    q += 1;
  }
  if (ez) {  // u = x, v = y: cells (i-1, j-1), (i, j-1), (i, j), (i-1, j)
    if (q < cap)
      mesh_emit(M, q, a_in, mesh_vertex_of(M, i - 1, j - 1, k), mesh_vertex_of(M, i, j - 1, k), own,
                mesh_vertex_of(M, i - 1, j, k));
  }
}

__global__ __launch_bounds__(64) void k_mesh_quads(MeshArgs M) {
  const uint32_t lane = threadIdx.x & 63u, nblk = (M.nw + kMeshTasks - 1u) / kMeshTasks;
  for (uint32_t blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const uint32_t mine = blk * kMeshTasks + lane;
    unsigned long long todo = __ballot(lane < kMeshTasks && mine < M.nw && M.qcnt[mine] != 0);
    while (todo != 0ull) {
      mesh_task_quads(M, blk * kMeshTasks + (uint32_t)__builtin_ctzll(todo));
      todo &= todo - 1ull;
    }
  }
}

// The device call's attributes: records v < min(vertices, vcap) from the
// context's staging copy (the point kernel ran over the whole capacity, the host
// not knowing the count) to the caller's array; three 16-byte words per record.
__global__ __launch_bounds__(256) void k_mesh_attr_copy(const uint4* __restrict__ src, uint4* __restrict__ dst,
                                                        const unsigned long long* __restrict__ counts, long long vcap) {
  const unsigned long long nv = counts[0];
  const unsigned long long n = (nv < (unsigned long long)vcap ? nv : (unsigned long long)vcap) * 3ull;
  for (unsigned long long i = (unsigned long long)blockIdx.x * 256ull + threadIdx.x; i < n;
       i += (unsigned long long)gridDim.x * 256ull)
    dst[i] = src[i];
}

}  // namespace rmd

namespace rm {

namespace {
unsigned mesh_emit_blocks(const rmd::MeshArgs& M) {
  const uint32_t nblk = (M.nw + rmd::kMeshTasks - 1u) / rmd::kMeshTasks;
  return nblk < rmd::kMeshMaxWg ? nblk : rmd::kMeshMaxWg;
}
}  // namespace

// Every dim >= 2.  The ballots and counts of M.vol, then their scans and the
// mesh's counts.  The per-wave arrays hold whole scan chunks (rm_mesh_args.hpp).
hipError_t launch_mesh_count(const rmd::MeshArgs& M, hipStream_t s) {
  const uint32_t ngroups = (M.nw + rmd::kMeshClassify - 1u) / rmd::kMeshClassify;
  const uint32_t blocks = ngroups < rmd::kMeshMaxWg ? ngroups : rmd::kMeshMaxWg;
  hipLaunchKernelGGL(rmd::k_mesh_classify, dim3(blocks), dim3(64), 0, s, M);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return e;
  const uint32_t nchunks = (uint32_t)(((size_t)M.nw + rmd::kMeshScanChunk - 1) / rmd::kMeshScanChunk);
  hipLaunchKernelGGL(rmd::k_mesh_scan, dim3(nchunks), dim3(rmd::kMeshScanLanes), 0, s, M);
  if ((e = hipGetLastError()) != hipSuccess) return e;
  hipLaunchKernelGGL(rmd::k_mesh_scan_chunks, dim3(1), dim3(rmd::kMeshScanLanes), 0, s, M, nchunks);
  return hipGetLastError();
}

// The vertices below M.vcap and the quads below M.qcap, after launch_mesh_count.
hipError_t launch_mesh_emit(const rmd::MeshArgs& M, hipStream_t s) {
  if (M.vcap > 0) {
    hipLaunchKernelGGL(rmd::k_mesh_vertices, dim3(mesh_emit_blocks(M)), dim3(64), 0, s, M);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  if (M.qcap > 0) hipLaunchKernelGGL(rmd::k_mesh_quads, dim3(mesh_emit_blocks(M)), dim3(64), 0, s, M);
  return hipGetLastError();
}

// n >= 1 staged records at most: those below min(counts[0], vcap) to dst.
hipError_t launch_mesh_attr_copy(const void* src, void* dst, const void* counts, int64_t vcap, int64_t n,
                                 hipStream_t s) {
  const int64_t words = n * 3, want = (words + 255) / 256;
  const unsigned blocks = (unsigned)(want < 65536 ? want : 65536);
  hipLaunchKernelGGL(rmd::k_mesh_attr_copy, dim3(blocks), dim3(256), 0, s, static_cast<const uint4*>(src),
                     static_cast<uint4*>(dst), static_cast<const unsigned long long*>(counts), (long long)vcap);
  return hipGetLastError();
}

}  // namespace rm
