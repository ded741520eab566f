// rm_mesh_args.hpp — the kernel arguments of SDF mesh extraction (rm_sdf_mesh,
// include/rm_api.h), shared by the kernels (rm_mesh.hip) and the
// host (rm_api_mesh.hip).
#pragma once

#include <cstddef>
#include <cstdint>

namespace rmd {

// k_mesh_scan takes the waves' counts in chunks of this many (1024 lanes x 16
// counts, one 16-byte load each), a workgroup per chunk; the per-wave arrays are
// allocated up to a whole number of chunks, and the scan reads a count past the
// last wave as 0.  A wave's offset is its chunk's (chunks, 64 bits) + its own
// within the chunk (voff / qoff, words).
constexpr int kMeshScanLanes = 1024, kMeshScanPer = 16, kMeshScanShift = 14;
constexpr size_t kMeshScanChunk = (size_t)kMeshScanLanes * kMeshScanPer;
static_assert(kMeshScanChunk == (size_t)1 << kMeshScanShift, "a wave's chunk is b >> kMeshScanShift");
// Workgroups of a mesh launch at most, as rm_sdf_args.hpp kSdfGridMaxWg.
constexpr uint32_t kMeshMaxWg = 1u << 24;

// The point grid drives the waves, as it drives k_sdf_grid's: wave b = row bpr +
// x-block, row = iz ny + iy, its lane l the point ix = 64 x-block + l.  A lane
// stands for its point (the quads of the three edges that start there) and for
// the cell whose low corner the point is (its vertex), where that cell exists.
// The nw = bpr ny nz waves (<= nx ny nz <= 2^31 - 1) are taken by the workgroups
// of a 1-D launch with a grid stride.
struct MeshArgs {
  float origin[3], step[3];
  int32_t nx, ny, nz;
  uint32_t bpr;  // x-blocks per row: ceil(nx / 64)
  uint32_t nw;   // bpr * ny * nz
  const float* vol;  // [nz][ny][nx]: rm_sdf_grid's distances
  // per wave, written by k_mesh_classify
  unsigned long long* active;  // [nw] the lanes whose cell is active
  unsigned long long* edges;   // [nw][4] the lanes whose x, y, z edge emits a quad; the lanes whose point is inside
  uint8_t* vcnt;               // [nw] popcount of active, 0..64
  uint8_t* qcnt;               // [nw] popcounts of the three edge masks, 0..192
  // per wave, written by k_mesh_scan: exclusive scans of vcnt / qcnt within the wave's chunk
  uint32_t* voff;              // [nw] below 2^20
  uint32_t* qoff;              // [nw] below 2^22
  // per chunk: the chunk's sums (k_mesh_scan), then their exclusive scans (k_mesh_scan_chunks):
  // vertices (below the cells: < 2^31), quads (below 3 points: past 32 bits)
  unsigned long long* chunks;  // [ceil(nw / kMeshScanChunk)][2]
  unsigned long long* counts;  // [2] rm_sdf_mesh_counts: vertices, quads
  // outputs, written below the capacities only
  float* pos;         // [vcap][3]
  uint32_t* indices;  // [qcap][4], or [qcap][6] with triangles set; 16-byte aligned
  long long vcap, qcap;
  uint32_t triangles;
};

}  // namespace rmd
