"""SDF mesh extraction against the volume it is made from (diagnostic, not product).

  python tools/probe_sdf_mesh.py [--rounds 15] [--n 256]

One MI355X, an n^3 grid (default 256^3 = 16.8 M points) spanning the scene's box
(-32, -7, -36) .. (22, 12, 16) at iTime = 1, the built-in scene and the default
table.  Kernel times by the context's own events (rm_enable_timing /
rm_kernel_time_ms; a mesh call is one bracketed sequence), the variants alternating
within every round after a warm-up; median [min, max]:

  (a) grid dist        rm_sdf_grid_device, dist only, on the same grid: the volume pass
                       alone, the floor the mesh cannot go below
  (b) mesh             rm_sdf_mesh_device without attributes, capacities = the counts
  (c) mesh + attr      rm_sdf_mesh_device with attributes and RM_MESH_NORMAL
  (d) copy             a device-to-device copy (torch, torch's events) moving the bytes
                       (b) has to read and write: the volume written and read once, the
                       per-wave arrays written and read once, the positions and indices
                       written (an ideal count from the sizes, not a counter)

Before timing, the probe checks the mesh of a 64^3 grid over the same box against
tests/sdf_mesh_model.py on the context's own rm_sdf_grid volume, bit for bit.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32 = np.float32
LO, HI = (-32.0, -7.0, -36.0), (22.0, 12.0, 16.0)
WAVE_BYTES = 32 + 8 + 4 + 4 + 1 + 1  # rm_mesh_args.hpp: the per-wave arrays


def fmt(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]"


def box_grid(n):
    origin = [float(F32(v)) for v in LO]
    step = [float(F32((h - l) / (n - 1))) for l, h in zip(LO, HI)]
    return origin, step, (n, n, n)


def probe_scene(rm, torch, name, scene, n, rounds, warmup):
    import sdf_mesh_model as MM
    dev = torch.device("cuda", torch.cuda.current_device())
    lib = rm.lib()
    r = rm.Renderer(64, 64)
    if scene is not None:
        r.set_scene(scene)
    u = rm.default_uniforms()
    u.iTime = 1.0
    r.set_uniforms(u)

    # the check: a 64^3 grid against the host-side model
    o64, s64, d64 = box_grid(64)
    pos, quads, attr = r.sdf_mesh(o64, s64, d64, normals=True)
    wpos, wquads = MM.mesh(r.sdf_grid(o64, s64, d64), o64, s64)
    ok = pos.tobytes() == wpos.tobytes() and quads.tobytes() == wquads.tobytes()
    ok &= attr.tobytes() == r.sdf(pos, rm.RM_SDF_NORMAL).tobytes()
    print(f"{name}: check  64^3 mesh ({len(pos)} vertices, {len(quads)} quads) == model, attr == rm_sdf_points: {ok}")
    if not ok:
        sys.exit("probe_sdf_mesh: the meshes differ")

    origin, step, dims = box_grid(n)
    N = n ** 3
    g = rm.rm_sdf_grid_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims))
    counts = torch.zeros(2, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    assert lib.rm_sdf_mesh_device(r.handle, C.byref(g), 0, None, None, 0, None, 0, counts.data_ptr()) == rm.RM_OK
    r.synchronize()
    nv, nq = counts.cpu().tolist()
    nw = (n + 63) // 64 * n * n
    print(f"{name}: {n}^3 = {N} points, {nw} waves, {nv} vertices, {nq} quads")
    dist = torch.empty(N, dtype=torch.float32, device=dev)
    tpos = torch.empty((max(nv, 1), 3), dtype=torch.float32, device=dev)
    tatt = torch.empty((max(nv, 1), 12), dtype=torch.float32, device=dev)
    tidx = torch.empty((max(nq, 1), 4), dtype=torch.int32, device=dev)

    def grid():
        assert lib.rm_sdf_grid_device(r.handle, C.byref(g), dist.data_ptr(), None) == rm.RM_OK

    def mesh(attrs):
        assert lib.rm_sdf_mesh_device(r.handle, C.byref(g), rm.RM_MESH_NORMAL if attrs else 0, tpos.data_ptr(),
                                      tatt.data_ptr() if attrs else None, nv, tidx.data_ptr(), nq,
                                      counts.data_ptr()) == rm.RM_OK

    r.enable_timing(True)
    r.kernel_time_ms(reset=True)

    def timed(fn):
        def run():
            fn()
            ms, launches = r.kernel_time_ms(reset=True)  # synchronises
            assert launches == 1, launches
            return ms
        return run

    moved = 2 * 4 * N + 2 * WAVE_BYTES * nw + 12 * nv + 16 * nq  # read + written by (b), ideal
    src = torch.zeros(moved // 8, dtype=torch.float32, device=dev)  # a copy reads and writes each byte
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy():
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    variants = {"(a) grid dist": timed(grid), "(b) mesh": timed(lambda: mesh(False)),
                "(c) mesh + attr NORMAL": timed(lambda: mesh(True)), "(d) copy": copy}
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # alternating: drift hits every variant alike
            res[k].append(fn())
    print(f"{'variant':<26} {'median [min, max] ms':<30} ({rounds} rounds, alternating)")
    for k, v in res.items():
        print(f"{k:<26} {fmt(v)}")
    med = {k: statistics.median(v) for k, v in res.items()}
    own = med["(b) mesh"] - med["(a) grid dist"]
    print(f"(d) moves {moved / 1e6:.1f} MB (read + write) at {moved / med['(d) copy'] / 1e9:.2f} TB/s")
    print(f"the mesher's own cost (b) - (a) = {own:.4f} ms = {own / med['(d) copy']:.2f} x (d); "
          f"(b) / (a) = {med['(b) mesh'] / med['(a) grid dist']:.3f}")
    print(f"the attributes (c) - (b) = {med['(c) mesh + attr NORMAL'] - med['(b) mesh']:.4f} ms for {nv} vertices\n")
    r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--n", type=int, default=256)
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_sdf_mesh: no GPU (nothing here is measured on a CPU)")
    probe_scene(rm, torch, "built-in scene", None, a.n, a.rounds, a.warmup)
    probe_scene(rm, torch, "default table", rm.default_scene(), a.n, a.rounds, a.warmup)


if __name__ == "__main__":
    main()
