"""SDF field queries against the stores they make (diagnostic, not product).

  python tools/probe_sdf.py [--rounds 15] [--n 256]

One MI355X, an n^3 grid (default 256^3 = 16.8 M points) spanning the scene's box
(-32, -7, -36) .. (22, 12, 16), the built-in scene and the default table.  Kernel
times by the context's own events (rm_enable_timing / rm_kernel_time_ms), the
variants alternating within every round after a warm-up; median [min, max]:

  (a) points VALUE / NORMAL   rm_sdf_points_device over the grid's coordinates (12 B read,
                              48 B written per point)
  (b) grid x64 / x256v4       rm_sdf_grid_device, dist only and dist + ids, in both lane
                              mappings: 64 consecutive x per wave with 4-byte stores (taken
                              for outputs 4 bytes past a 16-byte boundary), and 4 x per lane,
                              256 per wave, with 16-byte stores (aligned outputs)
      x64 aligned, nx - 1     the 64-per-wave mapping on aligned outputs, taken by an odd nx
                              (n - 1 columns of the same grid; its time is scaled by
                              n / (n - 1)): the mapping apart from the 4-byte offset
  (c) copy4 / copy8 / copy48  a device-to-device copy of the same output bytes (torch,
                              torch's events): the stores' hardware bound

Before timing, the probe checks (b) == (a) bit for bit, in both mappings.
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))

F32 = np.float32
LO, HI = (-32.0, -7.0, -36.0), (22.0, 12.0, 16.0)


def fmt(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]"


def probe_scene(rm, torch, name, scene, n, rounds, warmup):
    dev = torch.device("cuda", torch.cuda.current_device())
    N = n ** 3
    origin = [F32(v) for v in LO]
    step = [F32((h - l) / (n - 1)) for l, h in zip(LO, HI)]
    g = rm.rm_sdf_grid_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(n, n, n))
    g_odd = rm.rm_sdf_grid_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(n - 1, n, n))
    ax = [origin[a] + np.arange(n, dtype=F32) * step[a] for a in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    pts = torch.from_numpy(np.stack([x.reshape(-1), y.reshape(-1), z.reshape(-1)], axis=1).astype(F32)).to(dev)
    rec = torch.empty((N, 12), dtype=torch.float32, device=dev)
    # outputs with room for the 4-byte offset; the aligned views start 16 bytes in
    dbuf = torch.empty(N + 8, dtype=torch.float32, device=dev)
    ibuf = torch.empty(N + 8, dtype=torch.int32, device=dev)
    assert dbuf.data_ptr() % 16 == 0 and ibuf.data_ptr() % 16 == 0
    lib = rm.lib()
    r = rm.Renderer(64, 64)
    if scene is not None:
        r.set_scene(scene)
    u = rm.default_uniforms()
    u.iTime = 1.0
    r.set_uniforms(u)

    def points(flags):
        assert lib.rm_sdf_points_device(r.handle, pts.data_ptr(), N, flags, rec.data_ptr()) == rm.RM_OK

    def grid(off, ids, desc=g):
        assert lib.rm_sdf_grid_device(r.handle, C.byref(desc), dbuf.data_ptr() + 4 * off,
                                      ibuf.data_ptr() + 4 * off if ids else None) == rm.RM_OK

    # (b) == (a), bit for bit, in both mappings
    torch.cuda.synchronize()
    points(0)
    r.synchronize()
    want = rec.view(torch.int32)
    ok = True
    for off in (4, 5):
        dbuf.zero_()
        ibuf.zero_()
        torch.cuda.synchronize()  # torch's stream is not the context's: clear before the kernel writes
        grid(off, True)
        r.synchronize()
        ok &= bool((dbuf[off:off + N].view(torch.int32) == want[:, 0]).all())
        ok &= bool((ibuf[off:off + N] == want[:, 1]).all())
    inside = int((rec[:, 0] < 0).sum())
    print(f"{name}: {n}^3 = {N} points, {inside} inside an object")
    print(f"check  grid (both mappings) == points, dist and ids bit for bit: {ok}")
    if not ok:
        sys.exit("probe_sdf: the values differ")

    r.enable_timing(True)
    r.kernel_time_ms(reset=True)

    def timed(fn):
        def run():
            fn()
            ms, launches = r.kernel_time_ms(reset=True)  # synchronises
            assert launches == 1, launches
            return ms
        return run

    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def copy(words):
        src = torch.zeros(N * words, dtype=torch.float32, device=dev)
        dst = torch.empty_like(src)

        def run():
            ev[0].record()
            dst.copy_(src)
            ev[1].record()
            ev[1].synchronize()
            return ev[0].elapsed_time(ev[1])
        return run

    variants = {
        "(a) points VALUE": timed(lambda: points(0)),
        "(a) points NORMAL": timed(lambda: points(2)),
        "(b) grid x64 dist": timed(lambda: grid(5, False)),
        "(b) grid x64 dist+ids": timed(lambda: grid(5, True)),
        "(b) grid x64 aligned dist+ids": (lambda f: lambda: f() * n / (n - 1))(timed(lambda: grid(4, True, g_odd))),
        "(b) grid x256v4 dist": timed(lambda: grid(4, False)),
        "(b) grid x256v4 dist+ids": timed(lambda: grid(4, True)),
        "(c) copy4": copy(1), "(c) copy8": copy(2), "(c) copy48": copy(12),
    }
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
    print(f"copy rates: copy4 {2 * N * 4 / med['(c) copy4'] / 1e9:.2f}, copy8 {2 * N * 8 / med['(c) copy8'] / 1e9:.2f}, "
          f"copy48 {2 * N * 48 / med['(c) copy48'] / 1e9:.2f} TB/s (read + write)")
    for k, c in (("(b) grid x64 dist", "(c) copy4"), ("(b) grid x256v4 dist", "(c) copy4"),
                 ("(b) grid x64 dist+ids", "(c) copy8"), ("(b) grid x256v4 dist+ids", "(c) copy8"),
                 ("(a) points VALUE", "(c) copy48"), ("(a) points NORMAL", "(c) copy48")):
        print(f"{k} / {c} = {med[k] / med[c]:.2f};  {N / med[k] / 1e6:.2f} G points/s")
    print(f"x64 aligned / x64 at +4 bytes (dist+ids) = "
          f"{med['(b) grid x64 aligned dist+ids'] / med['(b) grid x64 dist+ids']:.3f}; x256v4 / x64 aligned = "
          f"{med['(b) grid x256v4 dist+ids'] / med['(b) grid x64 aligned dist+ids']:.3f}")
    print(f"(b) x256v4 dist+ids / (a) VALUE = {med['(b) grid x256v4 dist+ids'] / med['(a) points VALUE']:.3f}; "
          f"(b) x64 dist+ids / (a) VALUE = {med['(b) grid x64 dist+ids'] / med['(a) points VALUE']:.3f}; "
          f"x256v4 / x64 (dist+ids) = {med['(b) grid x256v4 dist+ids'] / med['(b) grid x64 dist+ids']:.3f}\n")
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
        sys.exit("probe_sdf: no GPU (nothing here is measured on a CPU)")
    probe_scene(rm, torch, "built-in scene", None, a.n, a.rounds, a.warmup)
    probe_scene(rm, torch, "default table", rm.default_scene(), a.n, a.rounds, a.warmup)


if __name__ == "__main__":
    main()
