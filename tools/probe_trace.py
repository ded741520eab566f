"""Ray queries against the frame they could replace (diagnostic, not product).

  python tools/probe_trace.py [--rounds 15] [--width 1920 --height 1080]

One MI355X, the cfg 2 frame: 1080p, sweep frame 60, 1 bounce, no supersampling.
Kernel times by the context's own events (rm_enable_timing / rm_kernel_time_ms),
one launch per sample, the variants alternating within every round after a warm-up:

  k_pixel        the frame itself (rm_dispatch): the yardstick, unchanged by this work
  shade_pixel    RM_TRACE_SHADE of the frame's W x H primary rays from a device
                 buffer, in pixel order (row-major: a wave is 64 pixels of one row)
  shade_tile     the same rays in 8x8-tile order (a wave is k_pixel's 8x8 tile)
  shade_random   the same rays in a seeded random permutation
  hit_tile       RM_TRACE_HIT alone, tile order

For each: median / min / max kernel ms, rays per second and the memory a ray moves
(24 B read + 48 B written) as a rate and as a share of the 6.3 TB/s a copy kernel
reaches on this part (8 TB/s peak).  The rays are the oracle's castRay in numpy
float32 (the same IEEE operations), so the probe first checks that the SHADE trace
equals the frame's own RGBA32F image bit for bit at this size, in every order.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))

F32 = np.float32
HBM_COPY_TBS, HBM_PEAK_TBS = 6.3, 8.0
BYTES_PER_RAY = 24 + 48


def primary_rays(u, W, H):
    """castRay (glsl:68-74) for every pixel without supersampling, uv as glsl:301-305."""
    cam = u.camera
    x, y, dr = (np.array(list(v), F32) for v in (cam.xAxis, cam.yAxis, cam.dir))
    P = F32(45.0) * F32(0.01745329251994329576923690768489)
    uvx = ((np.arange(W, dtype=np.int32) * 2 - W).astype(F32) / F32(W))[None, :]
    uvy = ((np.arange(H, dtype=np.int32) * 2 - H).astype(F32) / F32(H))[:, None]
    v = [(uvx * x[k] + uvy * y[k]) + dr[k] * P for k in range(4)]
    dd = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])
    inv = F32(1.0) / np.sqrt(dd)
    d = np.stack([v[0] * inv, v[1] * inv, v[2] * inv], axis=-1).astype(F32)
    o = np.broadcast_to(np.array(list(cam.pos)[:3], F32), d.shape).copy()
    return o.reshape(-1, 3), d.reshape(-1, 3)


def orders(W, H, seed=1):
    idx = np.arange(W * H, dtype=np.int64).reshape(H, W)
    th, tw = H // 8, W // 8
    assert th * 8 == H and tw * 8 == W, "the tile order wants multiples of 8"
    tile = idx.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(-1)
    return {"pixel": idx.reshape(-1), "tile": tile,
            "random": np.random.default_rng(seed).permutation(W * H)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_trace: no GPU (nothing here is measured on a CPU)")
    W, H = a.width, a.height
    n = W * H
    u = rm.sweep_uniforms(60, 120, 1, False, rm.RM_SHADOW_SOFT)
    o, d = primary_rays(u, W, H)
    perm = orders(W, H)
    dev = torch.device("cuda", torch.cuda.current_device())
    rays = {k: (torch.from_numpy(o[p]).to(dev), torch.from_numpy(d[p]).to(dev)) for k, p in perm.items()}

    # the same values first: SHADE in every order against the frame's own RGBA32F image
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA32F) as c:
        c.dispatch(u)
        img = c.read_rgba32f().reshape(-1, 4)[:, :3].view(np.uint32)
        for k, p in perm.items():
            got = c.trace(*rays[k], rm.RM_TRACE_SHADE)
            c.synchronize()
            col = got.cpu().numpy()[:, 9:12].view(np.uint32)
            same = bool((col == img[p]).all())
            print(f"check  shade_{k:<7} == the frame's RGBA32F image, bit for bit: {same}")
            if not same:
                sys.exit("probe_trace: the trace and the frame differ")
        hit = c.trace(*rays["tile"], rm.RM_TRACE_HIT).cpu().numpy()[:, 0]
        print(f"frame  {W}x{H}, {n} primary rays, {int((hit != -1.0).sum())} hit "
              f"({100.0 * (hit != -1.0).mean():.1f} %)")

    r = rm.Renderer(W, H)  # RGBA8, as bench.py renders cfg 2
    r.set_uniforms(u)
    r.enable_timing(True)
    variants = {
        "k_pixel": lambda: r.dispatch(),
        "shade_pixel": lambda: r.trace(*rays["pixel"], rm.RM_TRACE_SHADE),
        "shade_tile": lambda: r.trace(*rays["tile"], rm.RM_TRACE_SHADE),
        "shade_random": lambda: r.trace(*rays["random"], rm.RM_TRACE_SHADE),
        "hit_tile": lambda: r.trace(*rays["tile"], rm.RM_TRACE_HIT),
    }

    def one(fn):
        keep = fn()  # (a trace's result tensor lives until its kernel has run)
        ms, launches = r.kernel_time_ms(reset=True)  # synchronises
        assert launches == 1, launches
        del keep
        return ms

    for _ in range(a.warmup):
        for fn in variants.values():
            one(fn)
    res = {k: [] for k in variants}
    for _ in range(a.rounds):
        for k, fn in variants.items():  # alternating: drift hits every variant alike
            res[k].append(one(fn))
    base = statistics.median(res["k_pixel"])
    print(f"\n{'variant':<13} {'median ms':>10} {'min':>8} {'max':>8} {'vs k_pixel':>11} {'Mrays/s':>9} "
          f"{'B/ray':>6} {'GB/s':>8} {'of copy peak':>13}   ({a.rounds} rounds, alternating)")
    for k, v in res.items():
        m = statistics.median(v)
        b = 4 if k == "k_pixel" else BYTES_PER_RAY  # the frame writes one RGBA8 pixel per ray
        gbs = n * b / (m * 1e-3) / 1e9
        print(f"{k:<13} {m:>10.4f} {min(v):>8.4f} {max(v):>8.4f} {m / base:>10.2f}x {n / (m * 1e-3) / 1e6:>9.1f} "
              f"{b:>6d} {gbs:>8.1f} {100.0 * gbs / (HBM_COPY_TBS * 1e3):>12.2f}%")
    t_mem = n * BYTES_PER_RAY / (HBM_COPY_TBS * 1e12) * 1e3
    print(f"\nmemory bound of a trace of {n} rays: {n * BYTES_PER_RAY / 1e6:.1f} MB / {HBM_COPY_TBS} TB/s "
          f"(copy kernel; peak {HBM_PEAK_TBS}) = {t_mem:.4f} ms")
    for k in ("shade_tile", "hit_tile"):
        m = statistics.median(res[k])
        print(f"  {k}: {m:.4f} ms = {m / t_mem:.1f} x that bound -> "
              f"{'memory' if m < 1.5 * t_mem else 'compute / latency'} bound")
    r.close()


if __name__ == "__main__":
    main()
