"""The fused G-buffer against what a caller had to do without it (diagnostic, not product;
DESIGN §4.10).

  python tools/probe_gbuffer.py [--rounds 15] [--cfg 2 3]
  python tools/probe_gbuffer.py --waves-ab tools/variants/librm_gbuf_w7.so [--rounds 9]

One MI355X, two frames: cfg 2 (1080p, sweep frame 60, 1 bounce, no supersampling) and
cfg 3 (4K, sweep frame 60, 3 bounces, AA).  Kernel times by the context's own events
(rm_enable_timing / rm_kernel_time_ms), the variants alternating within every round
after a warm-up; median [min, max] over the rounds:

  (a) plain        rm_dispatch of an RGBA8 context (as bench.py renders the frame)
  (b) gbuffer      rm_dispatch of an RGBA8 | G-buffer context: the fused kernel
  (c) plain+trace  (a) plus rm_trace_rays_device(HIT | NORMAL) of the frame's primary
                   rays from a device buffer in 8x8-tile order: the two kernels' times
                   added, what the same records cost without the fused output
  copy32           a device-to-device copy of 32 B per pixel (torch, torch's events):
                   the yardstick for (b) - (a), the price of the G-buffer's stores

The rays are castRay in numpy float32 (with AA on: the first sample's, uv + 0.25 / dims),
so the probe first checks that the G-buffer equals the trace of those rays bit for bit.

--waves-ab LIB: the launch bound of k_gbuf_pixel / k_gbuf_sample.  LIB is a librm built
with another RM_GBUF_WAVES (tools/build_variant.sh gbuf_w7 -DRM_GBUF_WAVES=7); each
(round, library) is a process of its own (RM_LIBRM), the two alternating, each timing
variant (b) alone.
"""
import argparse
import json
import os
import statistics
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))

F32 = np.float32
CFGS = {2: (1920, 1080, 1, False), 3: (3840, 2160, 3, True)}
HITN = 2  # RM_TRACE_HIT | RM_TRACE_NORMAL


def primary_rays(u, W, H, aa):
    """castRay (glsl:68-74) of every pixel's G-buffer ray: uv as glsl:301-305, with AA on
    the first sample's offset pair added (glsl:311-313)."""
    cam = u.camera
    x, y, dr = (np.array(list(v), F32) for v in (cam.xAxis, cam.yAxis, cam.dir))
    P = F32(45.0) * F32(0.01745329251994329576923690768489)
    uvx = ((np.arange(W, dtype=np.int32) * 2 - W).astype(F32) / F32(W))[None, :]
    uvy = ((np.arange(H, dtype=np.int32) * 2 - H).astype(F32) / F32(H))[:, None]
    if aa:
        uvx = uvx + F32(0.25) / F32(W)
        uvy = uvy + F32(0.25) / F32(H)
    v = [(uvx * x[k] + uvy * y[k]) + dr[k] * P for k in range(4)]
    dd = (v[0] * v[0] + v[1] * v[1]) + (v[2] * v[2] + v[3] * v[3])
    inv = F32(1.0) / np.sqrt(dd)
    d = np.stack([v[0] * inv, v[1] * inv, v[2] * inv], axis=-1).astype(F32)
    o = np.broadcast_to(np.array(list(cam.pos)[:3], F32), d.shape).copy()
    return o.reshape(-1, 3), d.reshape(-1, 3)


def tile_order(W, H):
    idx = np.arange(W * H, dtype=np.int64).reshape(H, W)
    th, tw = H // 8, W // 8
    assert th * 8 == H and tw * 8 == W, "the tile order wants multiples of 8"
    return idx.reshape(th, 8, tw, 8).transpose(0, 2, 1, 3).reshape(-1)


def fmt(v):
    return f"{statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]"


def timed_dispatch(r):
    r.dispatch()
    ms, launches = r.kernel_time_ms(reset=True)  # synchronises
    assert launches == 1, launches
    return ms


def probe_cfg(rm, torch, cfg, rounds, warmup):
    W, H, bounces, aa = CFGS[cfg]
    n = W * H
    u = rm.sweep_uniforms(60, 120, bounces, aa, rm.RM_SHADOW_SOFT)
    o, d = primary_rays(u, W, H, aa)
    p = tile_order(W, H)
    dev = torch.device("cuda", torch.cuda.current_device())
    to, td = torch.from_numpy(o[p]).to(dev), torch.from_numpy(d[p]).to(dev)

    plain = rm.Renderer(W, H)  # RGBA8, as bench.py renders the frame
    gb = rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER)
    for r in (plain, gb):
        r.set_uniforms(u)
    # the same values first: the G-buffer against the trace of these rays, and the colour image
    gb.dispatch()
    g = gb.read_gbuffer().reshape(-1)[p]
    tr = gb.trace(to, td, HITN)
    gb.synchronize()
    t = tr.cpu().numpy().view(np.uint32)
    want = np.concatenate([t[:, 0:2], t[:, 6:9], t[:, 3:6]], axis=1)  # t, id, normal, albedo
    same = bool((g.view(np.uint32).reshape(-1, 8) == want).all())
    plain.dispatch()
    same_img = plain.read_rgba8().tobytes() == gb.read_rgba8().tobytes()
    print(f"cfg {cfg}: {W}x{H}, {bounces} bounce(s), AA {'on' if aa else 'off'}; "
          f"{int((g['t'] != -1.0).sum())} of {n} primary rays hit")
    print(f"check  G-buffer == trace(HIT | NORMAL) of the same rays, bit for bit: {same}")
    print(f"check  RGBA8 of the G-buffer context == the plain context's, byte for byte: {same_img}")
    if not (same and same_img):
        sys.exit("probe_gbuffer: the values differ")
    del tr

    for r in (plain, gb):
        r.enable_timing(True)
    src = torch.zeros(n * 8, dtype=torch.float32, device=dev)
    dst = torch.empty_like(src)
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]

    def a_plain():
        return timed_dispatch(plain)

    def b_gbuf():
        return timed_dispatch(gb)

    def c_plain_trace():
        ms = timed_dispatch(plain)
        keep = plain.trace(to, td, HITN)  # (the result tensor lives until its kernel has run)
        ms2, launches = plain.kernel_time_ms(reset=True)
        assert launches == 1, launches
        del keep
        return ms + ms2

    def copy32():
        ev[0].record()
        dst.copy_(src)
        ev[1].record()
        ev[1].synchronize()
        return ev[0].elapsed_time(ev[1])

    variants = {"(a) plain": a_plain, "(b) gbuffer": b_gbuf, "(c) plain+trace": c_plain_trace, "copy32": copy32}
    for _ in range(warmup):
        for fn in variants.values():
            fn()
    res = {k: [] for k in variants}
    for _ in range(rounds):
        for k, fn in variants.items():  # alternating: drift hits every variant alike
            res[k].append(fn())
    print(f"{'variant':<16} {'median [min, max] ms':<30} ({rounds} rounds, alternating)")
    for k, v in res.items():
        print(f"{k:<16} {fmt(v)}")
    a, b, c, cp = (statistics.median(res[k]) for k in variants)
    print(f"(b) - (a) = {b - a:+.4f} ms = {(b - a) / cp:.2f} x copy32 ({n * 32 / 1e6:.1f} MB; "
          f"the copy moves {2 * n * 32 / (cp * 1e-3) / 1e12:.2f} TB/s, read + write)")
    print(f"(c) - (b) = {c - b:+.4f} ms; (b) / (c) = {b / c:.3f}")
    apart = max(res["(b) gbuffer"]) < min(res["(c) plain+trace"])
    print(f"condition: (b) below (c) by more than the spreads overlap "
          f"(max (b) {max(res['(b) gbuffer']):.4f} < min (c) {min(res['(c) plain+trace']):.4f}): {apart}\n")
    plain.close()
    gb.close()
    return apart


def child(cfg, frames):
    """One process of --waves-ab: median kernel ms of `frames` G-buffer dispatches."""
    import torch  # noqa: F401
    import rmarch as rm
    W, H, bounces, aa = CFGS[cfg]
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER) as r:
        r.set_uniforms(rm.sweep_uniforms(60, 120, bounces, aa, rm.RM_SHADOW_SOFT))
        r.enable_timing(True)
        ms = [timed_dispatch(r) for _ in range(frames + 3)][3:]
    print(json.dumps({"ms": statistics.median(ms)}))


def waves_ab(lib, cfgs, rounds, frames):
    libs = {"librm.so (RM_GBUF_WAVES default)": None, os.path.basename(lib): os.path.abspath(lib)}
    for cfg in cfgs:
        res = {k: [] for k in libs}
        for _ in range(rounds):
            for k, path in libs.items():  # alternating processes
                env = dict(os.environ)
                if path:
                    env["RM_LIBRM"] = path
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(cfg),
                                      "--frames", str(frames)], env=env, capture_output=True, text=True,
                                     timeout=120, check=True).stdout
                res[k].append(json.loads(out.strip().split("\n")[-1])["ms"])
        print(f"cfg {cfg}, G-buffer dispatch, kernel ms, median [min, max] of {rounds} alternating processes "
              f"(each the median of {frames} frames)")
        for k, v in res.items():
            print(f"  {k:<36} {fmt(v)}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cfg", type=int, nargs="+", default=[2, 3], choices=sorted(CFGS))
    ap.add_argument("--waves-ab", metavar="LIB")
    ap.add_argument("--frames", type=int, default=15)
    ap.add_argument("--child", type=int)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.frames)
    if a.waves_ab:
        return waves_ab(a.waves_ab, a.cfg, a.rounds, a.frames)
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_gbuffer: no GPU (nothing here is measured on a CPU)")
    ok = [probe_cfg(rm, torch, cfg, a.rounds, a.warmup) for cfg in a.cfg]
    if not all(ok):
        print("the fused path is NOT faster than plain + trace beyond the spreads on every frame")


if __name__ == "__main__":
    main()
