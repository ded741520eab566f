"""Adaptive supersampling against the full 4x frame and the frame without AA (diagnostic,
not product).

  python tools/probe_adaptive.py [--rounds 5] [--cfg 3 2] [--out profiles/adaptive_probe.txt]

One MI355X, one process, one RGBA8 context per configuration (as bench.py renders it):
cfg 3 (3840x2160, 3 bounces) and cfg 2 (1920x1080, 1 bounce) on the 20 sweep frames
bench.py's --steps 20 samples (frames 0, 6, .. 114 of 120).  For every frame, the
variants alternate within every round after a warm-up round:

  AA on          rm_dispatch with AA = 1 (k_sample: cfg 3 as the benchmark runs it)
  AA off         rm_dispatch with AA = 0 (k_pixel)
  adaptive T     rm_dispatch_adaptive at thresholds 4, 8, 16, 32 and 255: pass 1, the
                 flags, the scan, the list and the refinement, one event pair around all

Kernel time by the context's own events (rm_enable_timing / rm_kernel_time_ms), the
flagged share from rm_aa_refined.  Per variant: the sweep mean of the per-frame medians,
and the range of those medians over the frames.  Threshold 255 flags nothing, so
"adaptive 255 - AA off" is what the three bookkeeping kernels and the empty refinement
launch cost.  Before timing, on frame 60: threshold 255 gives the AA-off image, and an
all-ones mask the AA-on image, byte for byte.

A single launch of these frames ends on its longest waves, and an adaptive
frame is two such launches in a row, so two more sections follow: the same variants with
frames overlapped on 3 contexts, as bench.py issues them (host wall time per frame), and
the refinement's grid size (RM_AA_REFINE_WAVES) on cfg 3.
"""
import argparse
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))

CFGS = {2: (1920, 1080, 1), 3: (3840, 2160, 3)}
THRESHOLDS = (4, 8, 16, 32, 255)
FRAMES = [k * 120 // 20 for k in range(20)]


def timed(r, fn):
    fn()
    ms, launches = r.kernel_time_ms(reset=True)  # synchronises
    assert launches == 1, launches
    return ms


def probe_cfg(rm, cfg, rounds, say):
    W, H, bounces = CFGS[cfg]
    on = {f: rm.sweep_uniforms(f, 120, bounces, True, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    off = {f: rm.sweep_uniforms(f, 120, bounces, False, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    with rm.Renderer(W, H) as r:
        # the same values first
        r.dispatch(off[60])
        a = r.read_rgba8()
        r.dispatch(on[60])
        b = r.read_rgba8()
        r.dispatch_adaptive(off[60], 255)
        same_off = r.read_rgba8().tobytes() == a.tobytes() and r.aa_refined() == 0
        r.dispatch_refine(np.ones((H, W), np.uint8), off[60])
        same_on = r.read_rgba8().tobytes() == b.tobytes() and r.aa_refined() == W * H
        say(f"cfg {cfg}: {W}x{H}, {bounces} bounce(s), soft shadows, {len(FRAMES)} sweep frames, {rounds} rounds")
        say(f"check  frame 60, threshold 255 == the AA-off image, byte for byte: {same_off}")
        say(f"check  frame 60, all-ones mask == the AA-on image, byte for byte: {same_on}")
        if not (same_off and same_on):
            sys.exit("probe_adaptive: the values differ")
        r.enable_timing(True)
        r.kernel_time_ms(reset=True)
        variants = {"AA on": lambda f: r.dispatch(on[f]), "AA off": lambda f: r.dispatch(off[f])}
        for t in THRESHOLDS:
            variants[f"adaptive {t}"] = lambda f, t=t: r.dispatch_adaptive(off[f], t)
        ms = {k: {f: [] for f in FRAMES} for k in variants}
        share = {k: {} for k in variants}
        for rnd in range(rounds + 1):  # round 0 warms every variant up on every frame
            for f in FRAMES:
                for k, fn in variants.items():  # alternating: drift hits every variant alike
                    t = timed(r, lambda: fn(f))
                    if rnd:
                        ms[k][f].append(t)
                    elif k.startswith("adaptive"):
                        share[k][f] = r.aa_refined() / (W * H)
    med = {k: [statistics.median(ms[k][f]) for f in FRAMES] for k in variants}
    mean = {k: statistics.fmean(v) for k, v in med.items()}
    say(f"{'variant':<14} {'ms per frame: sweep mean [min, max over the frames]':<54} {'flagged share: mean [min, max]'}")
    for k in variants:
        line = f"{k:<14} {mean[k]:.4f} [{min(med[k]):.4f}, {max(med[k]):.4f}]".ljust(69)
        if share[k]:
            s = list(share[k].values())
            line += f" {statistics.fmean(s):.4f} [{min(s):.4f}, {max(s):.4f}]"
        say(line)
    say(f"bookkeeping: adaptive 255 - AA off = {mean['adaptive 255'] - mean['AA off']:+.4f} ms per frame")
    for t in THRESHOLDS[:-1]:
        k = f"adaptive {t}"
        slower = sum(1 for x, y in zip(med[k], med["AA on"]) if x >= y)
        say(f"{k} / AA on = {mean[k] / mean['AA on']:.3f} of the sweep's time; "
            f"not faster than AA on on {slower} of {len(FRAMES)} frames")
    say("")


def probe_grid(rm, rounds, say):
    """The refinement's grid size (RM_AA_REFINE_WAVES, read by rm_create): cfg 3 at
    threshold 8 and with an all-ones mask, one context per grid size, alternating."""
    W, H, bounces = CFGS[3]
    frames = FRAMES[::4]
    off = {f: rm.sweep_uniforms(f, 120, bounces, False, rm.RM_SHADOW_SOFT) for f in frames}
    ctx = {}
    for waves in (0, 8192, 16384, 32768, 65535):
        if waves:
            os.environ["RM_AA_REFINE_WAVES"] = str(waves)
        else:
            os.environ.pop("RM_AA_REFINE_WAVES", None)
        ctx[waves] = rm.Renderer(W, H)
        ctx[waves].enable_timing(True)
    os.environ.pop("RM_AA_REFINE_WAVES", None)
    ones = np.ones((H, W), np.uint8)
    for r in ctx.values():
        r.dispatch_refine(ones, off[frames[0]])  # allocates the context's buffers
        r.kernel_time_ms(reset=True)
    ms = {w: ([], []) for w in ctx}
    for rnd in range(rounds + 1):
        for f in frames:
            for w, r in ctx.items():
                a = timed(r, lambda: r.dispatch_adaptive(off[f], 8))
                b = timed(r, lambda: r.dispatch_refine(ones, off[f]))
                if rnd:
                    ms[w][0].append(a)
                    ms[w][1].append(b)
    say(f"refinement grid (RM_AA_REFINE_WAVES), cfg 3, frames {frames}, {rounds} rounds: mean ms per frame")
    say(f"{'waves':<18} {'adaptive 8':<12} {'all-ones mask (every pixel refined)'}")
    for w, (a, b) in ms.items():
        say(f"{(str(w) if w else 'default'):<18} {statistics.fmean(a):<12.4f} {statistics.fmean(b):.4f}")
    say("")
    for r in ctx.values():
        r.close()


def probe_throughput(rm, cfg, rounds, say):
    """Frames overlapped as bench.py issues them: 3 contexts, each on its own stream, 60
    frames issued round-robin without waiting, then one wait: host wall time per frame."""
    import time
    W, H, bounces = CFGS[cfg]
    on = [rm.sweep_uniforms(f, 120, bounces, True, rm.RM_SHADOW_SOFT) for f in FRAMES]
    off = [rm.sweep_uniforms(f, 120, bounces, False, rm.RM_SHADOW_SOFT) for f in FRAMES]
    ctx = [rm.Renderer(W, H) for _ in range(3)]
    variants = {"AA on": lambda r, k: r.dispatch(on[k]), "AA off": lambda r, k: r.dispatch(off[k]),
                "adaptive 8": lambda r, k: r.dispatch_adaptive(off[k], 8),
                "adaptive 32": lambda r, k: r.dispatch_adaptive(off[k], 32)}
    n = 60
    ms = {k: [] for k in variants}
    for rnd in range(rounds + 1):
        for name, fn in variants.items():
            for r in ctx:
                r.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                fn(ctx[k % 3], k % len(FRAMES))
            for r in ctx:
                r.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / n)
    say(f"throughput, cfg {cfg}: 3 contexts on their own streams, {n} frames issued round-robin, one wait; "
        f"host wall ms per frame, median [min, max] of {rounds} rounds")
    for name, v in ms.items():
        say(f"{name:<14} {statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]")
    say(f"adaptive 8 / AA on = {statistics.median(ms['adaptive 8']) / statistics.median(ms['AA on']):.3f}")
    say("")
    for r in ctx:
        r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--cfg", type=int, nargs="+", default=[3, 2], choices=sorted(CFGS))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_probe.txt"))
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_adaptive: no GPU (nothing here is measured on a CPU)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/probe_adaptive.py --rounds {a.rounds} --cfg {' '.join(map(str, a.cfg))}: kernel ms by the "
        f"context's events, one process, one context per configuration, variants alternating per frame")
    for cfg in a.cfg:
        probe_cfg(rm, cfg, a.rounds, say)
    for cfg in a.cfg:
        probe_throughput(rm, cfg, a.rounds, say)
    if 3 in a.cfg:
        probe_grid(rm, a.rounds, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
