"""Geometry-edge adaptive supersampling against colour contrast, the full 4x frame and the
frame without AA (diagnostic, not product).

  python tools/probe_adaptive_edges.py [--rounds 5] [--out profiles/adaptive_edges_probe.txt]

One MI355X, one process, cfg 3 (3840x2160, 3 bounces, soft shadows) on the 20 sweep frames
bench.py's --steps 20 samples (frames 0, 6, .. 114 of 120).  Two contexts: a plain RGBA8 one,
as bench.py renders, and an RGBA8 + G-buffer one.  For every frame the variants alternate
within every round after a warm-up round:

  AA on              rm_dispatch with AA = 1, plain context (cfg 3 as the benchmark runs it)
  AA off, G-buffer   rm_dispatch with AA = 0 on the G-buffer context (pass 1 of every row below)
  colour 8           rm_dispatch_adaptive at threshold 8, plain context
  ID                 rm_dispatch_adaptive_edges, RM_AA_EDGE_ID alone
  ID|DEPTH|NORMAL    the defaults of rm_aa_criteria_init (depth_rel 0.05, normal_cos 0.9)
  all bits           the five criteria, colour threshold 8
  DEPTH inf          DEPTH at depth_rel = +inf: flags nothing, so "DEPTH inf - AA off, G-buffer"
                     is what the classifier, the scan, the scatter and the empty refinement
                     cost; once per lane mapping of the classifier (RM_AA_EDGES_NAIVE)
  ID|DEPTH|NORMAL, plain form
                     the defaults again with the classifier's plain form

Kernel time by the context's own events (rm_enable_timing / rm_kernel_time_ms), one frame at a
time; the flagged share from rm_aa_refined.  Per variant: the sweep mean of the per-frame
medians, and the range of those medians over the frames.  Then the same variants with frames
overlapped on 3 contexts, as bench.py issues them (host wall time per frame).

Before timing, on frame 60 at full size: the image of every edge variant equals a plain
context's rm_dispatch_refine_device run with that variant's mask, byte for byte, and both
lane mappings give the same mask.
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))

W, H, BOUNCES = 3840, 2160, 3
FRAMES = [k * 120 // 20 for k in range(20)]
COLOUR_BOOKKEEPING_MS = 0.086  # profiles/adaptive_probe.txt: adaptive 255 - AA off, cfg 3


class naive_form:
    """The classifier's plain form for the calls inside (RM_AA_EDGES_NAIVE is read by every call)."""

    def __enter__(self):
        os.environ["RM_AA_EDGES_NAIVE"] = "1"

    def __exit__(self, *a):
        os.environ.pop("RM_AA_EDGES_NAIVE", None)


def variants(rm, on, off):
    """name -> (which context, call(r, frame), flags anything)"""
    ID, DEP, NOR, ALB, COL = (rm.RM_AA_EDGE_ID, rm.RM_AA_EDGE_DEPTH, rm.RM_AA_EDGE_NORMAL, rm.RM_AA_EDGE_ALBEDO,
                              rm.RM_AA_EDGE_COLOR)
    inf = float("inf")

    def plain_form(fn):
        def call(r, f):
            with naive_form():
                fn(r, f)
        return call

    idn = lambda r, f: r.dispatch_adaptive_edges(off[f], ID | DEP | NOR)  # noqa: E731
    dinf = lambda r, f: r.dispatch_adaptive_edges(off[f], DEP, depth_rel=inf)  # noqa: E731
    return {
        "AA on": ("plain", lambda r, f: r.dispatch(on[f]), False),
        "AA off, G-buffer": ("gbuf", lambda r, f: r.dispatch(off[f]), False),
        "colour 8": ("plain", lambda r, f: r.dispatch_adaptive(off[f], 8), True),
        "ID": ("gbuf", lambda r, f: r.dispatch_adaptive_edges(off[f], ID), True),
        "ID|DEPTH|NORMAL": ("gbuf", idn, True),
        "all bits": ("gbuf", lambda r, f: r.dispatch_adaptive_edges(off[f], ID | DEP | NOR | ALB | COL), True),
        "DEPTH inf": ("gbuf", dinf, True),
        "DEPTH inf, plain form": ("gbuf", plain_form(dinf), True),
        "ID|DEPTH|NORMAL, plain form": ("gbuf", plain_form(idn), True),
    }


def check(rm, ctx, var, say):
    import numpy as np
    import torch
    p, g = ctx["plain"], ctx["gbuf"]
    masks = {}
    for name, (which, fn, flags) in var.items():
        if which != "gbuf" or not flags:
            continue
        fn(g, 60)
        m, img = g.read_aa_mask(), g.read_rgba8()
        masks[name] = m
        dev = torch.from_numpy(m).to(f"cuda:{p.device}")
        torch.cuda.synchronize()
        p.dispatch_refine(dev.data_ptr())
        same = p.read_rgba8().tobytes() == img.tobytes() and p.aa_refined() == int(m.sum()) == g.aa_refined()
        say(f"check  frame 60, {name}: {int(m.sum())} flagged; the image == rm_dispatch_refine_device with "
            f"the same mask on a plain context, byte for byte: {same}")
        if not same:
            sys.exit("probe_adaptive_edges: the values differ")
    same = (np.array_equal(masks["DEPTH inf"], masks["DEPTH inf, plain form"]) and not masks["DEPTH inf"].any()
            and np.array_equal(masks["ID|DEPTH|NORMAL"], masks["ID|DEPTH|NORMAL, plain form"]))
    say(f"check  frame 60, both lane mappings give the same mask, and DEPTH inf flags nothing: {same}")
    if not same:
        sys.exit("probe_adaptive_edges: the lane mappings differ")


def timed(r, fn):
    fn()
    ms, launches = r.kernel_time_ms(reset=True)  # synchronises
    assert launches == 1, launches
    return ms


def probe_kernel_time(rm, rounds, say):
    on = {f: rm.sweep_uniforms(f, 120, BOUNCES, True, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    off = {f: rm.sweep_uniforms(f, 120, BOUNCES, False, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    var = variants(rm, on, off)
    ctx = {"plain": rm.Renderer(W, H), "gbuf": rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER)}
    ctx["plain"].set_uniforms(off[60])
    say(f"cfg 3: {W}x{H}, {BOUNCES} bounces, soft shadows, {len(FRAMES)} sweep frames, {rounds} rounds")
    check(rm, ctx, var, say)
    for r in ctx.values():
        r.enable_timing(True)
        r.kernel_time_ms(reset=True)
    ms = {k: {f: [] for f in FRAMES} for k in var}
    share = {k: {} for k in var}
    for rnd in range(rounds + 1):  # round 0 warms every variant up on every frame
        for f in FRAMES:
            for k, (which, fn, flags) in var.items():  # alternating: drift hits every variant alike
                r = ctx[which]
                t = timed(r, lambda: fn(r, f))
                if rnd:
                    ms[k][f].append(t)
                elif flags:
                    share[k][f] = r.aa_refined() / (W * H)
    for r in ctx.values():
        r.close()
    med = {k: [statistics.median(ms[k][f]) for f in FRAMES] for k in var}
    mean = {k: statistics.fmean(v) for k, v in med.items()}
    say(f"{'variant':<28} {'ms per frame: sweep mean [min, max over the frames]':<54} {'flagged share: mean [min, max]'}")
    for k in var:
        line = f"{k:<28} {mean[k]:.4f} [{min(med[k]):.4f}, {max(med[k]):.4f}]".ljust(83)
        if share[k]:
            s = list(share[k].values())
            line += f" {statistics.fmean(s):.4f} [{min(s):.4f}, {max(s):.4f}]"
        say(line)
    base = mean["AA off, G-buffer"]
    say(f"bookkeeping, two-pair form: DEPTH inf - AA off, G-buffer = {mean['DEPTH inf'] - base:+.4f} ms per frame")
    say(f"bookkeeping, plain form:    DEPTH inf - AA off, G-buffer = {mean['DEPTH inf, plain form'] - base:+.4f} ms per frame")
    say(f"bookkeeping, colour classifier (profiles/adaptive_probe.txt, adaptive 255 - AA off): "
        f"{COLOUR_BOOKKEEPING_MS:+.4f} ms per frame")
    for k in ("ID", "ID|DEPTH|NORMAL", "all bits", "ID|DEPTH|NORMAL, plain form"):
        for against in ("colour 8", "AA on"):
            slower = sum(1 for x, y in zip(med[k], med[against]) if x >= y)
            say(f"{k} / {against} = {mean[k] / mean[against]:.3f} of the sweep's time; "
                f"not faster on {slower} of {len(FRAMES)} frames")
    say("")


def probe_throughput(rm, rounds, say):
    """Frames overlapped as bench.py issues them: 3 contexts of each kind, each on its own stream,
    60 frames issued round-robin without waiting, then one wait: host wall time per frame."""
    on = [rm.sweep_uniforms(f, 120, BOUNCES, True, rm.RM_SHADOW_SOFT) for f in FRAMES]
    off = [rm.sweep_uniforms(f, 120, BOUNCES, False, rm.RM_SHADOW_SOFT) for f in FRAMES]
    var = variants(rm, on, off)
    ctx = {"plain": [rm.Renderer(W, H) for _ in range(3)],
           "gbuf": [rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER) for _ in range(3)]}
    n = 60
    ms = {k: [] for k in var}
    for rnd in range(rounds + 1):
        for name, (which, fn, _) in var.items():
            rs = ctx[which]
            for r in rs:
                r.synchronize()
            t0 = time.perf_counter()
            for k in range(n):
                fn(rs[k % 3], k % len(FRAMES))
            for r in rs:
                r.synchronize()
            if rnd:
                ms[name].append((time.perf_counter() - t0) * 1e3 / n)
    say(f"throughput, cfg 3: 3 contexts on their own streams, {n} frames issued round-robin, one wait; "
        f"host wall ms per frame, median [min, max] of {rounds} rounds")
    for name, v in ms.items():
        say(f"{name:<28} {statistics.median(v):.4f} [{min(v):.4f}, {max(v):.4f}]")
    for k in ("ID", "ID|DEPTH|NORMAL", "all bits"):
        say(f"{k} / colour 8 = {statistics.median(ms[k]) / statistics.median(ms['colour 8']):.3f}, "
            f"/ AA on = {statistics.median(ms[k]) / statistics.median(ms['AA on']):.3f}")
    say("")
    for rs in ctx.values():
        for r in rs:
            r.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_edges_probe.txt"))
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_adaptive_edges: no GPU (nothing here is measured on a CPU)")
    os.environ.pop("RM_AA_EDGES_NAIVE", None)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/probe_adaptive_edges.py --rounds {a.rounds}: kernel ms by the context's events, one process, "
        f"variants alternating per frame")
    probe_kernel_time(rm, a.rounds, say)
    probe_throughput(rm, a.rounds, say)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
