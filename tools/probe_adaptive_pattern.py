"""Pattern refinement in the adaptive calls against the calls it joins (diagnostic, not
product).

  python tools/probe_adaptive_pattern.py [--rounds 5] [--out profiles/adaptive_pattern_probe.txt]

One MI355X, one process: cfg 3's shape (3840x2160, 3 bounces, soft shadows) on 12 sweep frames
(0, 10, .. 110 of 120), one RGBA8 + G-buffer context for the adaptive calls and rm_dispatch, one
plain RGBA8 context for the whole-frame rm_dispatch_pattern (G-buffer contexts refuse it).  The
criteria are rm_aa_criteria_init's (ID | DEPTH | NORMAL).  For every frame the variants alternate
within every round after a warm-up round, every call timed alone by its context's own events
(rm_enable_timing / rm_kernel_time_ms: one pair brackets pass 1 through the refinement):

  edges, edges'      rm_dispatch_adaptive_edges, twice: the A/A pair (k_adapt_refine)
  A REFERENCE        rm_dispatch_adaptive_pattern, RM_PATTERN_REFERENCE: the same image by
                     k_adapt_refine_pattern (equal work)
  A GRID2/3/4        rm_dispatch_adaptive_pattern, 4, 9 and 16 centred samples on the flagged pixels
  W GRID2/3/4        rm_dispatch_pattern of the same pattern over the whole frame (plain context)
  AA off, AA off'    rm_dispatch with AA = 0 on the G-buffer context: pass 1 alone, twice
  A n = 1            rm_dispatch_adaptive_pattern, one sample at (0, 0): pass 1 and the flagged
                     pixels once more by k_adapt_refine_pattern_one

Per variant: the sweep mean of the per-frame medians, and a round's sweep mean for every round.
The bar for A REFERENCE against edges (equal work) is the project's own: the difference of the
rounds' sweep means stays within twice the largest A/A difference of those rounds.  Before
timing, on frame 60: A REFERENCE gives rm_dispatch_adaptive_edges' image and mask, byte for byte,
and the flagged share is printed.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))

W, H, BOUNCES = 3840, 2160, 3
FRAMES = [k * 120 // 12 for k in range(12)]


def timed(r, fn):
    fn()
    ms, launches = r.kernel_time_ms(reset=True)  # synchronises
    assert launches == 1, launches
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "adaptive_pattern_probe.txt"))
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_adaptive_pattern: no GPU (nothing here is measured on a CPU)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/probe_adaptive_pattern.py --rounds {a.rounds}: ms by the contexts' events, one process, "
        f"variants alternating per frame")
    off = {f: rm.sweep_uniforms(f, 120, BOUNCES, False, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    pat = {k: rm.sample_pattern(v) for k, v in (("REFERENCE", rm.RM_PATTERN_REFERENCE), ("GRID2", rm.RM_PATTERN_GRID2),
                                                ("GRID3", rm.RM_PATTERN_GRID3), ("GRID4", rm.RM_PATTERN_GRID4))}
    pat["n = 1"] = rm.custom_pattern([0.0], [0.0])
    n_of = {"edges": 4, "edges'": 4, "A REFERENCE": 4, "A GRID2": 4, "A GRID3": 9, "A GRID4": 16, "A n = 1": 1}
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER) as r, rm.Renderer(W, H) as p:
        r.dispatch_adaptive_edges(off[60])
        img, mask, flagged60 = r.read_rgba8(), r.read_aa_mask(), r.aa_refined()
        r.dispatch_adaptive_pattern(off[60], None, pat["REFERENCE"])
        same = r.read_rgba8().tobytes() == img.tobytes() and r.read_aa_mask().tobytes() == mask.tobytes()
        say(f"cfg 3's shape: {W}x{H}, {BOUNCES} bounces, soft shadows, {len(FRAMES)} sweep frames, {a.rounds} rounds; "
            f"criteria ID | DEPTH | NORMAL at the defaults")
        say(f"check  frame 60, A REFERENCE == rm_dispatch_adaptive_edges' image and mask, byte for byte: {same}")
        say(f"       frame 60 flags {flagged60} of {W * H} pixels ({100.0 * flagged60 / (W * H):.3f} %)")
        if not same:
            sys.exit("probe_adaptive_pattern: the values differ")
        flagged = {}
        for f in FRAMES:
            r.dispatch_adaptive_edges(off[f])
            flagged[f] = r.aa_refined()
        say("flagged pixels per frame: " + " ".join(str(flagged[f]) for f in FRAMES) +
            f" (mean share {100.0 * statistics.fmean(flagged.values()) / (W * H):.3f} %)")
        for c in (r, p):
            c.enable_timing(True)
            c.kernel_time_ms(reset=True)
        variants = {"edges": (r, lambda f: r.dispatch_adaptive_edges(off[f])),
                    "edges'": (r, lambda f: r.dispatch_adaptive_edges(off[f])),
                    "A REFERENCE": (r, lambda f: r.dispatch_adaptive_pattern(off[f], None, pat["REFERENCE"])),
                    "A GRID2": (r, lambda f: r.dispatch_adaptive_pattern(off[f], None, pat["GRID2"])),
                    "W GRID2": (p, lambda f: p.dispatch_pattern(off[f], pat["GRID2"])),
                    "A GRID3": (r, lambda f: r.dispatch_adaptive_pattern(off[f], None, pat["GRID3"])),
                    "W GRID3": (p, lambda f: p.dispatch_pattern(off[f], pat["GRID3"])),
                    "A GRID4": (r, lambda f: r.dispatch_adaptive_pattern(off[f], None, pat["GRID4"])),
                    "W GRID4": (p, lambda f: p.dispatch_pattern(off[f], pat["GRID4"])),
                    "AA off": (r, lambda f: r.dispatch(off[f])), "AA off'": (r, lambda f: r.dispatch(off[f])),
                    "A n = 1": (r, lambda f: r.dispatch_adaptive_pattern(off[f], None, pat["n = 1"]))}
        ms = {k: {f: [] for f in FRAMES} for k in variants}
        for rnd in range(a.rounds + 1):  # round 0 warms every variant up on every frame
            for f in FRAMES:
                for k, (ctx, fn) in variants.items():  # alternating: drift hits every variant alike
                    t = timed(ctx, lambda: fn(f))
                    if rnd:
                        ms[k][f].append(t)
    med = {k: [statistics.median(ms[k][f]) for f in FRAMES] for k in variants}
    mean = {k: statistics.fmean(v) for k, v in med.items()}
    per_round = {k: [statistics.fmean(ms[k][f][i] for f in FRAMES) for i in range(a.rounds)] for k in variants}
    say(f"{'variant':<12} {'ms per frame: sweep mean [min, max over the frames]':<52} rounds' sweep means")
    for k in variants:
        say(f"{k:<12} " + f"{mean[k]:.4f} [{min(med[k]):.4f}, {max(med[k]):.4f}]".ljust(52) + " " +
            " ".join(f"{x:.4f}" for x in per_round[k]))

    def against(k, base, twin):
        d = [x - y for x, y in zip(per_round[k], per_round[base])]
        aa = [x - y for x, y in zip(per_round[twin], per_round[base])]
        bar = 2 * max(abs(x) for x in aa)
        worst = max(abs(x) for x in d)
        say(f"{k} - {base}: rounds {' '.join(f'{x:+.4f}' for x in d)} ms; A/A ({twin} - {base}) "
            f"{' '.join(f'{x:+.4f}' for x in aa)} ms; largest |difference| {worst:.4f} against the bar "
            f"2 x {bar / 2:.4f} = {bar:.4f}: {'within' if worst <= bar else 'BEYOND'}; ratio of the sweep means "
            f"{mean[k] / mean[base]:.4f}")

    against("A REFERENCE", "edges", "edges'")
    against("A n = 1", "AA off", "AA off'")
    # the refinement's share: the call less pass 1 alone, over the sample-rays of the flagged pixels
    say("the refinement beyond pass 1 (call - AA off, per frame, then the sweep mean), per million sample-rays "
        "over the flagged pixels:")
    for k, n in n_of.items():
        if k.endswith("'"):
            continue
        us = [1e3 * (m - o) / (flagged[f] * n / 1e6) for m, o, f in zip(med[k], med["AA off"], FRAMES)]
        say(f"  {k:<12} {mean[k] - mean['AA off']:.4f} ms beyond pass 1, {statistics.fmean(us):.2f} us per Msample-ray "
            f"[{min(us):.2f}, {max(us):.2f}]")
    for g in ("GRID2", "GRID3", "GRID4"):
        rays = W * H * n_of[f"A {g}"] / 1e6
        say(f"{g}: adaptive {mean[f'A {g}']:.4f} ms = {mean[f'A {g}'] / mean['edges']:.3f} x rm_dispatch_adaptive_edges, "
            f"{mean[f'A {g}'] / mean[f'W {g}']:.3f} x the whole-frame rm_dispatch_pattern ({mean[f'W {g}']:.4f} ms, "
            f"{1e3 * mean[f'W {g}'] / rays:.2f} us per Msample-ray), {mean[f'A {g}'] / mean['AA off']:.3f} x pass 1 alone")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
