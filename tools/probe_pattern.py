"""Sample-pattern frames against the frame kernels (diagnostic, not product).

  python tools/probe_pattern.py [--rounds 5] [--out profiles/pattern_probe.txt]

One MI355X, one process, one RGBA8 context: cfg 3 (3840x2160, 3 bounces, soft shadows) on
12 sweep frames (0, 10, .. 110 of 120).  For every frame the variants alternate within
every round after a warm-up round, every launch timed alone by the context's own events
(rm_enable_timing / rm_kernel_time_ms):

  AA on, AA on'    rm_dispatch with AA = 1 (k_sample), twice: the A/A pair
  REFERENCE        rm_dispatch_pattern, RM_PATTERN_REFERENCE: the same image by k_pattern
  GRID2, GRID4     rm_dispatch_pattern, 4 and 16 re-centred samples
  AA off, AA off'  rm_dispatch with AA = 0 (k_pixel), twice
  n = 1            rm_dispatch_pattern, one sample at (0, 0): the same image by k_pattern_one

Per variant: the sweep mean of the per-frame medians, and a round's sweep mean for every
round.  The bar for REFERENCE against AA on (equal work) is the project's own: the
difference of the rounds' sweep means stays within twice the largest A/A difference of
those rounds.  Before timing, on frame 60: REFERENCE gives the AA-on image and n = 1 the
AA-off image, byte for byte.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pattern_probe.txt"))
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_pattern: no GPU (nothing here is measured on a CPU)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/probe_pattern.py --rounds {a.rounds}: kernel ms by the context's events, one process, one "
        f"context, variants alternating per frame")
    on = {f: rm.sweep_uniforms(f, 120, BOUNCES, True, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    off = {f: rm.sweep_uniforms(f, 120, BOUNCES, False, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    pat = {k: rm.sample_pattern(v) for k, v in (("REFERENCE", rm.RM_PATTERN_REFERENCE), ("GRID2", rm.RM_PATTERN_GRID2),
                                                ("GRID4", rm.RM_PATTERN_GRID4))}
    pat["n = 1"] = rm.custom_pattern([0.0], [0.0])
    samples = {"AA on": 4, "AA on'": 4, "REFERENCE": 4, "GRID2": 4, "GRID4": 16, "AA off": 1, "AA off'": 1, "n = 1": 1}
    with rm.Renderer(W, H) as r:
        r.dispatch(on[60])
        b = r.read_rgba8()
        r.dispatch_pattern(on[60], pat["REFERENCE"])
        same_on = r.read_rgba8().tobytes() == b.tobytes()
        r.dispatch(off[60])
        c = r.read_rgba8()
        r.dispatch_pattern(off[60], pat["n = 1"])
        same_off = r.read_rgba8().tobytes() == c.tobytes()
        say(f"cfg 3: {W}x{H}, {BOUNCES} bounces, soft shadows, {len(FRAMES)} sweep frames, {a.rounds} rounds")
        say(f"check  frame 60, REFERENCE == the AA-on image, byte for byte: {same_on}")
        say(f"check  frame 60, n = 1 at (0, 0) == the AA-off image, byte for byte: {same_off}")
        if not (same_on and same_off):
            sys.exit("probe_pattern: the values differ")
        r.enable_timing(True)
        r.kernel_time_ms(reset=True)
        variants = {"AA on": lambda f: r.dispatch(on[f]), "AA on'": lambda f: r.dispatch(on[f]),
                    "REFERENCE": lambda f: r.dispatch_pattern(on[f], pat["REFERENCE"]),
                    "GRID2": lambda f: r.dispatch_pattern(on[f], pat["GRID2"]),
                    "GRID4": lambda f: r.dispatch_pattern(on[f], pat["GRID4"]),
                    "AA off": lambda f: r.dispatch(off[f]), "AA off'": lambda f: r.dispatch(off[f]),
                    "n = 1": lambda f: r.dispatch_pattern(off[f], pat["n = 1"])}
        ms = {k: {f: [] for f in FRAMES} for k in variants}
        for rnd in range(a.rounds + 1):  # round 0 warms every variant up on every frame
            for f in FRAMES:
                for k, fn in variants.items():  # alternating: drift hits every variant alike
                    t = timed(r, lambda: fn(f))
                    if rnd:
                        ms[k][f].append(t)
    med = {k: [statistics.median(ms[k][f]) for f in FRAMES] for k in variants}
    mean = {k: statistics.fmean(v) for k, v in med.items()}
    per_round = {k: [statistics.fmean(ms[k][f][i] for f in FRAMES) for i in range(a.rounds)] for k in variants}
    say(f"{'variant':<11} {'ms per frame: sweep mean [min, max over the frames]':<52} {'us per Msample-ray':<19} rounds' sweep means")
    for k in variants:
        rays = W * H * samples[k] / 1e6
        say(f"{k:<11} " + f"{mean[k]:.4f} [{min(med[k]):.4f}, {max(med[k]):.4f}]".ljust(52) +
            f" {1e3 * mean[k] / rays:<19.3f} " + " ".join(f"{x:.4f}" for x in per_round[k]))

    def against(k, base, twin):
        d = [x - y for x, y in zip(per_round[k], per_round[base])]
        aa = [x - y for x, y in zip(per_round[twin], per_round[base])]
        bar = 2 * max(abs(x) for x in aa)
        worst = max(abs(x) for x in d)
        say(f"{k} - {base}: rounds {' '.join(f'{x:+.4f}' for x in d)} ms; A/A ({twin} - {base}) "
            f"{' '.join(f'{x:+.4f}' for x in aa)} ms; largest |difference| {worst:.4f} against the bar "
            f"2 x {bar / 2:.4f} = {bar:.4f}: {'within' if worst <= bar else 'BEYOND'}; ratio of the sweep means "
            f"{mean[k] / mean[base]:.4f}")

    against("REFERENCE", "AA on", "AA on'")
    against("GRID2", "AA on", "AA on'")
    against("n = 1", "AA off", "AA off'")
    say(f"GRID4 per sample-ray / REFERENCE per sample-ray = {(mean['GRID4'] / 16) / (mean['REFERENCE'] / 4):.4f}")
    say(f"n = 1 / AA off = {mean['n = 1'] / mean['AA off']:.3f} (k_pattern_one against k_pixel: the same wave and render)")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
