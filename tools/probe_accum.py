"""Progressive accumulation against what a caller had to do without it (diagnostic, not
product).

  python tools/probe_accum.py [--rounds 5] [--out profiles/accum_probe.txt]

One MI355X, one process: cfg 3's shape (3840x2160, 3 bounces, soft shadows) on 12 sweep frames
(0, 10, .. 110 of 120).  For every frame the variants alternate within every round after a
warm-up round.  For each of jitter1 (one sample), GRID2 (4) and GRID4 (16):

  (a) pattern, pattern'   rm_dispatch_pattern on an RGBA8 context, twice: the A/A pair
  (b) accum, restart      rm_dispatch_accumulate on that context in steady state (N > 0: the sum
                          is read) and with RM_ACCUM_RESTART (N = 0: it is only written)
  (c) caller              what the parent commit offered: rm_dispatch_pattern on an RGBA32F
                          context plus the caller's own blend on the same stream, torch's
                          sum += img; out = sum / N.  The C-ABI hands out no device pointer to the
                          RGBA32F image, so the blend runs on a device tensor of the image's shape
                          and type: the bytes moved are the image's, and the readback a real
                          caller also pays is left out, in (c)'s favour.
  (d) copy                a device-to-device copy of 32 B per pixel, the bytes the fused tail adds
                          (16 read, 16 written)

Every library launch is timed alone by its context's own events (rm_enable_timing /
rm_kernel_time_ms), the torch work by a pair of torch events on the stream the RGBA32F context
renders on; (c) is the sum of the two, without the gap between the launches.

Per variant: the sweep mean of the per-frame medians, and a round's sweep mean for every round.
(b) - (a) is held to the project's bar, twice the largest A/A difference of the same rounds,
and set beside (d); the claim is that the slowest round of (b) is below the fastest of (c).
Before timing, on frame 60: (b) after a restart is (a)'s image byte for byte.
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "accum_probe.txt"))
    a = ap.parse_args()
    import torch
    import rmarch as rm

    if not torch.cuda.is_available():
        sys.exit("probe_accum: no GPU (nothing here is measured on a CPU)")
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"tools/probe_accum.py --rounds {a.rounds}: ms by the contexts' events (library launches) and torch "
        f"events (the caller's blend, the copy), one process, variants alternating per frame")
    say(f"librm: {os.path.relpath(rm.LIBRM_PATH, ROOT)}")
    off = {f: rm.sweep_uniforms(f, 120, BOUNCES, False, rm.RM_SHADOW_SOFT) for f in FRAMES + [60]}
    pats = {"jitter1": rm.custom_pattern([0.3125], [-0.21875]), "GRID2": rm.sample_pattern(rm.RM_PATTERN_GRID2),
            "GRID4": rm.sample_pattern(rm.RM_PATTERN_GRID4)}
    dev = torch.device("cuda", 0)
    stream = torch.cuda.Stream(device=dev)
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8) as r, rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA32F) as r32:
        say(f"cfg 3's shape: {W}x{H}, {BOUNCES} bounces, soft shadows, {len(FRAMES)} sweep frames, {a.rounds} rounds")
        for k, p in pats.items():
            r.dispatch_pattern(off[60], p)
            want = r.read_rgba8()
            r.dispatch_accumulate(off[60], p)  # an earlier sum
            r.dispatch_accumulate(off[60], p, restart=True)
            same = r.read_rgba8().tobytes() == want.tobytes()
            say(f"check  frame 60, {k}: rm_dispatch_accumulate after a restart == the rm_dispatch_pattern image, "
                f"byte for byte: {same}")
            if not same:
                sys.exit("probe_accum: the values differ")
        # the caller's side of (c), and (d)'s buffers
        img = torch.rand((H, W, 4), dtype=torch.float32, device=dev)
        total = torch.zeros_like(img)
        out = torch.empty_like(img)
        dst = torch.empty_like(img)
        count = [0]
        r32.set_stream(stream.cuda_stream)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

        def torch_ms(fn):
            with torch.cuda.stream(stream):
                e0.record(stream)
                fn()
                e1.record(stream)
            e1.synchronize()
            return e0.elapsed_time(e1)

        def blend(n):
            count[0] += n
            total.add_(img)
            torch.div(total, float(count[0]), out=out)

        for x in (r, r32):
            x.enable_timing(True)
            x.kernel_time_ms(reset=True)
        variants = {}
        for k, p in pats.items():
            variants[f"{k} pattern"] = lambda f, p=p: timed(r, lambda: r.dispatch_pattern(off[f], p))
            variants[f"{k} pattern'"] = lambda f, p=p: timed(r, lambda: r.dispatch_pattern(off[f], p))
            variants[f"{k} accum"] = lambda f, p=p: timed(r, lambda: r.dispatch_accumulate(off[f], p))
            variants[f"{k} restart"] = lambda f, p=p: timed(r, lambda: r.dispatch_accumulate(off[f], p, restart=True))
            variants[f"{k} caller"] = lambda f, p=p: (timed(r32, lambda: r32.dispatch_pattern(off[f], p))
                                                      + torch_ms(lambda: blend(int(p.n))))
        variants["copy 32 B/px"] = lambda f: torch_ms(lambda: dst.copy_(img))
        ms = {k: {f: [] for f in FRAMES} for k in variants}
        try:
            for rnd in range(a.rounds + 1):  # round 0 warms every variant up on every frame
                for f in FRAMES:
                    for k, fn in variants.items():  # alternating: drift hits every variant alike
                        t = fn(f)
                        if rnd:
                            ms[k][f].append(t)
        finally:
            r32.synchronize()
            r32.set_stream(None)
        say(f"samples in the sum at the end: {r.accum_samples()} (every 'accum' launch continued a sum, the one the "
            f"restart before it left, and read it)")
    med = {k: [statistics.median(ms[k][f]) for f in FRAMES] for k in variants}
    mean = {k: statistics.fmean(v) for k, v in med.items()}
    per_round = {k: [statistics.fmean(ms[k][f][i] for f in FRAMES) for i in range(a.rounds)] for k in variants}
    say(f"{'variant':<18} {'ms per frame: sweep mean [min, max over the frames]':<52} rounds' sweep means")
    for k in variants:
        say(f"{k:<18} " + f"{mean[k]:.4f} [{min(med[k]):.4f}, {max(med[k]):.4f}]".ljust(52) + " " +
            " ".join(f"{x:.4f}" for x in per_round[k]))
    copy = mean["copy 32 B/px"]
    say(f"(d) the copy: {copy:.4f} ms, {W * H * 32 / copy / 1e6:.0f} GB/s")
    for k in pats:
        base, twin = f"{k} pattern", f"{k} pattern'"
        aa = [x - y for x, y in zip(per_round[twin], per_round[base])]
        bar = 2 * max(abs(x) for x in aa)
        for b in (f"{k} accum", f"{k} restart"):
            d = [x - y for x, y in zip(per_round[b], per_round[base])]
            worst = max(abs(x) for x in d)
            extra = mean[b] - mean[base]
            say(f"(b) - (a), {b}: rounds {' '.join(f'{x:+.4f}' for x in d)} ms; A/A {' '.join(f'{x:+.4f}' for x in aa)} "
                f"ms; largest |difference| {worst:.4f} against the bar 2 x {bar / 2:.4f} = {bar:.4f}: "
                f"{'within' if worst <= bar else 'BEYOND'}; sweep means differ by {extra:+.4f} ms, "
                f"{'within' if extra <= copy else 'beyond'} what the copy's {copy:.4f} ms explains")
        slowest_b = max(per_round[f"{k} accum"])
        fastest_c = min(per_round[f"{k} caller"])
        say(f"claim, {k}: slowest round of (b) {slowest_b:.4f} ms {'<' if slowest_b < fastest_c else '>='} fastest "
            f"round of (c) {fastest_c:.4f} ms: {'holds' if slowest_b < fastest_c else 'DOES NOT HOLD'}; "
            f"(c) - (b) = {mean[f'{k} caller'] - mean[f'{k} accum']:+.4f} ms per frame")
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
