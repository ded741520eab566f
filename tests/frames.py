"""Frames on the GPU (a helper, not a test): contexts and renders, the parity bar against
the oracle, the bit-for-bit frame comparisons, and the one cache of the reference frames
the adaptive and pattern tests share.  Importable without a device: everything that
touches one happens inside the functions, on the rmarch module `rm` the tests hand in.
`compare` is the bar of DESIGN.md §5, as tests/test_gpu_parity.py states it."""
from operator import itemgetter

import numpy as np

from scenes import scene_of
from uniforms import main_u, with_aa

BOTH, ALL = 3, 7       # RM_OUT_RGBA8 | RM_OUT_RGBA32F, | RM_OUT_GBUFFER
RGBA8_TOL = 1          # LSB, asserted (north_star: +-2)
RGBA32F_TOL = 2.0e-6   # absolute, colours are O(1): ~16 ULP at 1.0


def images(r):
    return r.read_rgba8(), r.read_rgba32f()


def renderer(rm, W, H, scene=None, outputs=BOTH, specialize=False, **kw):
    r = rm.Renderer(W, H, outputs=outputs, **kw)
    if specialize:
        r.specialize_scene(True)
    if scene is not None:
        r.set_scene(scene)
    return r


def render(rm, u, W, H, scene=None, counters=True, outputs=BOTH, specialize=False, **kw):
    """One frame of u: its two colour images and, from a counting context, the frame
    counters and the per-pixel sdf counts."""
    with renderer(rm, W, H, scene, outputs, specialize, counters=counters, **kw) as r:
        r.dispatch(u)
        out = {"rgba8": r.read_rgba8(), "rgba32f": r.read_rgba32f()}
        if counters:
            out["counters"] = r.counters()
            out["sdf_counts"] = r.sdf_counts()
    return out


def compare(ref, got, label):
    np.testing.assert_array_equal(got["sdf_counts"], ref["sdf_counts"],
                                  err_msg=f"{label}: per-pixel sdf counts differ (geometry)")
    assert got["counters"] == ref["counters"], f"{label}: counters differ: {got['counters']} vs {ref['counters']}"
    d8 = np.abs(got["rgba8"].astype(np.int16) - ref["rgba8"].astype(np.int16))
    assert d8.max() <= RGBA8_TOL, f"{label}: RGBA8 max|d|={d8.max()} ({(d8 > 0).sum()} px)"
    # the reference itself yields NaN for some uniforms (camera inside a
    # primitive); NaN must appear exactly where the oracle has it
    fin = np.isfinite(ref["rgba32f"])
    np.testing.assert_array_equal(np.isfinite(got["rgba32f"]), fin, err_msg=f"{label}: NaN/inf mask")
    df = np.abs(got["rgba32f"] - ref["rgba32f"])[fin]
    assert df.size == 0 or df.max() <= RGBA32F_TOL, f"{label}: RGBA32F max|d|={df.max()}"
    return int(d8.max()), float(df.max()) if df.size else 0.0


def production_equals_counting(rm, u, W, H, k, counted, label):
    """The production build (no counters) takes the proof-based early exits
    that the counting build only checks; both must give the same image."""
    prod = render(rm, u, W, H, kernel=k, counters=False)
    np.testing.assert_array_equal(prod["rgba32f"], counted["rgba32f"], err_msg=label)
    np.testing.assert_array_equal(prod["rgba8"], counted["rgba8"], err_msg=label)


def same(a, b):
    """Two renders equal: images, and counters and sdf counts where a has them."""
    np.testing.assert_array_equal(a["rgba32f"], b["rgba32f"])
    np.testing.assert_array_equal(a["rgba8"], b["rgba8"])
    if "counters" in a:
        assert a["counters"] == b["counters"], f"counters differ: {a['counters']} vs {b['counters']}"
        np.testing.assert_array_equal(a["sdf_counts"], b["sdf_counts"])


def same_frame(got, want, what):
    """(rgba8, rgba32f) pairs: byte for byte, and bit for bit as uint32."""
    assert got[0].tobytes() == want[0].tobytes(), f"{what}: rgba8, {int((got[0] != want[0]).any(-1).sum())} pixels differ"
    np.testing.assert_array_equal(got[1].view(np.uint32), want[1].view(np.uint32), err_msg=f"{what}: rgba32f")


# ---- the reference frames, rendered once ---------------------------------------------------
_refs = {}


def _frozen(arrays):
    for x in arrays:
        x.setflags(write=False)
    return arrays


def refs(rm, W, H, bounces=1, shadow=0, name="builtin", u=None, pattern=None):
    """The references of a frame on the scene `name` (tests/scenes.py scene_of), from other
    calls of the same library, each image pair (rgba8, rgba32f), every array read-only:

      A, B     rm_dispatch with AA off and with AA on, on a plain context with both colour outputs;
      G, G_aa  rm_dispatch's G-buffer with AA off and on, on a G-buffer context;
      P[pname] rm_dispatch_pattern(p) on a plain context, for pattern=(pname, p), added on demand.

    The frame is main_u(rm, bounces, shadow), rendered once per (name, W, H, bounces, shadow)
    and kept; with uniforms u of the caller's own nothing is kept."""
    key = (name, W, H, bounces, shadow)
    ref = _refs.get(key) if u is None else None
    if ref is None:
        ref = {"u": main_u(rm, bounces, shadow) if u is None else with_aa(u, False), "scene": scene_of(rm, name),
               "P": {}}
        with renderer(rm, W, H, ref["scene"]) as r:
            r.dispatch(ref["u"])
            ref["A"] = _frozen(images(r))
            r.dispatch(with_aa(ref["u"], True))
            ref["B"] = _frozen(images(r))
        with renderer(rm, W, H, ref["scene"], outputs=ALL) as r:
            r.dispatch(ref["u"])
            ref["G"], = _frozen((r.read_gbuffer(),))
            r.dispatch(with_aa(ref["u"], True))
            ref["G_aa"], = _frozen((r.read_gbuffer(),))
        if u is None:
            _refs[key] = ref
    if pattern is not None and pattern[0] not in ref["P"]:
        with renderer(rm, W, H, ref["scene"]) as r:
            r.dispatch_pattern(ref["u"], pattern[1])
            ref["P"][pattern[0]] = _frozen(images(r))
    return ref


ab = itemgetter("A", "B")  # A, B = ab(refs(...))


def pattern_frame(rm, W, H, p, pname, bounces=1, shadow=0, name="builtin"):
    """P = (rgba8, rgba32f): rm_dispatch_pattern(p) of refs' frame, once per key and pname."""
    return refs(rm, W, H, bounces, shadow, name, pattern=(pname, p))["P"][pname]
