"""Pattern refinement in the adaptive calls (RM_HAS_ADAPTIVE_PATTERN;
rm_dispatch_adaptive_pattern, rm_dispatch_refine_pattern, rm_dispatch_refine_pattern_device):
the C-ABI additions are in the built library and the header and are bound, a null context is
refused with nothing written, and the rmarch methods exist.  No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_dispatch_adaptive_pattern", "rm_dispatch_refine_pattern", "rm_dispatch_refine_pattern_device")


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int


def test_header_declares_the_feature(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    defs = dict(re.findall(r"^#define (RM_(?:HAS_ADAPTIVE_PATTERN|API_VERSION))\s+(\d+)u?\b", src, re.M))
    assert defs["RM_HAS_ADAPTIVE_PATTERN"] == "1" == str(rm.RM_HAS_ADAPTIVE_PATTERN)
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6  # a feature macro, no version bump
    flat = re.sub(r"\s+", " ", src)
    for decl in ("int rm_dispatch_adaptive_pattern(rm_ctx *ctx, const rm_aa_criteria *criteria, "
                 "const rm_sample_pattern *pattern);",
                 "int rm_dispatch_refine_pattern(rm_ctx *ctx, const uint8_t *mask, size_t row_pitch, "
                 "const rm_sample_pattern *pattern);",
                 "int rm_dispatch_refine_pattern_device(rm_ctx *ctx, const void *mask_dev, size_t row_pitch, "
                 "const rm_sample_pattern *pattern);"):
        assert decl in flat, decl
    # the section follows the sample patterns', and says what it leaves out
    assert src.index("#define RM_HAS_SAMPLE_PATTERN") < src.index("#define RM_HAS_ADAPTIVE_PATTERN")
    section = flat[flat.index("pattern refinement: the adaptive calls"):flat.index("#define RM_HAS_ADAPTIVE_PATTERN")]
    for word in ("batches", "graph replay", "shards", "hiprtc-specialised", "accumulation across calls"):
        assert word in section, word
    mirror = open(os.path.join(ROOT, "include", "rm", "texture.hpp")).read()
    assert "rm_dispatch_adaptive_pattern(p, " in mirror


def test_null_context_is_refused_and_nothing_written(rm):
    lib = rm.lib()
    cr = rm.rm_aa_criteria()
    lib.rm_aa_criteria_init(C.byref(cr))
    p = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    mask = (C.c_uint8 * 16)(*([1] * 16))
    before = bytes(cr), bytes(p), bytes(mask)
    assert lib.rm_dispatch_adaptive_pattern(None, C.byref(cr), C.byref(p)) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_adaptive_pattern(None, None, None) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_refine_pattern(None, mask, 4, C.byref(p)) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_refine_pattern(None, None, 0, None) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_refine_pattern_device(None, C.addressof(mask), 4, C.byref(p)) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_refine_pattern_device(None, None, 0, None) == rm.RM_ERR_INVALID
    assert (bytes(cr), bytes(p), bytes(mask)) == before, "nothing written"


def test_rmarch_methods_exist(rm):
    import inspect
    a = inspect.signature(rm.Renderer.dispatch_adaptive_pattern)
    assert list(a.parameters) == ["self", "u", "criteria", "pattern"]
    r = inspect.signature(rm.Renderer.dispatch_refine_pattern)
    assert list(r.parameters) == ["self", "mask", "pattern", "u", "row_pitch"]


# ---- the frames and criteria of tests/test_gpu_adaptive_pattern.py flag a proper subset -----------
def _oracle_gbuffer(rm, oracle, W, H, scene):
    """The AA-off G-buffer by the oracle's per-ray entry point: the records the frame kernels
    write bit for bit (tests/test_gpu_gbuffer.py)."""
    import numpy as np
    u = rm.sweep_uniforms(60, 120, 1, False, 0)
    o, d = np.empty((H, W, 3), np.float32), np.empty((H, W, 3), np.float32)
    for py in range(H):
        for px in range(W):
            uvx, uvy = np.float32(px * 2 - W) / np.float32(W), np.float32(py * 2 - H) / np.float32(H)
            o[py, px], d[py, px] = oracle.cast_ray(u, float(uvx), float(uvy))
    hits = oracle.trace_rays(u, o.reshape(-1, 3), d.reshape(-1, 3), rm.RM_TRACE_HIT | rm.RM_TRACE_NORMAL, scene)
    return hits.reshape(H, W)


def test_the_gpu_tests_edges_cases_are_not_vacuous(rm, oracle):
    """0 < flagged < W H for every shape, scene and criteria set the GPU file uses: ID | DEPTH |
    NORMAL on the oracle's G-buffer (independent of bounces and shadow mode), and COLOR at
    threshold 8, bracketed through the oracle's image: the GPU's RGBA8 is within 1 of it, so a
    difference above 8 there is above 6 here, and one above 10 here is above 8 there."""
    import numpy as np
    from adaptive_edges_model import COLOR, DEPTH, ID, NORMAL, edge_mask
    from adaptive_model import flag_mask
    from scenes import random_scene
    for W, H in [(130, 67), (37, 23), (9, 5), (8, 8)]:
        g = _oracle_gbuffer(rm, oracle, W, H, None)
        n = int(edge_mask(g, None, ID | DEPTH | NORMAL).sum())
        assert 0 < n < W * H, (W, H, n)
    for scene in (rm.default_scene(), random_scene(rm, 0)):
        g = _oracle_gbuffer(rm, oracle, 37, 23, scene)
        n = int(edge_mask(g, None, ID | DEPTH | NORMAL).sum())
        assert 0 < n < 37 * 23, n
    # (COLOR at 9 x 5 flags all 45 pixels: the GPU file uses the geometric criteria alone there)
    for (W, H), bounces in [((130, 67), 2), ((37, 23), 2), ((37, 23), 1)]:
        img = oracle.render(rm.sweep_uniforms(60, 120, bounces, False, 0), W, H)["rgba8"]
        lo, hi = int(flag_mask(img, 10).sum()), int(flag_mask(img, 6).sum())
        assert 0 < lo <= hi < W * H, (W, H, bounces, lo, hi)
        both = edge_mask(_oracle_gbuffer(rm, oracle, W, H, None), None, ID | DEPTH | NORMAL) | flag_mask(img, 6)
        assert int(both.astype(bool).sum()) < W * H, (W, H, bounces)  # and their union
