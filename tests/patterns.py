"""The sample patterns of the pattern tests and the frame they owe by the header's rule (a
helper, not a test).

"Model" is the rule of include/rm_api.h RM_HAS_SAMPLE_PATTERN with nothing of the frame
kernels in it: the uv from rm_pattern_uv_table (held against numpy by
tests/test_pattern_abi.py), the rays from the oracle's castRay, the colours from the same
context's SHADE trace of those rays, the sum and the quantisation in numpy float32
(tests/sample_pattern_model.py).  RGBA32F is compared as uint32 wherever the expected
value is not NaN and NaN-for-NaN elsewhere, RGBA8 byte for byte."""
import numpy as np

import sample_pattern_model as SPM


def random_patterns(rm):
    rng = np.random.default_rng(21)
    a = rng.uniform(-1.5, 1.5, (2, 7)).astype(np.float32)
    c = rng.uniform(-0.2, 0.2, (2, 16)).astype(np.float32)
    return {"abs7": rm.custom_pattern(a[0], a[1]), "cum16": rm.custom_pattern(c[0], c[1], cumulative=True),
            "jitter1": rm.custom_pattern([0.3125], [-0.21875])}


def patterns(rm):
    """The seven patterns rm_dispatch_pattern's frames are held to the model on."""
    out = {"grid2": rm.sample_pattern(rm.RM_PATTERN_GRID2), "rgss": rm.sample_pattern(rm.RM_PATTERN_RGSS),
           "grid3": rm.sample_pattern(rm.RM_PATTERN_GRID3), "grid4": rm.sample_pattern(rm.RM_PATTERN_GRID4)}
    out.update(random_patterns(rm))
    return out


def refine_patterns(rm):
    """The ten patterns of the pattern refinement: rounds 1 (GRID2, RGSS, REFERENCE, abs2), 2
    (abs7: 4 + 3), 3 (GRID3: 4 + 4 + 1), 4 (GRID4, cum16) and the two one-sample kernels'
    (jitter1, centre)."""
    rng = np.random.default_rng(22)
    a2 = rng.uniform(-1.5, 1.5, (2, 2)).astype(np.float32)
    out = {"grid2": rm.sample_pattern(rm.RM_PATTERN_GRID2), "rgss": rm.sample_pattern(rm.RM_PATTERN_RGSS),
           "grid3": rm.sample_pattern(rm.RM_PATTERN_GRID3), "grid4": rm.sample_pattern(rm.RM_PATTERN_GRID4),
           "reference": rm.sample_pattern(rm.RM_PATTERN_REFERENCE), "abs2": rm.custom_pattern(a2[0], a2[1])}
    out.update(random_patterns(rm))  # abs7, cum16, jitter1
    out["centre"] = rm.custom_pattern([0.0], [0.0])
    return out


def model(rm, oracle, r, u, p):
    """(rgba8, rgba32f) of pattern p's frame of u by the rule, the colours from r's SHADE trace."""
    W, H, n = r.width, r.height, int(p.n)
    uvx, uvy = rm.pattern_uv_table(p, W, H)
    o, d = np.empty((H, W, n, 3), np.float32), np.empty((H, W, n, 3), np.float32)
    for py in range(H):
        for px in range(W):
            for s in range(n):
                o[py, px, s], d[py, px, s] = oracle.cast_ray(u, float(uvx[px, s]), float(uvy[py, s]))
    r.set_uniforms(u)
    col = r.trace(o.reshape(-1, 3), d.reshape(-1, 3), rm.RM_TRACE_SHADE)["color"].reshape(H, W, n, 3)
    f32 = SPM.pixel_sum(np.moveaxis(col, 2, 0))
    return SPM.quantize(f32), f32


def equals_model(got, want, what):
    g8, g32 = got
    w8, w32 = want
    assert g32.shape == w32.shape and g8.shape == w8.shape, \
        f"{what}: shapes {g8.shape}, {g32.shape} against the model's {w8.shape}, {w32.shape}"
    nan = np.isnan(w32)
    assert np.isnan(g32[nan]).all(), f"{what}: NaN for NaN"
    bad = (g32.view(np.uint32) != w32.view(np.uint32)) & ~nan
    assert not bad.any(), f"{what}: rgba32f differs in {int(bad.any(-1).sum())} pixels, first at {np.argwhere(bad)[0]}"
    assert g8.tobytes() == w8.tobytes(), f"{what}: rgba8, {int((g8 != w8).any(-1).sum())} pixels differ"
