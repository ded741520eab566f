"""Sample patterns without a GPU (include/rm_api.h RM_HAS_SAMPLE_PATTERN):
the symbols and constants, the presets and rm_pattern_uv_table against the numpy model
(tests/sample_pattern_model.py), the validation, and the rule itself against the oracle:
the REFERENCE pattern's table, cast and rendered ray by ray and summed by the rule, is the
reference's AA pixel."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import sample_pattern_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rm_api.h")
SIZES = [(1, 1), (9, 5), (37, 23), (3840, 2160), (65536, 1)]


def model_pattern(rm, k):
    flags, dx, dy = M.preset(k)
    return rm.custom_pattern(dx, dy, bool(flags & M.CUMULATIVE))


def random_patterns(rm):
    """One absolute n = 7 and one cumulative n = 16 pattern, offsets within 2 pixels."""
    rng = np.random.default_rng(20)
    a = rng.uniform(-2, 2, (2, 7)).astype(np.float32)
    c = rng.uniform(-0.25, 0.25, (2, 16)).astype(np.float32)
    return [("abs7", 0, a[0], a[1]), ("cum16", M.CUMULATIVE, c[0], c[1])]


def fields(p):
    return int(p.struct_size), int(p.flags), int(p.n), list(p.dx), list(p.dy)


def test_symbols_and_constants(rm):
    L = rm.lib()
    for name in ("rm_sample_pattern_init", "rm_pattern_uv_table", "rm_dispatch_pattern"):
        assert hasattr(L, name) and name in rm.EXPORTED_SYMBOLS
    src = open(HEADER).read()
    defs = dict(re.findall(r"^#define (RM_(?:PATTERN_\w+|MAX_SAMPLES|HAS_SAMPLE_PATTERN))\s+(\d+)u?\b", src, re.M))
    assert set(defs) == {"RM_HAS_SAMPLE_PATTERN", "RM_MAX_SAMPLES", "RM_PATTERN_CUMULATIVE", "RM_PATTERN_REFERENCE",
                         "RM_PATTERN_GRID2", "RM_PATTERN_RGSS", "RM_PATTERN_GRID3", "RM_PATTERN_GRID4"}
    for name, v in defs.items():
        assert getattr(rm, name) == int(v), name
    assert (M.MAX_SAMPLES, M.CUMULATIVE) == (rm.RM_MAX_SAMPLES, rm.RM_PATTERN_CUMULATIVE)
    assert (M.REFERENCE, M.GRID2, M.RGSS, M.GRID3, M.GRID4) == (
        rm.RM_PATTERN_REFERENCE, rm.RM_PATTERN_GRID2, rm.RM_PATTERN_RGSS, rm.RM_PATTERN_GRID3, rm.RM_PATTERN_GRID4)
    assert C.sizeof(rm.rm_sample_pattern) == 140


def test_struct_layout_matches_the_c_compiler(rm, tmp_path):
    py = rm.rm_sample_pattern
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rm_api.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rm_sample_pattern));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rm_sample_pattern, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    got = dict(l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                 check=True).stdout.splitlines() if l)
    assert int(got["size"]) == C.sizeof(py) == 140
    for f, _ in py._fields_:
        assert int(got[f]) == getattr(py, f).offset, f


def test_nulls_are_refused_and_nothing_is_written(rm):
    L = rm.lib()
    p = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    assert L.rm_sample_pattern_init(None, rm.RM_PATTERN_GRID2) == rm.RM_ERR_INVALID
    before = fields(p)
    for bad in (-1, 5, 1 << 20):
        assert L.rm_sample_pattern_init(C.byref(p), bad) == rm.RM_ERR_INVALID
        assert fields(p) == before
    assert L.rm_dispatch_pattern(None, C.byref(p)) == rm.RM_ERR_INVALID
    assert L.rm_dispatch_pattern(None, None) == rm.RM_ERR_INVALID
    assert fields(p) == before
    uvx, uvy = np.full((9, 16), 7.0, np.float32), np.full((5, 16), 7.0, np.float32)
    assert L.rm_pattern_uv_table(None, 9, 5, uvx.ctypes.data, uvy.ctypes.data) == rm.RM_ERR_INVALID
    for w, h in ((0, 5), (9, 0), (65537, 5), (9, 65537), (-1, 5)):
        assert L.rm_pattern_uv_table(C.byref(p), w, h, uvx.ctypes.data, uvy.ctypes.data) == rm.RM_ERR_INVALID
    assert (uvx == 7.0).all() and (uvy == 7.0).all()
    # either output may be left out
    assert L.rm_pattern_uv_table(C.byref(p), 9, 5, None, uvy.ctypes.data) == rm.RM_OK
    assert L.rm_pattern_uv_table(C.byref(p), 9, 5, uvx.ctypes.data, None) == rm.RM_OK
    np.testing.assert_array_equal(uvx.view(np.uint32), rm.pattern_uv_table(p, 9, 5)[0].view(np.uint32))


@pytest.mark.parametrize("k", range(5))
def test_presets_equal_the_model(rm, k):
    p = rm.sample_pattern(k)
    flags, dx, dy = M.preset(k)
    n = len(dx)
    pad = [0.0] * (M.MAX_SAMPLES - n)
    assert fields(p) == (140, flags, n, list(dx) + pad, list(dy) + pad)
    # every offset is a dyadic rational with a short mantissa: 2 d and d itself are exact in float32
    for d in dx + dy:
        assert float(np.float32(d)) == d and (d * 32).is_integer()
    # the grids are centred: the offsets sum to zero on both axes
    if k != M.REFERENCE:
        assert sum(dx) == 0 and sum(dy) == 0


@pytest.mark.parametrize("W,H", SIZES)
def test_uv_table_equals_the_model_bit_for_bit(rm, W, H):
    cases = [(f"preset{k}", *M.preset(k)) for k in range(5)] + random_patterns(rm)
    for name, flags, dx, dy in cases:
        p = rm.custom_pattern(dx, dy, bool(flags & M.CUMULATIVE))
        uvx, uvy = rm.pattern_uv_table(p, W, H)
        mx, my = M.uv_table(flags, [float(x) for x in dx], [float(y) for y in dy], W, H)
        assert uvx.shape == (W, len(dx)) and uvy.shape == (H, len(dx))
        np.testing.assert_array_equal(uvx.view(np.uint32), mx.view(np.uint32), err_msg=f"{name} {W}x{H} uvx")
        np.testing.assert_array_equal(uvy.view(np.uint32), my.view(np.uint32), err_msg=f"{name} {W}x{H} uvy")
    # the preset structs give the same tables as their model offsets
    for k in range(5):
        a, b = rm.pattern_uv_table(rm.sample_pattern(k), W, H), rm.pattern_uv_table(model_pattern(rm, k), W, H)
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()


def test_reference_table_is_the_frame_table_and_n1_the_centre(rm):
    """The two anchors on the host: REFERENCE's uv are the AA frame's cumulative offsets
    (x0 + .25 / W, + .75 / W, ...), and (0, 0) alone is x0."""
    W, H = 37, 23
    uvx, uvy = rm.pattern_uv_table(rm.sample_pattern(rm.RM_PATTERN_REFERENCE), W, H)
    f = np.float32
    for uv, dim, offs in ((uvx, W, (.25, .75, .25, .75)), (uvy, H, (.25, .25, .75, .75))):
        v = (2 * np.arange(dim) - dim).astype(f) / f(dim)
        for s, o in enumerate(offs):
            v = v + f(o) / f(dim)
            np.testing.assert_array_equal(uv[:, s].view(np.uint32), v.view(np.uint32))
    cx, cy = rm.pattern_uv_table(rm.custom_pattern([0.0], [0.0]), W, H)
    np.testing.assert_array_equal(cx[:, 0], (2 * np.arange(W) - W).astype(f) / f(W))
    np.testing.assert_array_equal(cy[:, 0], (2 * np.arange(H) - H).astype(f) / f(H))


def _rc(rm, p):
    out = np.empty((9 + 5) * 16, np.float32)
    return rm.lib().rm_pattern_uv_table(C.byref(p), 9, 5, out.ctypes.data, out[9 * 16:].ctypes.data)


def test_validation(rm):
    ok = rm.sample_pattern(rm.RM_PATTERN_GRID3)  # n = 9
    assert _rc(rm, ok) == rm.RM_OK
    for field, bad in (("struct_size", 0), ("struct_size", 136), ("struct_size", 144), ("flags", 2), ("flags", 3),
                       ("flags", 1 << 31), ("n", 0), ("n", -1), ("n", 17), ("n", 1 << 30)):
        p = rm.rm_sample_pattern.from_buffer_copy(ok)
        setattr(p, field, bad)
        assert _rc(rm, p) == rm.RM_ERR_INVALID, (field, bad)
    bad_values = (float("nan"), float("inf"), float("-inf"), 16.000002, -16.000002, 1e30)
    for n in (1, 9, 16):
        for axis in ("dx", "dy"):
            for v in bad_values:
                for at in sorted({0, n // 2, n - 1}):  # every index below n is read
                    p = rm.rm_sample_pattern.from_buffer_copy(ok)
                    p.n = n
                    getattr(p, axis)[at] = v
                    assert _rc(rm, p) == rm.RM_ERR_INVALID, (n, axis, v, at)
                if n < 16:  # entries from n on are not
                    p = rm.rm_sample_pattern.from_buffer_copy(ok)
                    p.n = n
                    for at in range(n, 16):
                        getattr(p, axis)[at] = v
                    assert _rc(rm, p) == rm.RM_OK, (n, axis, v)
    # the bounds themselves are valid
    p = rm.custom_pattern([16.0, -16.0], [-16.0, 16.0])
    assert _rc(rm, p) == rm.RM_OK
    p.flags = rm.RM_PATTERN_CUMULATIVE
    assert _rc(rm, p) == rm.RM_OK


def test_reference_rule_is_the_oracles_aa_pixel(rm, oracle):
    """9 x 5 frame of rm_sweep_uniforms(60, 120, 1, 1, 0): the REFERENCE table through the
    oracle's castRay and render, summed by the rule, equals the oracle's AA pixel value for
    value (only the sign of a zero may differ)."""
    W, H = 9, 5
    u = rm.sweep_uniforms(60, 120, 1, True, 0)
    uvx, uvy = rm.pattern_uv_table(rm.sample_pattern(rm.RM_PATTERN_REFERENCE), W, H)
    for py in range(H):
        for px in range(W):
            cols = [oracle.render_ray(u, *oracle.cast_ray(u, float(uvx[px, s]), float(uvy[py, s]))) for s in range(4)]
            got, want = M.pixel_sum(cols), oracle.pixel(u, W, H, px, py)
            assert got.dtype == want.dtype == np.float32
            assert all(a == b or (np.isnan(a) and np.isnan(b)) for a, b in zip(got, want)), (px, py, got, want)
