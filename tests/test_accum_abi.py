"""Progressive accumulation without a GPU (include/rm_api.h RM_HAS_ACCUMULATION):
the symbols and constants, the refusal of nulls with nothing written, rm_sample_pattern_halton
against the model's Python floats bit for bit (tests/accum_model.py) and its validation, and
the C++ mirror."""
import ctypes as C
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import accum_model as AM

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "rm_api.h")
SYMBOLS = ("rm_dispatch_accumulate", "rm_accum_reset", "rm_accum_samples", "rm_read_accum", "rm_get_accum",
           "rm_sample_pattern_halton")
# first: 0..4095 in steps, around 2^31, the last valid ones
FIRSTS = list(range(0, 4096, 61)) + [4095, 2**31 - 17, 2**31 - 1, 2**31, 2**31 + 5, 2**40 - 16, 2**40]


def fields(p):
    return int(p.struct_size), int(p.flags), int(p.n), list(p.dx), list(p.dy)


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for m in ("dispatch_accumulate", "accumulate", "accum_reset", "accum_samples", "read_accum", "accum_ptr"):
        assert hasattr(rm.Renderer, m), m
    assert list(inspect.signature(rm.Renderer.dispatch_accumulate).parameters) == ["self", "u", "pattern", "restart"]
    assert list(inspect.signature(rm.Renderer.accumulate).parameters) == ["self", "u", "samples", "first"]
    assert list(inspect.signature(rm.halton_pattern).parameters) == ["first", "n"]


def test_header_declares_the_feature_and_constants_match_python(rm):
    src = open(HEADER).read()
    defs = dict(re.findall(r"^#define (RM_(?:HAS_ACCUMULATION|ACCUM_\w+|API_VERSION))\s+(\d+)u?\b", src, re.M))
    assert set(defs) == {"RM_HAS_ACCUMULATION", "RM_ACCUM_RESTART", "RM_API_VERSION"}
    assert defs["RM_HAS_ACCUMULATION"] == "1" == str(rm.RM_HAS_ACCUMULATION)
    assert int(defs["RM_ACCUM_RESTART"]) == rm.RM_ACCUM_RESTART == AM.RESTART == 1
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6  # a feature macro, no version bump
    flat = re.sub(r"\s+", " ", src)
    for decl in ("int rm_dispatch_accumulate(rm_ctx *ctx, const rm_sample_pattern *pattern, uint32_t flags);",
                 "int rm_accum_reset(rm_ctx *ctx);",
                 "int rm_accum_samples(const rm_ctx *ctx, int64_t *samples);",
                 "int rm_read_accum(rm_ctx *ctx, float *dst, size_t row_pitch, int flip_y);",
                 "int rm_get_accum(rm_ctx *ctx, void **device_ptr);",
                 "int rm_sample_pattern_halton(rm_sample_pattern *p, int64_t first, int32_t n);"):
        assert decl in flat, decl
    # the section follows the two it extends, and the sample patterns no longer disclaim the sum
    assert src.index("#define RM_HAS_ADAPTIVE_PATTERN") < src.index("#define RM_HAS_ACCUMULATION")
    patterns = flat[flat.index("sample patterns: a frame supersampled"):flat.index("#define RM_HAS_SAMPLE_PATTERN")]
    assert "accumulation across calls" not in patterns


def test_nulls_are_refused_and_nothing_is_written(rm):
    L = rm.lib()
    p = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    before = fields(p)
    n = C.c_int64(-77)
    ptr = C.c_void_p(0x1234)
    dst = np.full(16, 7.0, np.float32)
    assert L.rm_dispatch_accumulate(None, C.byref(p), 0) == rm.RM_ERR_INVALID
    assert L.rm_dispatch_accumulate(None, C.byref(p), rm.RM_ACCUM_RESTART) == rm.RM_ERR_INVALID
    assert L.rm_dispatch_accumulate(None, None, 0) == rm.RM_ERR_INVALID
    assert L.rm_accum_reset(None) == rm.RM_ERR_INVALID
    assert L.rm_accum_samples(None, C.byref(n)) == rm.RM_ERR_INVALID
    assert L.rm_accum_samples(None, None) == rm.RM_ERR_INVALID
    assert L.rm_read_accum(None, dst.ctypes.data, 0, 0) == rm.RM_ERR_INVALID
    assert L.rm_read_accum(None, None, 0, 0) == rm.RM_ERR_INVALID
    assert L.rm_get_accum(None, C.byref(ptr)) == rm.RM_ERR_INVALID
    assert L.rm_get_accum(None, None) == rm.RM_ERR_INVALID
    assert L.rm_sample_pattern_halton(None, 0, 4) == rm.RM_ERR_INVALID
    assert fields(p) == before and n.value == -77 and ptr.value == 0x1234 and (dst == 7.0).all(), "nothing written"


@pytest.mark.parametrize("n", [1, 4, 7, 16])
def test_halton_equals_the_model_bit_for_bit(rm, n):
    L = rm.lib()
    for first in FIRSTS:
        p = rm.rm_sample_pattern()
        C.memset(C.byref(p), 0xAB, C.sizeof(p))  # every byte is the call's
        assert L.rm_sample_pattern_halton(C.byref(p), first, n) == rm.RM_OK, first
        dx, dy = AM.halton(first, n)
        assert (int(p.struct_size), int(p.flags), int(p.n)) == (C.sizeof(rm.rm_sample_pattern), 0, n)
        got_x, got_y = np.array(list(p.dx), np.float32), np.array(list(p.dy), np.float32)
        assert got_x[:n].tobytes() == dx.tobytes() and got_y[:n].tobytes() == dy.tobytes(), first
        assert not got_x[n:].view(np.uint32).any() and not got_y[n:].view(np.uint32).any(), "entries past n are zero"
        assert bytes(rm.halton_pattern(first, n)) == bytes(p)


def test_halton_is_the_known_sequence(rm):
    """The model itself against the sequence's first terms: 1/2, 1/4, 3/4, 1/8 and 1/3, 2/3, 1/9, 4/9."""
    dx, dy = AM.halton(0, 4)
    assert list(dx) == [0.0, -0.25, 0.25, -0.375]
    want = [np.float32(v - 0.5) for v in (1 / 3, 2 / 3, 1 / 9, 4 / 9)]
    assert np.abs(dy - np.array(want, np.float32)).max() <= 2.0 ** -24  # 1/3 is not a double
    # every point lies in the pixel, and no two calls of consecutive ranges share one
    x, y = AM.halton(0, 16)
    x2, y2 = AM.halton(16, 16)
    assert (np.abs(np.concatenate([x, x2, y, y2])) <= 0.5).all()
    assert len({(float(a), float(b)) for a, b in zip(np.concatenate([x, x2]), np.concatenate([y, y2]))}) == 32
    assert AM.halton(5, 3)[0].tobytes() == x[5:8].tobytes()  # sample s of first is index first + s


def test_halton_validation_leaves_the_struct_untouched(rm):
    L = rm.lib()
    p = rm.sample_pattern(rm.RM_PATTERN_GRID3)
    before = bytes(p)
    for first, n in ((0, 0), (0, -1), (0, 17), (0, 1 << 20), (-1, 4), (2**40 + 1, 4), (2**62, 4), (-2**63, 1)):
        assert L.rm_sample_pattern_halton(C.byref(p), first, n) == rm.RM_ERR_INVALID, (first, n)
        assert bytes(p) == before, (first, n)
    with pytest.raises(rm.RMError):
        rm.halton_pattern(0, 17)


def test_every_halton_pattern_is_a_valid_pattern(rm):
    L = rm.lib()
    for first in FIRSTS:
        for n in (1, 5, 16):
            p = rm.halton_pattern(first, n)
            assert L.rm_pattern_uv_table(C.byref(p), 9, 5, None, None) == rm.RM_OK, (first, n)
    uvx, uvy = rm.pattern_uv_table(rm.halton_pattern(0, 16), 9, 5)
    assert uvx.shape == (9, 16) and uvy.shape == (5, 16) and np.isfinite(uvx).all() and np.isfinite(uvy).all()


def test_cpp_mirror_compiles(tmp_path):
    mirror = open(os.path.join(ROOT, "include", "rm", "texture.hpp")).read()
    assert "rm_dispatch_accumulate(p, &pattern, " in mirror and "inline int dispatchAccumulate(" in mirror
    src = tmp_path / "mirror.cpp"
    src.write_text('#include "rm/texture.hpp"\n'
                   "int both(rm_ctx* c, const rm_sample_pattern& p) {\n"
                   "  return rm::dispatchAccumulate(c, p) + rm::dispatchAccumulate(c, p, true) + "
                   "rm::dispatchAccumulate(c, 64);\n}\n")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                    str(src)], check=True)
