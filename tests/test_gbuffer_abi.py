"""The G-buffer output (RM_OUT_GBUFFER; rm_read_gbuffer, rm_set_output_gbuffer,
rm_get_output_gbuffer): the C-ABI additions load, rm_gbuffer_px is the 32 bytes the C
compiler lays out, the entry points refuse a null context, and a multi-GPU config
with the bit is refused before any device call.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_read_gbuffer", "rm_set_output_gbuffer", "rm_get_output_gbuffer")


def test_gbuffer_px_layout_matches_the_c_compiler(rm, tmp_path):
    """sizeof(rm_gbuffer_px) == 32 and every field offset of the ctypes mirror and of the
    numpy record equals the C compiler's for include/rm_api.h."""
    py = rm.rm_gbuffer_px
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rm_api.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rm_gbuffer_px));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rm_gbuffer_px, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l}
    assert got["size"] == 32 == C.sizeof(py) == rm.GBUFFER_DTYPE.itemsize
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset == rm.GBUFFER_DTYPE.fields[f][1], f
    assert [f for f, _ in py._fields_] == list(rm.GBUFFER_DTYPE.names) == ["t", "id", "normal", "albedo"]
    assert rm.GBUFFER_DTYPE["id"] == np.dtype("<i4")
    # rm_ray_hit's fields of the same names have the same types: comparable field by field
    for f in rm.GBUFFER_DTYPE.names:
        assert rm.GBUFFER_DTYPE[f] == rm.RAY_HIT_DTYPE[f], f


def test_header_constants_match_python(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    defs = dict(re.findall(r"^#define (RM_(?:OUT_\w+|HAS_GBUFFER|API_VERSION))\s+(\d+)", src, re.M))
    assert defs["RM_HAS_GBUFFER"] == "1" and defs["RM_OUT_GBUFFER"] == "4"
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6
    for name in ("RM_OUT_RGBA8", "RM_OUT_RGBA32F", "RM_OUT_GBUFFER", "RM_HAS_GBUFFER"):
        assert int(defs[name]) == getattr(rm, name), name


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for m in ("read_gbuffer", "set_output_gbuffer", "output_gbuffer_ptr"):
        assert hasattr(rm.Renderer, m), m


def test_null_context_is_refused(rm):
    lib = rm.lib()
    px = np.zeros(4, rm.GBUFFER_DTYPE)
    p = C.c_void_p(0x1234)
    assert lib.rm_read_gbuffer(None, px.ctypes.data, 0, 0) == rm.RM_ERR_INVALID
    assert lib.rm_set_output_gbuffer(None, None) == rm.RM_ERR_INVALID
    assert lib.rm_get_output_gbuffer(None, C.byref(p)) == rm.RM_ERR_INVALID
    assert p.value == 0x1234 and not px.tobytes().strip(b"\0"), "nothing written"


def test_multi_gpu_gbuffer_config_is_refused_without_a_device(rm):
    """The ngpus refusal sits with the multi-GPU validation, before any device call: it is
    RM_ERR_INVALID (not RM_ERR_NO_DEVICE) on a box without a GPU, with a message of its own."""
    for outputs in (rm.RM_OUT_GBUFFER, rm.RM_OUT_GBUFFER | rm.RM_OUT_RGBA8,
                    rm.RM_OUT_GBUFFER | rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F):
        for ngpus in (1, 2):
            with pytest.raises(rm.RMError) as e:
                rm.Renderer(64, 64, ngpus=ngpus, outputs=outputs)
            assert e.value.code == rm.RM_ERR_INVALID, (outputs, ngpus)
            assert "RM_OUT_GBUFFER" in str(e.value)
    # an unknown bit beside it is still refused on a one-device config
    with pytest.raises(rm.RMError) as e:
        rm.Renderer(64, 64, outputs=rm.RM_OUT_GBUFFER | 8)
    assert e.value.code == rm.RM_ERR_INVALID
    # the bit with counters: refused before the device is looked for
    with pytest.raises(rm.RMError) as e:
        rm.Renderer(64, 64, outputs=rm.RM_OUT_GBUFFER | rm.RM_OUT_RGBA8, counters=True)
    assert e.value.code == rm.RM_ERR_INVALID and "counters" in str(e.value)
