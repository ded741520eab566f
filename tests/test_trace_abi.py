"""Ray queries (rm_trace_rays, rm_trace_rays_device, rm_pick): the C-ABI additions
load, rm_ray_hit is the 48 bytes the C compiler lays out, and the entry points
refuse a null context.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_trace_rays", "rm_trace_rays_device", "rm_pick")


def test_ray_hit_layout_matches_the_c_compiler(rm, tmp_path):
    """sizeof(rm_ray_hit) == 48 and every field offset of the ctypes mirror and of the
    numpy record equals the C compiler's for include/rm_api.h."""
    py = rm.rm_ray_hit
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rm_api.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rm_ray_hit));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rm_ray_hit, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l}
    assert got["size"] == 48 == C.sizeof(py) == rm.RAY_HIT_DTYPE.itemsize
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset == rm.RAY_HIT_DTYPE.fields[f][1], f
    assert [f for f, _ in py._fields_] == list(rm.RAY_HIT_DTYPE.names)
    assert rm.RAY_HIT_DTYPE["id"] == np.dtype("<i4")


def test_header_constants_match_python(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    defs = dict(re.findall(r"^#define (RM_(?:TRACE_\w+|HAS_TRACE|API_VERSION))\s+(\d+)", src, re.M))
    assert defs["RM_HAS_TRACE"] == "1" and defs["RM_API_VERSION"] == "6"
    for name in ("RM_TRACE_HIT", "RM_TRACE_REFLECTED", "RM_TRACE_NORMAL", "RM_TRACE_SHADE",
                 "RM_TRACE_SHADOW", "RM_HAS_TRACE"):
        assert int(defs[name]) == getattr(rm, name), name
    assert (rm.RM_TRACE_HIT, rm.RM_TRACE_REFLECTED, rm.RM_TRACE_NORMAL, rm.RM_TRACE_SHADE,
            rm.RM_TRACE_SHADOW) == (0, 1, 2, 4, 8)


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert hasattr(rm.Renderer, "trace") and hasattr(rm.Renderer, "pick")


def test_null_context_is_refused(rm):
    lib = rm.lib()
    o = np.zeros((1, 3), np.float32)
    d = np.ones((1, 3), np.float32)
    hits = np.zeros(1, rm.RAY_HIT_DTYPE)
    assert lib.rm_trace_rays(None, o.ctypes.data, d.ctypes.data, 1, 0, hits.ctypes.data) == rm.RM_ERR_INVALID
    assert lib.rm_trace_rays_device(None, o.ctypes.data, d.ctypes.data, 1, 0,
                                    hits.ctypes.data) == rm.RM_ERR_INVALID
    assert lib.rm_pick(None, 0, 0, C.cast(hits.ctypes.data, C.POINTER(rm.rm_ray_hit))) == rm.RM_ERR_INVALID
    assert not hits.tobytes().strip(b"\0"), "nothing written"
