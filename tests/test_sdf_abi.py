"""SDF field queries (rm_sdf_points, rm_sdf_points_device, rm_sdf_grid,
rm_sdf_grid_device): the header declares them, the library exports them and rmarch
binds them; rm_sdf_grid_desc is the 36 bytes the C compiler lays out; the entry
points refuse a null context.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_sdf_points", "rm_sdf_points_device", "rm_sdf_grid", "rm_sdf_grid_device")


def test_header_declares_the_calls_and_constants(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(rm_ctx \*" % name, src, re.M), name
    defs = dict(re.findall(r"^#define (RM_(?:SDF_\w+|HAS_SDF_QUERY|TRACE_NORMAL|API_VERSION))\s+(\d+)", src, re.M))
    assert defs["RM_HAS_SDF_QUERY"] == "1" == str(rm.RM_HAS_SDF_QUERY)
    assert defs["RM_SDF_VALUE"] == "0" == str(rm.RM_SDF_VALUE)
    assert defs["RM_SDF_NORMAL"] == "2" == str(rm.RM_SDF_NORMAL) == defs["RM_TRACE_NORMAL"]
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6


def test_grid_desc_layout_matches_the_c_compiler(rm, tmp_path):
    py = rm.rm_sdf_grid_desc
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rm_api.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rm_sdf_grid_desc));']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rm_sdf_grid_desc, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: int(l.split()[1]) for l in out if l}
    assert got["size"] == 36 == C.sizeof(py)
    assert [f for f, _ in py._fields_] == ["origin", "step", "dims"]
    for f, _ in py._fields_:
        assert got[f] == getattr(py, f).offset, f


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for m in ("sdf", "sdf_grid"):
        assert hasattr(rm.Renderer, m), m


def test_null_context_is_refused(rm):
    lib = rm.lib()
    pts = np.zeros((4, 3), np.float32)
    out = np.zeros(4, rm.RAY_HIT_DTYPE)
    g = rm.rm_sdf_grid_desc((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(2, 2, 1))
    dist, ids = np.zeros(4, np.float32), np.zeros(4, np.int32)
    assert lib.rm_sdf_points(None, pts.ctypes.data, 4, 0, out.ctypes.data) == rm.RM_ERR_INVALID
    assert lib.rm_sdf_points_device(None, pts.ctypes.data, 4, 0, out.ctypes.data) == rm.RM_ERR_INVALID
    assert lib.rm_sdf_grid(None, C.byref(g), dist.ctypes.data, ids.ctypes.data) == rm.RM_ERR_INVALID
    assert lib.rm_sdf_grid_device(None, C.byref(g), dist.ctypes.data, ids.ctypes.data) == rm.RM_ERR_INVALID
    assert not out.tobytes().strip(b"\0") and not dist.any() and not ids.any(), "nothing written"
