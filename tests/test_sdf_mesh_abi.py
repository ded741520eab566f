"""SDF mesh extraction (rm_sdf_mesh, rm_sdf_mesh_device): the header declares the
calls and the constants, the library exports them and rmarch binds them;
rm_sdf_mesh_counts is the 16 bytes the C compiler lays out; the entry points refuse
a null context and write nothing.  No GPU needed."""
import ctypes as C
import os
import re
import subprocess

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_sdf_mesh", "rm_sdf_mesh_device")


def test_header_declares_the_calls_and_constants(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    for name in SYMBOLS:
        assert re.search(r"^int %s\(rm_ctx \*ctx, const rm_sdf_grid_desc \*grid, uint32_t flags," % name, src, re.M), name
    defs = dict(re.findall(r"^#define (RM_(?:MESH_\w+|HAS_SDF_MESH|SDF_NORMAL|API_VERSION))\s+(\d+)u?\b", src, re.M))
    assert defs["RM_HAS_SDF_MESH"] == "1" == str(rm.RM_HAS_SDF_MESH)
    assert defs["RM_MESH_QUADS"] == "0" == str(rm.RM_MESH_QUADS)
    assert defs["RM_MESH_TRIANGLES"] == "1" == str(rm.RM_MESH_TRIANGLES)
    assert defs["RM_MESH_NORMAL"] == "2" == str(rm.RM_MESH_NORMAL) == defs["RM_SDF_NORMAL"]
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6  # unchanged: a new entry point


def test_counts_layout_matches_the_c_compiler(rm, tmp_path):
    py = rm.rm_sdf_mesh_counts
    lines = ['#include <stdio.h>', '#include <stddef.h>', '#include "rm_api.h"', "int main(void) {",
             'printf("size %zu\\n", sizeof(rm_sdf_mesh_counts));',
             'printf("flags %u %u %u\\n", RM_MESH_QUADS, RM_MESH_TRIANGLES, RM_MESH_NORMAL);']
    for f, _ in py._fields_:
        lines.append(f'printf("{f} %zu\\n", offsetof(rm_sdf_mesh_counts, {f}));')
    lines.append("return 0; }")
    src = tmp_path / "layout.c"
    src.write_text("\n".join(lines))
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), "-o", str(exe), str(src)], check=True)
    out = subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n")
    got = {l.split()[0]: [int(v) for v in l.split()[1:]] for l in out if l}
    assert got["size"] == [16] and C.sizeof(py) == 16
    assert got["flags"] == [0, 1, 2]
    assert [f for f, _ in py._fields_] == ["vertices", "quads"]
    for f, _ in py._fields_:
        assert got[f] == [getattr(py, f).offset], f


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert len(getattr(lib, name).argtypes) == 9 and getattr(lib, name).restype is C.c_int
    assert hasattr(rm.Renderer, "sdf_mesh")


def test_null_context_is_refused(rm):
    lib = rm.lib()
    g = rm.rm_sdf_grid_desc((C.c_float * 3)(0, 0, 0), (C.c_float * 3)(1, 1, 1), (C.c_int32 * 3)(3, 3, 3))
    pos = np.zeros((8, 3), np.float32)
    attr = np.zeros(8, rm.RAY_HIT_DTYPE)
    idx = np.zeros((8, 6), np.uint32)
    n = rm.rm_sdf_mesh_counts(77, 78)
    rc = lib.rm_sdf_mesh(None, C.byref(g), 0, pos.ctypes.data, attr.ctypes.data, 8, idx.ctypes.data, 8, C.byref(n))
    assert rc == rm.RM_ERR_INVALID
    cnt = np.full(2, 77, np.uint64)
    rc = lib.rm_sdf_mesh_device(None, C.byref(g), 0, pos.ctypes.data, attr.ctypes.data, 8, idx.ctypes.data, 8,
                                cnt.ctypes.data)
    assert rc == rm.RM_ERR_INVALID
    assert not pos.any() and not idx.any() and not attr.tobytes().strip(b"\0"), "nothing written"
    assert (n.vertices, n.quads) == (77, 78) and (cnt == 77).all()
