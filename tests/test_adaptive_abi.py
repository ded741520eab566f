"""Adaptive supersampling (RM_HAS_ADAPTIVE_AA; rm_dispatch_adaptive, rm_dispatch_refine,
rm_dispatch_refine_device, rm_read_aa_mask, rm_get_aa_mask, rm_aa_refined): the C-ABI
additions load and are bound, the header's and Python's constants agree, and every
entry point refuses a null context without writing anything.  No GPU needed."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_dispatch_adaptive", "rm_dispatch_refine", "rm_dispatch_refine_device", "rm_read_aa_mask",
           "rm_get_aa_mask", "rm_aa_refined")


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    for m in ("dispatch_adaptive", "dispatch_refine", "read_aa_mask", "aa_mask_ptr", "aa_refined"):
        assert hasattr(rm.Renderer, m), m


def test_header_declares_them_and_constants_match_python(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    defs = dict(re.findall(r"^#define (RM_(?:HAS_ADAPTIVE_AA|API_VERSION))\s+(\d+)", src, re.M))
    assert defs["RM_HAS_ADAPTIVE_AA"] == "1" == str(rm.RM_HAS_ADAPTIVE_AA)
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6  # a feature macro, no version bump
    for name in SYMBOLS:
        assert re.search(r"^int %s\(rm_ctx \*ctx, " % name, src, re.M), name
    mirror = open(os.path.join(ROOT, "include", "rm", "texture.hpp")).read()
    assert "rm_dispatch_adaptive(p, threshold)" in mirror


def test_null_context_is_refused(rm):
    lib = rm.lib()
    mask = np.full(16, 7, np.uint8)
    p = C.c_void_p(0x1234)
    n = C.c_int64(-77)
    assert lib.rm_dispatch_adaptive(None, 8) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_refine(None, mask.ctypes.data, 0) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_refine_device(None, 0x1000, 0) == rm.RM_ERR_INVALID
    assert lib.rm_read_aa_mask(None, mask.ctypes.data, 0, 0) == rm.RM_ERR_INVALID
    assert lib.rm_get_aa_mask(None, C.byref(p)) == rm.RM_ERR_INVALID
    assert lib.rm_aa_refined(None, C.byref(n)) == rm.RM_ERR_INVALID
    assert p.value == 0x1234 and n.value == -77 and (mask == 7).all(), "nothing written"
