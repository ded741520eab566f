"""Geometry-edge adaptive supersampling (RM_HAS_ADAPTIVE_EDGES; rm_aa_criteria,
rm_aa_criteria_init, rm_dispatch_adaptive_edges): the C-ABI additions load and are bound,
the header's and Python's constants and struct agree, rm_aa_criteria_init gives the
documented defaults, and a null context or null criteria is refused with nothing written.
No GPU needed."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("rm_aa_criteria_init", "rm_dispatch_adaptive_edges")
EDGES = {"COLOR": 1, "ID": 2, "DEPTH": 4, "NORMAL": 8, "ALBEDO": 16}


def test_symbols_exported_and_bound(rm):
    lib = rm.lib()
    for name in SYMBOLS:
        assert hasattr(lib, name), name
        assert name in rm.EXPORTED_SYMBOLS
        assert getattr(lib, name).argtypes is not None and getattr(lib, name).restype is C.c_int
    assert hasattr(rm.Renderer, "dispatch_adaptive_edges")


def test_header_and_python_constants_agree(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    defs = dict(re.findall(r"^#define (RM_(?:HAS_ADAPTIVE_EDGES|API_VERSION|AA_EDGE_\w+))\s+(\d+)u?\b", src, re.M))
    assert defs["RM_HAS_ADAPTIVE_EDGES"] == "1" == str(rm.RM_HAS_ADAPTIVE_EDGES)
    assert defs["RM_API_VERSION"] == "6" and rm.RM_API_VERSION == 6  # a feature macro, no version bump
    for name, bit in EDGES.items():
        assert int(defs[f"RM_AA_EDGE_{name}"]) == bit == getattr(rm, f"RM_AA_EDGE_{name}"), name
    assert len([d for d in defs if d.startswith("RM_AA_EDGE_")]) == len(EDGES)
    assert re.search(r"^int rm_aa_criteria_init\(rm_aa_criteria \*c\);", src, re.M)
    assert re.search(r"^int rm_dispatch_adaptive_edges\(rm_ctx \*ctx, const rm_aa_criteria \*criteria\);", src, re.M)
    mirror = open(os.path.join(ROOT, "include", "rm", "texture.hpp")).read()
    assert "rm_dispatch_adaptive_edges(p, " in mirror


def test_struct_matches_the_header(rm):
    src = open(os.path.join(ROOT, "include", "rm_api.h")).read()
    body = re.search(r"typedef struct rm_aa_criteria \{(.*?)\} rm_aa_criteria;", src, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = re.findall(r"(uint32_t|int32_t|float)\s+(\w+);", body)
    ctype = {"uint32_t": C.c_uint32, "int32_t": C.c_int32, "float": C.c_float}
    assert [(n, ctype[t]) for t, n in fields] == list(rm.rm_aa_criteria._fields_)
    assert C.sizeof(rm.rm_aa_criteria) == 20


def test_criteria_init_gives_the_defaults(rm):
    cr = rm.rm_aa_criteria(1, 2, 3, 4.0, 5.0)
    assert rm.lib().rm_aa_criteria_init(C.byref(cr)) == rm.RM_OK
    assert cr.struct_size == 20
    assert cr.edges == rm.RM_AA_EDGE_ID | rm.RM_AA_EDGE_DEPTH | rm.RM_AA_EDGE_NORMAL
    assert cr.color_threshold == 8
    assert cr.depth_rel == C.c_float(0.05).value and cr.normal_cos == C.c_float(0.9).value
    assert rm.lib().rm_aa_criteria_init(None) == rm.RM_ERR_INVALID


def test_null_context_and_null_criteria_are_refused(rm):
    lib = rm.lib()
    cr = rm.rm_aa_criteria()
    lib.rm_aa_criteria_init(C.byref(cr))
    before = bytes(cr)
    assert lib.rm_dispatch_adaptive_edges(None, C.byref(cr)) == rm.RM_ERR_INVALID
    assert lib.rm_dispatch_adaptive_edges(None, None) == rm.RM_ERR_INVALID
    assert bytes(cr) == before, "nothing written"
