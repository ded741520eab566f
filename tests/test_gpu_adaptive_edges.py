"""Geometry-edge adaptive supersampling on the GPU (rm_dispatch_adaptive_edges).

Throughout, A is rm_dispatch with AA off and B rm_dispatch with AA on, on a plain context
with both colour outputs, and G is the AA-off rm_dispatch G-buffer on a G-buffer context
(tests/frames.py refs).  The definition (tests/adaptive_checks.py check_frame): the mask M is
the flagging rule (tests/adaptive_edges_model.py) applied to G and
A's RGBA8 image, exactly; the image is where(M, B, A), byte for byte in RGBA8 and bit for bit
in RGBA32F; rm_read_gbuffer is G, bit for bit; rm_aa_refined is M.sum().

Frames: rm_sweep_uniforms(60, 120, ., 0, 0) at 130 x 67 (ragged for the 8x8 tiles and for the
four-wave workgroups: 17 tile columns), 37 x 23 (neighbours across tile borders on both axes),
9 x 5 (across them in x only), 8 x 8 (one tile, no foreign neighbour) and 1 x 1.
"""
import ctypes as C

import numpy as np
import pytest

from adaptive_checks import DEFAULTS, check_frame, criteria
from adaptive_edges_model import ALBEDO, BITS, COLOR, COUNTS, DEPTH, ID, NORMAL, edge_mask
from adaptive_model import flag_mask
from frames import ALL, BOTH, refs, renderer
from scenes import scene_of
from uniforms import main_u, off_sweep_uniforms, with_aa

pytestmark = pytest.mark.gpu

W0, H0 = 130, 67
SHAPES = [(130, 67), (37, 23), (9, 5), (8, 8), (1, 1)]
GEOMETRY = ID | DEPTH | NORMAL | ALBEDO
COMBOS = [COLOR, ID, DEPTH, NORMAL, ALBEDO, ID | DEPTH | NORMAL, GEOMETRY | COLOR]


def check_edges(r, u, edges, ref, what, **kw):
    par = dict(DEFAULTS, **kw)
    r.dispatch_adaptive_edges(u, edges, **par)
    with np.errstate(all="ignore"):
        want = edge_mask(ref["G"], ref["A"][0], edges, **par)
    return check_frame(r, want, ref["A"], ref["B"], f"{what} edges {edges}", ref["G"])[0]


# ---- 1. the definition ----------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 2])
@pytest.mark.parametrize("W,H", SHAPES)
def test_edges_equal_definition(rm, gpu, W, H, bounces):
    u = main_u(rm, bounces)
    ref = refs(rm, W, H, bounces)
    with rm.Renderer(W, H, outputs=ALL) as r:
        for edges in COMBOS:
            M = check_edges(r, u, edges, ref, f"{W}x{H} b{bounces}")
            if (W, H) == (1, 1):
                assert not M.any()
            if (W, H) in COUNTS and edges in BITS.values():
                # the G-buffer is bit-exact against the oracle, so these are the oracle's counts
                name = [k for k, b in BITS.items() if b == edges][0]
                assert int(M.sum()) == COUNTS[(W, H)][name], (name, int(M.sum()))
        if (W, H) == (W0, H0):
            M = r.read_aa_mask()  # all five bits
            assert M.any() and not M.all()
            c8 = r.read_rgba8()
            assert (c8 != ref["A"][0]).any() and (c8 != ref["B"][0]).any()
        # u.AA is ignored, and the uniforms stay as they are
        r.dispatch_adaptive_edges(with_aa(u, True), ID | DEPTH | NORMAL)
        assert r.get_uniforms().AA == 1
        check_frame(r, edge_mask(ref["G"], None, ID | DEPTH | NORMAL, **DEFAULTS), ref["A"], ref["B"], "u.AA = 1", ref["G"])


@pytest.mark.parametrize("outputs", [1 | 4, 2 | 4], ids=["rgba8", "rgba32f"])
def test_one_colour_output(rm, gpu, outputs):
    """COLOR reads the RGBA8 image, or quantises the RGBA32F one."""
    u = main_u(rm)
    ref = refs(rm, W0, H0)
    with rm.Renderer(W0, H0, outputs=outputs) as r:
        for edges in (COLOR, GEOMETRY | COLOR):
            check_edges(r, u, edges, ref, f"outputs {outputs}")


@pytest.mark.parametrize("W,H", [(130, 67), (37, 23), (9, 5)])
def test_plain_form_gives_the_same_frame(rm, gpu, monkeypatch, W, H):
    """RM_AA_EDGES_NAIVE: the classifier with four pair tests per lane, kept for measurement."""
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2)
    with rm.Renderer(W, H, outputs=ALL) as r:
        monkeypatch.setenv("RM_AA_EDGES_NAIVE", "1")  # read by every call
        for edges in COMBOS:
            check_edges(r, u, edges, ref, f"{W}x{H} plain form")
        monkeypatch.setenv("RM_AA_EDGES_NAIVE", "0")
        check_edges(r, u, GEOMETRY | COLOR, ref, f"{W}x{H} two-pair form again")


# ---- 2. COLOR alone is rm_dispatch_adaptive ---------------------------------------------------------
@pytest.mark.parametrize("outputs", [BOTH, ALL], ids=["plain", "gbuffer"])
def test_color_alone_is_dispatch_adaptive(rm, gpu, outputs):
    u = main_u(rm)
    ref = refs(rm, W0, H0)
    with rm.Renderer(W0, H0, outputs=BOTH) as p, rm.Renderer(W0, H0, outputs=outputs) as r:
        for thr in (0, 8, 255):
            p.dispatch_adaptive(u, thr)
            r.dispatch_adaptive_edges(u, COLOR, color_threshold=thr, depth_rel=-1.0, normal_cos=7.0)
            np.testing.assert_array_equal(r.read_aa_mask(), p.read_aa_mask())
            assert r.read_rgba8().tobytes() == p.read_rgba8().tobytes()
            assert r.read_rgba32f().tobytes() == p.read_rgba32f().tobytes()
            assert r.aa_refined() == p.aa_refined()
            check_frame(r, flag_mask(ref["A"][0], thr), ref["A"], ref["B"], f"thr {thr}", ref["G"])


# ---- 3. tables ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("specialize", [False, True], ids=["generic", "specialised"])
@pytest.mark.parametrize("which", ["random0", "floor0"])
def test_tables(rm, gpu, which, specialize):
    scene = scene_of(rm, which)
    u = main_u(rm)
    ref = refs(rm, W0, H0, name=which)
    with renderer(rm, W0, H0, scene, ALL, specialize) as r:
        for edges in COMBOS:
            check_edges(r, u, edges, ref, which)


# ---- 4. caller-owned buffers and stream --------------------------------------------------------------
def test_caller_owned_gbuffer(rm, gpu):
    import torch
    W, H = 37, 23
    u, u2 = main_u(rm), rm.sweep_uniforms(20, 120, 1, False, 0)
    ref = refs(rm, W, H)
    edges = ID | DEPTH | NORMAL
    want = edge_mask(ref["G"], None, edges, **DEFAULTS)
    with rm.Renderer(W, H, outputs=ALL) as r:
        dev = torch.device("cuda", r.device)
        s = torch.cuda.Stream(device=dev)
        # the context's own G-buffer holds another frame's records
        r.dispatch(u2)
        stale = r.read_gbuffer()
        assert (edge_mask(stale, None, edges, **DEFAULTS) != want).any()
        try:
            with torch.cuda.stream(s):
                r.set_stream(s.cuda_stream)
                buf = torch.full((H * W * 8 + 8,), -7.25, dtype=torch.float32, device=dev)
                out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
                r.set_output_gbuffer(buf.data_ptr())
                r.set_output_rgba8(out.data_ptr())
                r.dispatch_adaptive_edges(u, edges)
                got8, gotg = out.cpu().numpy(), buf.cpu().numpy()  # ordered after the frame on the stream
            r.synchronize()
            assert gotg[:H * W * 8].tobytes() == ref["G"].tobytes(), "the caller's buffer holds pass 1's records"
            assert (gotg[H * W * 8:] == np.float32(-7.25)).all(), "the sentinel after the last record"
            assert got8.tobytes() == np.where(want.astype(bool)[..., None], ref["B"][0], ref["A"][0]).tobytes()
            check_frame(r, want, ref["A"], ref["B"], "caller-owned", ref["G"])  # the caller's buffer's mask, not the stale one's
        finally:
            r.synchronize()
            r.set_output_gbuffer(None)
            r.set_output_rgba8(None)
            r.set_stream(None)
        assert r.read_gbuffer().tobytes() == stale.tobytes(), "the context's own buffer was left alone"


# ---- 5. uniforms off the sweep -----------------------------------------------------------------------------
@pytest.mark.parametrize("i", [0, 1, 2, 3, 16], ids=[f"case{i}" for i in range(4)] + ["nan_camera"])
def test_off_sweep_uniforms(rm, gpu, i):
    u, (W, H) = off_sweep_uniforms(rm, i)
    assert (W, H) == (67, 41)
    with np.errstate(all="ignore"):
        ref = refs(rm, W, H, u=u)
        with rm.Renderer(W, H, outputs=ALL) as r:
            r.dispatch(with_aa(u, False))
            own = r.read_gbuffer()  # this context's own G
            assert own.tobytes() == ref["G"].tobytes()
            for edges in (ID | DEPTH | NORMAL, GEOMETRY | COLOR):
                check_edges(r, u, edges, dict(ref, G=own), f"case {i}")


# ---- 6. extremes ----------------------------------------------------------------------------------------------
def test_extremes(rm, gpu):
    u = main_u(rm)
    ref = refs(rm, W0, H0)
    with rm.Renderer(W0, H0, outputs=ALL) as r:
        M0 = check_edges(r, u, DEPTH, ref, "depth_rel 0", depth_rel=0.0)
        assert M0.sum() >= COUNTS[(W0, H0)]["DEPTH"]  # a wider net than depth_rel 0.05's
        M = check_edges(r, u, DEPTH, ref, "depth_rel inf", depth_rel=float("inf"))
        assert not M.any() and r.aa_refined() == 0
        assert r.read_rgba8().tobytes() == ref["A"][0].tobytes() and r.read_rgba32f().tobytes() == ref["A"][1].tobytes()
        Mn = check_edges(r, u, NORMAL, ref, "normal_cos -1", normal_cos=-1.0)
        Mp = check_edges(r, u, NORMAL, ref, "normal_cos 1", normal_cos=1.0)
        assert Mp.sum() >= COUNTS[(W0, H0)]["NORMAL"] >= Mn.sum()  # dot < -1 <= dot < 0.9 <= dot < 1


# ---- 7. nothing sticky ------------------------------------------------------------------------------------------
def test_nothing_sticky(rm, gpu):
    u = main_u(rm)
    ref = refs(rm, W0, H0)
    with rm.Renderer(W0, H0, outputs=ALL) as r:
        r.enable_timing(True)
        _, n0 = r.kernel_time_ms()
        check_edges(r, u, ID | DEPTH | NORMAL, ref, "first")
        ms, n1 = r.kernel_time_ms()
        assert n1 - n0 == 1 and ms > 0.0  # one event pair: one launch of one frame
        r.dispatch(with_aa(u, True))  # the plain AA-on frame, as always
        assert r.read_rgba8().tobytes() == ref["B"][0].tobytes()
        assert r.read_rgba32f().tobytes() == ref["B"][1].tobytes()
        assert r.read_gbuffer().tobytes() == ref["G_aa"].tobytes(), "the first sample's G-buffer"
        assert ref["G_aa"].tobytes() != ref["G"].tobytes()
        # the mask and the count stay those of the last adaptive dispatch; the buffers are reused
        np.testing.assert_array_equal(r.read_aa_mask(), edge_mask(ref["G"], None, ID | DEPTH | NORMAL, **DEFAULTS))
        ptr = r.aa_mask_ptr()
        check_edges(r, u, ALBEDO, ref, "again")
        assert r.aa_mask_ptr() == ptr
        r.dispatch(with_aa(u, False))
        assert r.read_rgba8().tobytes() == ref["A"][0].tobytes() and r.read_gbuffer().tobytes() == ref["G"].tobytes()


# ---- 8. refused contexts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["no_gbuffer", "gbuffer_only", "counters", "nshards", "nshards_gbuffer", "graph"])
def test_refused_contexts(rm, gpu, kind):
    W, H = 64, 48
    u = main_u(rm)
    lib = rm.lib()
    kw, edges = {"no_gbuffer": (dict(outputs=BOTH), ID),
                 "gbuffer_only": (dict(outputs=rm.RM_OUT_GBUFFER), ID),
                 "counters": (dict(outputs=BOTH, counters=True), COLOR),
                 "nshards": (dict(outputs=BOTH, nshards=2, shard=0, row_block=8), COLOR),
                 "nshards_gbuffer": (dict(outputs=ALL, nshards=2, shard=0, row_block=8), GEOMETRY | COLOR),
                 "graph": (dict(outputs=BOTH), COLOR)}[kind]
    with rm.Renderer(W, H, outputs=BOTH) as p:
        p.dispatch(u)
        want = p.read_rgba8()
    with rm.Renderer(W, H, **kw) as r:
        if kind == "graph":
            r.graph_enable(True)
        r.set_uniforms(u)
        cr = criteria(rm, edges)
        assert lib.rm_dispatch_adaptive_edges(r.handle, C.byref(cr)) == rm.RM_ERR_STATE
        assert "rm_dispatch_adaptive_edges" in lib.rm_last_error(r.handle).decode()
        if kind == "no_gbuffer":  # every geometry bit, alone and beside COLOR
            for e in (DEPTH, NORMAL, ALBEDO, COLOR | ID):
                cr = criteria(rm, e)
                assert lib.rm_dispatch_adaptive_edges(r.handle, C.byref(cr)) == rm.RM_ERR_STATE
        # the context renders correctly afterwards
        r.dispatch(u)
        if kind == "gbuffer_only":
            assert (r.read_gbuffer()["t"] != np.float32(-1.0)).any()
        elif kind.startswith("nshards"):
            assert r.read_rgba8().any()
        else:
            assert r.read_rgba8().tobytes() == want.tobytes()
        if kind in ("graph", "no_gbuffer"):  # with the graph off again, or with COLOR alone, the call works
            if kind == "graph":
                r.graph_enable(False)
            r.dispatch_adaptive_edges(u, COLOR, color_threshold=255)
            assert r.read_rgba8().tobytes() == want.tobytes() and r.aa_refined() == 0


# ---- 9. refused arguments ------------------------------------------------------------------------------------------
def test_refused_arguments(rm, gpu):
    W, H = 37, 23
    lib = rm.lib()
    u = main_u(rm)
    ref = refs(rm, W, H)
    nan = float("nan")
    bad = [("edges = 0", criteria(rm, 0), None),
           ("an unknown bit", criteria(rm, ID | 32), None),
           ("a high unknown bit", criteria(rm, 1 << 31), None),
           ("struct_size + 4", criteria(rm, ID, size=24), None),
           ("struct_size - 4", criteria(rm, ID, size=16), None),
           ("color_threshold 256", criteria(rm, COLOR, color_threshold=256), GEOMETRY),
           ("color_threshold -1", criteria(rm, COLOR | ID, color_threshold=-1), GEOMETRY),
           ("depth_rel -1", criteria(rm, DEPTH, depth_rel=-1.0), ID | NORMAL | ALBEDO | COLOR),
           ("depth_rel NaN", criteria(rm, DEPTH | ID, depth_rel=nan), ID | NORMAL | ALBEDO | COLOR),
           ("normal_cos 2", criteria(rm, NORMAL, normal_cos=2.0), ID | DEPTH | ALBEDO | COLOR),
           ("normal_cos NaN", criteria(rm, NORMAL | COLOR, normal_cos=nan), ID | DEPTH | ALBEDO | COLOR)]
    with rm.Renderer(W, H, outputs=ALL) as r:
        r.set_uniforms(u)
        out = np.full((H, W), 5, np.uint8)
        assert lib.rm_dispatch_adaptive_edges(r.handle, None) == rm.RM_ERR_INVALID
        assert "rm_dispatch_adaptive_edges" in lib.rm_last_error(r.handle).decode()
        assert lib.rm_read_aa_mask(r.handle, out.ctypes.data, 0, 0) == rm.RM_ERR_STATE  # none yet
        assert (out == 5).all()
        for what, cr, accepted_with in bad:
            before = bytes(cr)
            assert lib.rm_dispatch_adaptive_edges(r.handle, C.byref(cr)) == rm.RM_ERR_INVALID, what
            assert "rm_dispatch_adaptive_edges" in lib.rm_last_error(r.handle).decode(), what
            assert bytes(cr) == before
            # the context renders correctly after the refusal
            check_edges(r, u, ID | DEPTH | NORMAL, ref, f"after {what}")
            if accepted_with is not None:
                # the same bad value is not read when its bit is clear
                cr.edges = accepted_with
                par = dict(color_threshold=cr.color_threshold, depth_rel=cr.depth_rel, normal_cos=cr.normal_cos)
                good = dict(DEFAULTS)
                good.update({k: v for k, v in par.items() if k in _read_under(accepted_with)})
                assert lib.rm_dispatch_adaptive_edges(r.handle, C.byref(cr)) == rm.RM_OK, what
                with np.errstate(all="ignore"):
                    want = edge_mask(ref["G"], ref["A"][0], accepted_with, **good)
                    check_frame(r, want, ref["A"], ref["B"], f"{what}, bit clear", ref["G"])
        # the mask's pointer and readers work on a G-buffer context
        assert r.aa_mask_ptr() != 0
        assert lib.rm_read_aa_mask(r.handle, out.ctypes.data, W - 1, 0) == rm.RM_ERR_INVALID
        # and the three older calls keep refusing it
        assert lib.rm_dispatch_adaptive(r.handle, 8) == rm.RM_ERR_STATE
        assert lib.rm_dispatch_refine_device(r.handle, r.aa_mask_ptr(), 0) == rm.RM_ERR_STATE


def _read_under(edges):
    return ({"color_threshold"} if edges & COLOR else set()) | ({"depth_rel"} if edges & DEPTH else set()) | \
        ({"normal_cos"} if edges & NORMAL else set())
