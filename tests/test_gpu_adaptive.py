"""Adaptive supersampling on the GPU (rm_dispatch_adaptive, rm_dispatch_refine /
_device, rm_read_aa_mask, rm_get_aa_mask, rm_aa_refined).

Throughout, A is rm_dispatch with AA off and B rm_dispatch with AA on, on a plain
context with both colour outputs (tests/frames.py refs); C and M are the adaptive frame
and its mask.  The definition (tests/adaptive_checks.py check_frame): M is the flagging
rule (tests/adaptive_model.py) applied to A's RGBA8 image, or the caller's mask normalised
to 0 / 1, and C is where(M, B, A), byte for byte in RGBA8 and bit for bit (as uint32) in
RGBA32F.

Main frame: rm_sweep_uniforms(60, 120, 1, ., 0) at 130 x 67: ragged for the 8x8 tiles
and for the refinement's groups of 16, and its primary rays hit every object id.
"""
import ctypes as C

import numpy as np
import pytest

from adaptive_checks import ADAPTIVE_CALLS, caller_masks, check_frame, expected, refused
from adaptive_model import flag_mask
from frames import BOTH, ab, images, refs, renderer
from scenes import scene_of
from uniforms import main_u, off_sweep_uniforms, with_aa

pytestmark = pytest.mark.gpu

W0, H0 = 130, 67
SHAPES = [(130, 67), (37, 23), (9, 5), (1, 1)]


def check_adaptive(rm, r, u, thr, A, B, what):
    r.dispatch_adaptive(u, thr)
    return check_frame(r, flag_mask(A[0], thr), A, B, what)


# ---- 1. adaptive equals its definition -------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 2])
@pytest.mark.parametrize("W,H", SHAPES)
def test_adaptive_equals_definition(rm, gpu, W, H, bounces):
    u = main_u(rm, bounces)
    A, B = ab(refs(rm, W, H, bounces))
    with rm.Renderer(W, H, outputs=BOTH) as r:
        for thr in (0, 16, 255):
            M, c8, _ = check_adaptive(rm, r, u, thr, A, B, f"{W}x{H} b{bounces} thr{thr}")
            if thr == 255:
                assert not M.any() and c8.tobytes() == A[0].tobytes()
            if (W, H) == (1, 1):
                assert not M.any()
            if (W, H) == (W0, H0) and thr == 16:
                # the oracle's frame gives 0.466 at one bounce, and the GPU's pixels are within
                # 1 LSB of it, which moves a few dozen pixels at most
                assert 0.3 < M.mean() < 0.6, M.mean()
                assert (c8 != A[0]).any() and (c8 != B[0]).any()
        # u.AA is ignored, and the uniforms stay as they are
        r.dispatch_adaptive(with_aa(u, True), 16)
        assert r.get_uniforms().AA == 1
        check_frame(r, flag_mask(A[0], 16), A, B, "u.AA = 1")


@pytest.mark.parametrize("shadow", [0, 1])
def test_both_shadow_modes(rm, gpu, shadow):
    u = main_u(rm, 1, shadow)
    A, B = ab(refs(rm, W0, H0, 1, shadow))
    with rm.Renderer(W0, H0, outputs=BOTH) as r:
        check_adaptive(rm, r, u, 16, A, B, f"shadow {shadow}")
    if shadow:
        assert A[0].tobytes() != ab(refs(rm, W0, H0))[0][0].tobytes()


@pytest.mark.parametrize("thr", [0, 16])
def test_rgba32f_only_context(rm, gpu, thr):
    u = main_u(rm)
    A, B = ab(refs(rm, W0, H0))
    with rm.Renderer(W0, H0, outputs=rm.RM_OUT_RGBA32F) as r:
        r.dispatch_adaptive(u, thr)
        M = r.read_aa_mask()
        np.testing.assert_array_equal(M, flag_mask(A[0], thr))
        np.testing.assert_array_equal(r.read_rgba32f().view(np.uint32), expected(M, A, B)[1])
        assert r.aa_refined() == int(M.sum())


# ---- 2. against the oracle directly ------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(130, 67), (37, 23)])
def test_against_the_oracle(rm, oracle, gpu, W, H):
    u = main_u(rm)
    off = oracle.render(with_aa(u, False), W, H, want_counts=False)["rgba8"]
    on = oracle.render(with_aa(u, True), W, H, want_counts=False)["rgba8"]
    with rm.Renderer(W, H, outputs=BOTH) as r:
        r.dispatch_adaptive(u, 16)
        M, c8 = r.read_aa_mask(), r.read_rgba8()
    want = np.where(M.astype(bool)[..., None], on, off).astype(np.int16)
    d = np.abs(c8.astype(np.int16) - want)
    print(f"{W}x{H}: flagged {int(M.sum())}, max |delta| {int(d.max())} LSB, {int((d > 0).sum())} values differ")
    assert d.max() <= 1  # the project's RGBA8 bar
    assert M.any() and not M.all()


# ---- 3. caller masks, host and device -----------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "device"])
def test_caller_masks(rm, gpu, where):
    import torch
    W, H = W0, H0
    u = main_u(rm)
    A, B = ab(refs(rm, W, H))
    masks = caller_masks(W, H)
    assert masks["random"].sum() % 16 != 0 and set(np.unique(masks["values"])) == {0, 2, 255}
    with rm.Renderer(W, H, outputs=BOTH) as r:
        for name, m in masks.items():
            if where == "host":
                r.dispatch_refine(m, u)
            else:
                t = torch.from_numpy(m).to(f"cuda:{r.device}")
                torch.cuda.synchronize()
                r.dispatch_refine(t.data_ptr(), u)
            M, c8, c32 = check_frame(r, (m != 0).astype(np.uint8), A, B, f"{where} {name}")
            if name == "ones":  # the refine path alone reproduces the AA-on frame
                assert c8.tobytes() == B[0].tobytes() and c32.tobytes() == B[1].tobytes()
            if name == "zeros":
                assert c8.tobytes() == A[0].tobytes() and c32.tobytes() == A[1].tobytes()
            if name == "values":
                assert set(np.unique(M)) == {0, 1}
        # a padded row_pitch, and flip_y
        m = masks["random"]
        wide = np.full((H, W + 13), 9, np.uint8)
        wide[:, :W] = m
        if where == "host":
            r.dispatch_refine(wide[:, :W], u)
        else:
            t = torch.from_numpy(wide).to(f"cuda:{r.device}")
            torch.cuda.synchronize()
            r.dispatch_refine(t.data_ptr(), u, row_pitch=W + 13)
        check_frame(r, m, A, B, f"{where} padded")
        np.testing.assert_array_equal(r.read_aa_mask(flip_y=True), m[::-1])
        out = np.full((H, W + 5), 77, np.uint8)
        assert rm.lib().rm_read_aa_mask(r.handle, out.ctypes.data, W + 5, 0) == rm.RM_OK
        assert (out[:, :W] == m).all() and (out[:, W:] == 77).all()
        # the context's own mask as the device mask: the previous frame's flags again
        r.dispatch_refine(r.aa_mask_ptr(), u)
        check_frame(r, m, A, B, f"{where} own mask")


# ---- 4. the stride loop ---------------------------------------------------------------------------
def test_stride_loop(rm, gpu, monkeypatch):
    W, H = W0, H0
    u = main_u(rm)
    A, B = ab(refs(rm, W, H))
    masks = caller_masks(W, H)
    monkeypatch.setenv("RM_AA_REFINE_WAVES", "3")  # 8710 pixels: 545 groups over 3 waves
    with rm.Renderer(W, H, outputs=BOTH) as r:
        monkeypatch.delenv("RM_AA_REFINE_WAVES")  # read at rm_create
        for name in ("ones", "random"):
            r.dispatch_refine(masks[name], u)
            check_frame(r, masks[name], A, B, f"3 waves, {name}")
        check_adaptive(rm, r, u, 16, A, B, "3 waves, adaptive")


# ---- 5. tables ----------------------------------------------------------------------------------------
def test_default_scene_table_equals_builtin(rm, gpu):
    u = main_u(rm)
    with rm.Renderer(W0, H0, outputs=BOTH) as r:
        r.dispatch_adaptive(u, 16)
        want = (r.read_aa_mask().tobytes(),) + tuple(x.tobytes() for x in images(r))
        r.set_scene(rm.default_scene())
        r.dispatch_adaptive(u, 16)
        assert (r.read_aa_mask().tobytes(),) + tuple(x.tobytes() for x in images(r)) == want


# (specialised: pass 1 by the table's hiprtc kernels, the refinement by the generic code;
# one table, the quickest to compile)
@pytest.mark.parametrize("which,specialize", [("random0", False), ("random1", False), ("floor0", False),
                                              ("floor0", True)],
                         ids=["random0", "random1", "floor0", "floor0-specialised"])
def test_tables(rm, gpu, which, specialize):
    scene = scene_of(rm, which)
    u = main_u(rm)
    A, B = ab(refs(rm, W0, H0, name=which))
    with renderer(rm, W0, H0, scene, specialize=specialize) as r:
        check_adaptive(rm, r, u, 16, A, B, which)
        r.dispatch_refine(np.ones((H0, W0), np.uint8), u)
        check_frame(r, np.ones((H0, W0), np.uint8), A, B, f"{which} all ones")


# ---- 6. uniforms off the sweep ------------------------------------------------------------------------
@pytest.mark.parametrize("i", range(5), ids=[f"case{i}" for i in range(4)] + ["nan_camera"])
def test_off_sweep_uniforms(rm, gpu, i):
    u, (W, H) = off_sweep_uniforms(rm, i if i < 4 else 16)  # 16: one non-finite camera
    assert (W, H) == (67, 41)
    with np.errstate(all="ignore"):
        A, B = ab(refs(rm, W, H, u=u))
        with rm.Renderer(W, H, outputs=BOTH) as r:
            check_adaptive(rm, r, u, 8, A, B, f"case {i}")


# ---- 7. not sticky, reusable -------------------------------------------------------------------------
def test_not_sticky_and_reusable(rm, gpu):
    W, H = W0, H0
    u, u2 = main_u(rm, 1, aa=True), rm.sweep_uniforms(20, 120, 2, False, 0)
    A, B = ab(refs(rm, W, H))
    A2, _ = ab(refs(rm, W, H, u=u2))
    masks = caller_masks(W, H)
    with rm.Renderer(W, H, outputs=BOTH) as r:
        r.enable_timing(True)
        _, n0 = r.kernel_time_ms()
        check_adaptive(rm, r, u, 16, A, B, "first")
        ptr = r.aa_mask_ptr()
        r.dispatch(u)  # the plain AA-on frame, as always
        assert r.read_rgba8().tobytes() == B[0].tobytes() and r.read_rgba32f().tobytes() == B[1].tobytes()
        r.dispatch_frames([u, u2])
        assert r.read_frame_rgba8(0).tobytes() == B[0].tobytes()
        assert r.read_frame_rgba8(1).tobytes() == A2[0].tobytes()
        assert r.read_rgba32f().tobytes() == A2[1].tobytes()
        ms, n1 = r.kernel_time_ms()
        assert n1 - n0 == 4 and ms > 0.0  # one launch of one frame per adaptive dispatch; the batch counts 2
        # two thresholds, then a mask: the buffers are reused and each frame is right
        check_adaptive(rm, r, u, 4, A, B, "thr 4")
        check_adaptive(rm, r, u, 32, A, B, "thr 32")
        r.dispatch_refine(masks["checker"], u)
        check_frame(r, masks["checker"], A, B, "then a mask")
        assert r.aa_mask_ptr() == ptr
        _, n2 = r.kernel_time_ms()
        assert n2 - n1 == 3
        # the mask and the count stay those of the last such dispatch
        r.dispatch(u2)
        np.testing.assert_array_equal(r.read_aa_mask(), masks["checker"])
        assert r.aa_refined() == int(masks["checker"].sum())


# ---- 8. stream interop ----------------------------------------------------------------------------------
def test_stream_interop(rm, gpu):
    import torch
    W, H = W0, H0
    u = main_u(rm)
    A, B = ab(refs(rm, W, H))
    m = caller_masks(W, H)["random"]
    want8 = expected(m, A, B)[0]
    with rm.Renderer(W, H, outputs=BOTH) as r:
        dev = torch.device("cuda", r.device)
        s, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        host = torch.from_numpy(m).pin_memory()
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(s):
                r.set_stream(s.cuda_stream)
                r.set_output_rgba8(out.data_ptr())
                mask = torch.empty((H, W), dtype=torch.uint8, device=dev)
                mask.copy_(host, non_blocking=True)  # filled on the stream, no host sync after it
                mask.mul_(3)                         # any non-zero byte
                r.dispatch_refine(mask.data_ptr(), u)
                got = out.cpu()                      # ordered after the frame on the same stream
                assert got.numpy().tobytes() == want8.tobytes()
                # rm_wait_output orders a second stream after the frame
                out.zero_()
                r.dispatch_adaptive(u, 16)
                r.wait_output(s2.cuda_stream)
                with torch.cuda.stream(s2):
                    again = out.clone()
                s2.synchronize()
                assert again.cpu().numpy().tobytes() == expected(flag_mask(A[0], 16), A, B)[0].tobytes()
            np.testing.assert_array_equal(r.read_aa_mask(), flag_mask(A[0], 16))
        finally:
            r.synchronize()
            r.set_output_rgba8(None)
            r.set_stream(None)


# ---- 9. refusals -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["counters", "nshards", "gbuffer", "graph", "ngpus", "communicator"])
def test_refused_contexts(rm, gpu, kind):
    import torch
    W, H = 64, 48
    u = main_u(rm)
    mask = np.ones((H, W), np.uint8)
    kw = {"counters": dict(counters=True), "nshards": dict(nshards=2, shard=0, row_block=8),
          "gbuffer": dict(outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER), "graph": {},
          "ngpus": dict(ngpus=1, row_block=8), "communicator": dict(row_block=8, shard=0, nshards=1)}[kind]
    ref = None
    if kind in ("graph", "communicator", "gbuffer"):
        with rm.Renderer(W, H) as p:
            p.dispatch(u)
            ref = p.read_rgba8()
    with rm.Renderer(W, H, **kw) as r:
        dev = torch.ones((H, W), dtype=torch.uint8, device=f"cuda:{max(r.device, 0)}")
        torch.cuda.synchronize()
        if kind == "communicator":
            r.comm_init(rm.comm_unique_id(), 1, 0)
        if kind == "graph":
            r.graph_enable(True)
        r.set_uniforms(u)
        refused(rm, r, rm.RM_ERR_STATE, None, None, mask, dev.data_ptr(), calls=ADAPTIVE_CALLS)
        # the context renders correctly afterwards
        r.dispatch(u)
        img = r.read_rgba8()
        assert img.any()
        if ref is not None:
            assert img.tobytes() == ref.tobytes()
        if kind == "graph":  # and with the graph off again the calls work
            r.graph_enable(False)
            r.dispatch_adaptive(u, 255)
            assert r.read_rgba8().tobytes() == ref.tobytes() and r.aa_refined() == 0


def test_refused_arguments_and_order(rm, gpu):
    import torch
    W, H = 64, 48
    lib = rm.lib()
    u = main_u(rm)
    A, B = ab(refs(rm, W, H))
    mask = np.ones((H, W), np.uint8)
    with rm.Renderer(W, H, outputs=BOTH) as r:
        dev = torch.ones((H, W), dtype=torch.uint8, device=f"cuda:{r.device}")
        torch.cuda.synchronize()
        r.set_uniforms(u)
        out = np.full((H, W), 5, np.uint8)
        n = C.c_int64(-3)
        # before the first such dispatch (a plain dispatch does not count)
        r.dispatch(u)
        assert lib.rm_read_aa_mask(r.handle, out.ctypes.data, 0, 0) == rm.RM_ERR_STATE
        assert "rm_read_aa_mask" in lib.rm_last_error(r.handle).decode()
        assert lib.rm_aa_refined(r.handle, C.byref(n)) == rm.RM_ERR_STATE
        assert "rm_aa_refined" in lib.rm_last_error(r.handle).decode()
        assert (out == 5).all() and n.value == -3
        for thr in (-1, 256, 1 << 20):
            assert lib.rm_dispatch_adaptive(r.handle, thr) == rm.RM_ERR_INVALID
            assert "rm_dispatch_adaptive" in lib.rm_last_error(r.handle).decode()
        assert lib.rm_dispatch_refine(r.handle, None, 0) == rm.RM_ERR_INVALID
        assert "rm_dispatch_refine" in lib.rm_last_error(r.handle).decode()
        assert lib.rm_dispatch_refine_device(r.handle, None, 0) == rm.RM_ERR_INVALID
        assert "rm_dispatch_refine_device" in lib.rm_last_error(r.handle).decode()
        assert lib.rm_dispatch_refine(r.handle, mask.ctypes.data, W - 1) == rm.RM_ERR_INVALID
        assert lib.rm_dispatch_refine_device(r.handle, dev.data_ptr(), W - 1) == rm.RM_ERR_INVALID
        assert "row_pitch" in lib.rm_last_error(r.handle).decode()
        assert lib.rm_get_aa_mask(r.handle, None) == rm.RM_ERR_INVALID
        assert lib.rm_read_aa_mask(r.handle, out.ctypes.data, 0, 0) == rm.RM_ERR_STATE  # still none
        # the context renders correctly afterwards
        check_adaptive(rm, r, u, 16, A, B, "after the refusals")
        assert lib.rm_read_aa_mask(r.handle, out.ctypes.data, W - 1, 0) == rm.RM_ERR_INVALID
        assert lib.rm_read_aa_mask(r.handle, None, 0, 0) == rm.RM_ERR_INVALID
