"""Sample-pattern frames on the GPU (rm_dispatch_pattern; include/rm_api.h
RM_HAS_SAMPLE_PATTERN).

Every frame is rm_sweep_uniforms(60, 120, b, ., s) on a context with both colour outputs.
The shapes: 37 x 23 is ragged for the 4x4 tiles on both axes, 9 x 5 and 1 x 1 are the
small cases, and 261 x 6 has 66 tile columns, past one 64-block window of tile_col.

"Model" is the header's rule with nothing of the frame kernels in it (tests/patterns.py
model, equals_model); the plain AA-off and AA-on frames are tests/frames.py refs' A and B.
"""
import ctypes as C

import numpy as np
import pytest

from frames import images, refs, renderer, same_frame
from patterns import equals_model, model, patterns
from scenes import scene_of
from uniforms import main_u

pytestmark = pytest.mark.gpu

SHAPES = [(37, 23), (9, 5), (1, 1), (261, 6)]
SCENES = ["builtin", "default-table", "random-table"]


# ---- 1, 2. the two anchors: the AA-on and the AA-off frame ----------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_reference_pattern_is_the_aa_frame(rm, gpu, W, H, name):
    ref = rm.sample_pattern(rm.RM_PATTERN_REFERENCE)
    with renderer(rm, W, H, scene_of(rm, name)) as r:
        for bounces in (0, 2):
            for shadow in (0, 1):
                r.dispatch_pattern(main_u(rm, bounces, shadow), ref)
                same_frame(images(r), refs(rm, W, H, bounces, shadow, name)["B"], f"{name} {W}x{H} b{bounces} s{shadow}")


@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_one_centre_sample_is_the_plain_frame(rm, gpu, W, H, name):
    centre = rm.custom_pattern([0.0], [0.0])
    with renderer(rm, W, H, scene_of(rm, name)) as r:
        for bounces in (0, 2):
            for shadow in (0, 1):
                r.dispatch_pattern(main_u(rm, bounces, shadow), centre)
                same_frame(images(r), refs(rm, W, H, bounces, shadow, name)["A"], f"{name} {W}x{H} b{bounces} s{shadow}")
    if (W, H) == (37, 23):  # the anchors are two different frames
        assert refs(rm, W, H, 2, 0, name)["A"][0].tobytes() != refs(rm, W, H, 2, 0, name)["B"][0].tobytes()


# ---- 3. every other pattern against the model ---------------------------------------------------
@pytest.mark.parametrize("name,W,H", [("builtin", 37, 23), ("builtin", 261, 6), ("random-table", 37, 23)])
def test_frame_equals_model(rm, oracle, gpu, name, W, H):
    u = main_u(rm, 2)
    with renderer(rm, W, H, scene_of(rm, name)) as r:
        for pname, p in patterns(rm).items():
            r.dispatch_pattern(u, p)
            got = images(r)
            equals_model(got, model(rm, oracle, r, u, p), f"{name} {W}x{H} {pname}")
            assert (got[1][..., 3] == 1.0).all()


# ---- 4. the sum follows the pattern's order --------------------------------------------------------
def test_sample_order_is_the_sum_order(rm, oracle, gpu):
    W, H = 37, 23
    u = main_u(rm, 2)
    g4 = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    perm = np.random.default_rng(4).permutation(16)
    pp = rm.custom_pattern([g4.dx[i] for i in perm], [g4.dy[i] for i in perm])
    with renderer(rm, W, H) as r:
        r.dispatch_pattern(u, g4)
        f1 = images(r)
        m1 = model(rm, oracle, r, u, g4)
        r.dispatch_pattern(u, pp)
        f2 = images(r)
        m2 = model(rm, oracle, r, u, pp)
    equals_model(f1, m1, "grid4")
    equals_model(f2, m2, "grid4 permuted")
    ok = ~(np.isnan(m1[1]) | np.isnan(m2[1]))
    dm = m1[1].view(np.uint32) ^ m2[1].view(np.uint32)
    assert dm[ok].any(), "the two orders round differently somewhere in this frame"
    df = f1[1].view(np.uint32) ^ f2[1].view(np.uint32)
    np.testing.assert_array_equal(df[ok], dm[ok])


# ---- 5. offsets far outside the pixel: the uv range of the pattern, not of the frame ------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_sixteen_pixel_offsets(rm, oracle, gpu, name):
    W, H = 37, 23
    u = main_u(rm, 2)
    p = rm.custom_pattern([16.0, -16.0, 16.0, -16.0], [16.0, 16.0, -16.0, -16.0])
    with renderer(rm, W, H, scene_of(rm, name)) as r:
        r.dispatch_pattern(u, p)
        got = images(r)
        equals_model(got, model(rm, oracle, r, u, p), f"{name} +-16")
    assert got[0].tobytes() != refs(rm, W, H, 2, 0, name)["A"][0].tobytes()


# ---- 6. one colour output ----------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_single_output_contexts(rm, gpu, name):
    W, H = 37, 23
    u = main_u(rm, 1)
    p = rm.sample_pattern(rm.RM_PATTERN_GRID3)  # three rounds, the last with one sample
    with renderer(rm, W, H, scene_of(rm, name)) as r:
        r.dispatch_pattern(u, p)
        want = images(r)
    with renderer(rm, W, H, scene_of(rm, name), outputs=rm.RM_OUT_RGBA8) as r:
        r.dispatch_pattern(u, p)
        assert r.read_rgba8().tobytes() == want[0].tobytes()
    with renderer(rm, W, H, scene_of(rm, name), outputs=rm.RM_OUT_RGBA32F) as r:
        r.dispatch_pattern(u, p)
        np.testing.assert_array_equal(r.read_rgba32f().view(np.uint32), want[1].view(np.uint32))


# ---- 7. the caller's image and stream ---------------------------------------------------------------
def test_caller_output_and_stream(rm, gpu):
    import torch
    W, H = 37, 23
    u = main_u(rm, 1)
    g2, rg = rm.sample_pattern(rm.RM_PATTERN_GRID2), rm.sample_pattern(rm.RM_PATTERN_RGSS)
    with renderer(rm, W, H) as r:
        r.dispatch_pattern(u, g2)
        want_g2 = r.read_rgba8()
        r.dispatch_pattern(u, rg)
        want_rg = r.read_rgba8()
        assert want_g2.tobytes() != want_rg.tobytes()
        dev = torch.device("cuda", r.device)
        s, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(s):
                r.set_stream(s.cuda_stream)
                r.set_output_rgba8(out.data_ptr())
                assert r.output_rgba8_ptr() == out.data_ptr()
                r.dispatch_pattern(u, g2)  # another pattern than the last: its table is uploaded on s
                first = out.clone()
                r.dispatch_pattern(u, rg)
                r.wait_output(s2.cuda_stream)
                with torch.cuda.stream(s2):
                    second = out.clone()
                s2.synchronize()
            s.synchronize()
            assert first.cpu().numpy().tobytes() == want_g2.tobytes()
            assert second.cpu().numpy().tobytes() == want_rg.tobytes()
            assert r.read_rgba8().tobytes() == want_rg.tobytes()
        finally:
            r.synchronize()
            r.set_output_rgba8(None)
            r.set_stream(None)
        r.dispatch_pattern(u, g2)
        assert r.read_rgba8().tobytes() == want_g2.tobytes()


# ---- 8. rm_scene_specialize: the generic table code renders, the same image --------------------
def test_specialised_context_gives_the_same_image(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 2)
    scene = scene_of(rm, "floor-table")
    p = rm.sample_pattern(rm.RM_PATTERN_GRID3)
    with renderer(rm, W, H, scene) as r:
        r.dispatch_pattern(u, p)
        want = images(r)
    with renderer(rm, W, H, scene, specialize=True) as r:
        r.dispatch_pattern(u, p)
        same_frame(images(r), want, "specialised")
        r.dispatch_pattern(u, rm.sample_pattern(rm.RM_PATTERN_REFERENCE))
        r2 = images(r)
        r.dispatch(main_u(rm, 2, 0, True))  # the specialised AA kernel
        same_frame(r2, images(r), "specialised reference")


# ---- 9. nothing is sticky -----------------------------------------------------------------------------
def test_uniforms_stay_and_later_dispatches_are_unchanged(rm, gpu):
    W, H = 37, 23
    u_on = main_u(rm, 1, 0, True)
    with renderer(rm, W, H) as fresh:
        fresh.dispatch(u_on)
        want_plain = images(fresh)
    with renderer(rm, W, H) as fresh:
        fresh.dispatch_adaptive(u_on, 16)
        want_adaptive = images(fresh)
    g4 = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    with renderer(rm, W, H) as r:
        r.dispatch_pattern(main_u(rm, 1, 0, False), g4)
        off = images(r)
        r.dispatch_pattern(u_on, g4)  # u.AA = 1 is ignored ...
        same_frame(images(r), off, "u.AA ignored")
        assert bytes(r.get_uniforms()) == bytes(u_on)  # ... and stays
        r.dispatch()
        same_frame(images(r), want_plain, "rm_dispatch afterwards")
        r.dispatch_pattern(None, g4)
        r.dispatch_adaptive(None, 16)
        same_frame(images(r), want_adaptive, "rm_dispatch_adaptive afterwards")
        assert bytes(r.get_uniforms()) == bytes(u_on)
        # patterns in turn: the table follows the pattern, and a repeated one is the same frame
        g2, rg = rm.sample_pattern(rm.RM_PATTERN_GRID2), rm.sample_pattern(rm.RM_PATTERN_RGSS)
        seen = {}
        for k, p in [("g2", g2), ("rg", rg), ("g4", g4), ("g2", g2), ("g2", g2), ("g4", g4), ("rg", rg)]:
            r.dispatch_pattern(None, p)
            now = images(r)
            if k in seen:
                same_frame(now, seen[k], f"{k} again")
            seen[k] = now
        same_frame(seen["g4"], off, "grid4 again")
        assert seen["g2"][1].tobytes() != seen["rg"][1].tobytes()


# ---- 10. timing ---------------------------------------------------------------------------------------
def test_one_timed_launch(rm, gpu):
    with renderer(rm, 37, 23) as r:
        r.enable_timing(True)
        _, n0 = r.kernel_time_ms()
        r.dispatch_pattern(main_u(rm, 1), rm.sample_pattern(rm.RM_PATTERN_GRID4))
        ms, n1 = r.kernel_time_ms()
        assert n1 - n0 == 1 and ms > 0.0
        r.dispatch_pattern(None, rm.RM_PATTERN_GRID3)  # a new table: the upload is outside the bracket's count
        r.dispatch_pattern(None, rm.RM_PATTERN_GRID3)
        _, n2 = r.kernel_time_ms()
        assert n2 - n1 == 2
        assert r.frame_phases()["render_ms"] > 0.0


# ---- 11. refusals ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["counters", "nshards", "gbuffer", "graph"])
def test_refused_contexts(rm, gpu, kind):
    W, H = 64, 48
    u = main_u(rm, 1)
    p = rm.sample_pattern(rm.RM_PATTERN_GRID2)
    kw = {"counters": dict(counters=True), "nshards": dict(nshards=2, shard=0, row_block=8),
          "gbuffer": dict(outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER), "graph": {}}[kind]
    with rm.Renderer(W, H, **kw) as r:
        if kind == "graph":
            r.graph_enable(True)
            r.graph_dispatch(u)
        else:
            r.dispatch(u)
        before = r.read_rgba8()
        assert rm.lib().rm_dispatch_pattern(r.handle, C.byref(p)) == rm.RM_ERR_STATE
        assert "rm_dispatch_pattern" in rm.lib().rm_last_error(r.handle).decode()
        assert r.read_rgba8().tobytes() == before.tobytes()
        if kind == "graph":  # and with the graph off again the call works
            r.graph_enable(False)
            r.dispatch_pattern(u, rm.custom_pattern([0.0], [0.0]))
            assert r.read_rgba8().tobytes() == before.tobytes()


def test_refused_patterns(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 1)
    L = rm.lib()
    with renderer(rm, W, H) as r:
        r.dispatch_pattern(u, rm.RM_PATTERN_RGSS)
        before = images(r)
        assert L.rm_dispatch_pattern(r.handle, None) == rm.RM_ERR_INVALID
        ok = rm.sample_pattern(rm.RM_PATTERN_GRID3)
        for field, bad, word in (("struct_size", 136, "struct_size"), ("flags", 2, "flags"), ("n", 0, "n must"),
                                 ("n", 17, "n must")):
            p = rm.rm_sample_pattern.from_buffer_copy(ok)
            setattr(p, field, bad)
            assert L.rm_dispatch_pattern(r.handle, C.byref(p)) == rm.RM_ERR_INVALID, field
            msg = L.rm_last_error(r.handle).decode()
            assert "rm_dispatch_pattern" in msg and word in msg, msg
        for v in (float("nan"), float("inf"), 16.5, -17.0):
            for at in (0, 8):
                p = rm.rm_sample_pattern.from_buffer_copy(ok)
                p.dy[at] = v
                assert L.rm_dispatch_pattern(r.handle, C.byref(p)) == rm.RM_ERR_INVALID, (v, at)
                assert "offset" in L.rm_last_error(r.handle).decode()
            p = rm.rm_sample_pattern.from_buffer_copy(ok)
            p.dx[9] = v  # not read
            r.dispatch_pattern(u, p)
            r.dispatch_pattern(u, rm.RM_PATTERN_RGSS)
        same_frame(images(r), before, "after the refusals")
