"""Progressive accumulation on the GPU (rm_dispatch_accumulate; include/rm_api.h
RM_HAS_ACCUMULATION).

Every frame is rm_sweep_uniforms(60, 120, b, ., 0) on a context with both colour outputs unless
a test says otherwise.  The shapes are the pattern tests': 37 x 23 is ragged for the 4x4 and the
8x8 tiles on both axes, 9 x 5 and 1 x 1 are the small cases, and 261 x 6 has 66 tile columns,
past one window of tile_col.

The references are other calls of the same library (rm_dispatch_pattern's frames, tests/frames.py)
for the first two anchors, and the rule in numpy float32 (tests/accum_model.py) on the same
context's SHADE traces past them.  Frames are compared bit for bit as uint32 and byte for byte
(frames.same_frame, patterns.equals_model), the sum image as uint32 (records.bits_equal)."""
import ctypes as C

import numpy as np
import pytest

import accum_model as AM
from frames import images, pattern_frame, refs, renderer, same_frame
from patterns import equals_model, refine_patterns
from records import bits_equal
from scenes import scene_of
from uniforms import main_u, with_aa

pytestmark = pytest.mark.gpu

SHAPES = [(37, 23), (9, 5), (1, 1), (261, 6)]
SCENES = ["builtin", "default-table", "random-table"]
# one round; 4 + 4 + 1; four rounds; 4 + 3; the one-sample kernels
ANCHOR1 = ("grid2", "grid3", "grid4", "abs7", "jitter1", "centre")
# the whole pattern and the sizes of the calls it is cut into
SPLITS = [("grid4", [4, 4, 4, 4]), ("grid4", [1, 6, 9]), ("grid4", [1] * 16), ("abs7", [3, 4])]


def moved(u, k):
    """u at another time, from another place and under another light."""
    v = type(u).from_buffer_copy(u)
    v.iTime = u.iTime + 0.37 * k
    v.camera.pos[0] = u.camera.pos[0] + 0.8 * k
    v.camera.pos[1] = u.camera.pos[1] + 0.3 * k
    v.light.position[0] = u.light.position[0] - 3.0 * k
    v.light.position[2] = u.light.position[2] + 2.0 * k
    return v


def check_state(r, acc, what):
    """The context's frame, sum image and count against the model's."""
    equals_model(images(r), acc.frame(), what)
    bits_equal(r.read_accum(), acc.image(), f"{what}: sum image")
    assert r.accum_samples() == acc.N, what


# ---- 1. anchor 1: with N == 0 one call is the pattern frame ------------------------------------
@pytest.mark.parametrize("name", SCENES)
@pytest.mark.parametrize("W,H", SHAPES)
def test_first_call_is_the_pattern_frame(rm, oracle, gpu, W, H, name):
    pats = refine_patterns(rm)
    for bounces in (0, 2):
        u = main_u(rm, bounces)
        with renderer(rm, W, H, scene_of(rm, name)) as r:
            assert r.accum_samples() == 0
            for i, pname in enumerate(ANCHOR1):
                p = pats[pname]
                want = pattern_frame(rm, W, H, p, pname, bounces, 0, name)
                # a fresh context; then after rm_accum_reset and with RM_ACCUM_RESTART, which
                # follow earlier accumulating calls
                for how in (("fresh",) if i == 0 else ()) + ("reset", "restart"):
                    what = f"{name} {W}x{H} b{bounces} {pname} {how}"
                    if how == "reset":
                        r.accum_reset()
                        assert r.accum_samples() == 0
                    r.dispatch_accumulate(u, p, restart=how == "restart")
                    same_frame(images(r), want, what)
                    assert r.accum_samples() == int(p.n), what
                acc = AM.run([AM.colours(rm, oracle, r, u, p)])
                check_state(r, acc, f"{name} {W}x{H} b{bounces} {pname}")
                assert (r.read_accum()[..., 3] == np.float32(int(p.n))).all()


# ---- 2. anchor 2: however a pattern's samples are split into calls ----------------------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
@pytest.mark.parametrize("W,H", [(37, 23), (261, 6)])
def test_split_calls_are_the_whole_patterns_frame(rm, gpu, W, H, name):
    u = main_u(rm, 2)
    pats = refine_patterns(rm)
    scene = scene_of(rm, name)
    with renderer(rm, W, H, scene) as r, renderer(rm, W, H, scene) as ref:
        for pname, sizes in SPLITS:
            p, at = pats[pname], 0
            r.accum_reset()
            for part in AM.split(p, sizes, rm.custom_pattern):
                r.dispatch_accumulate(u, part)
                at += int(part.n)
                what = f"{name} {W}x{H} {pname} {sizes} at {at}"
                ref.dispatch_pattern(u, AM.prefix(p, at, rm.custom_pattern))  # the prefix's pattern frame
                same_frame(images(r), images(ref), what)
                assert r.accum_samples() == at, what
                assert (r.read_accum()[..., 3] == np.float32(at)).all(), what
            same_frame(images(r), pattern_frame(rm, W, H, p, pname, 2, 0, name), f"{name} {W}x{H} {pname} {sizes}")


# ---- 3. past 16 samples: the running sum of the model ----------------------------------------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_past_sixteen_samples_is_the_running_sum(rm, oracle, gpu, name):
    W, H = 37, 23
    u = main_u(rm, 2)
    scene = scene_of(rm, name)
    acc = AM.Sum()
    with renderer(rm, W, H, scene) as r:
        for n in (1, 4, 7, 16, 1, 16):
            p = rm.halton_pattern(acc.N, n)
            acc.add(AM.colours(rm, oracle, r, u, p))  # (a trace between the calls: it leaves the sum alone)
            r.dispatch_accumulate(None, p)
            check_state(r, acc, f"{name} after {acc.N} samples")
        assert acc.N == 45
        last = images(r)
    # the convenience loop walks the same sequence in other calls (16 + 16 + 13): the same sum
    with renderer(rm, W, H, scene) as r:
        r.accumulate(u, 45)
        assert r.accum_samples() == 45
        same_frame(images(r), last, f"{name}: Renderer.accumulate")
        r.accumulate(None, 3, first=45)
        assert r.accum_samples() == 48


# ---- 4. the uniforms move between calls, and nothing resets by itself ---------------------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_uniforms_move_between_calls(rm, oracle, gpu, name):
    W, H = 37, 23
    pats = refine_patterns(rm)
    acc = AM.Sum()
    first = None
    with renderer(rm, W, H, scene_of(rm, name)) as r:
        for k, pname in enumerate(("grid2", "jitter1", "abs7", "grid3")):
            u = moved(main_u(rm, 1), k)
            cols = AM.colours(rm, oracle, r, u, pats[pname])
            first = cols if first is None else first
            acc.add(cols)
            r.dispatch_accumulate(u, pats[pname])
            check_state(r, acc, f"{name} call {k} ({pname})")
            assert bytes(r.get_uniforms()) == bytes(u)  # the last set, and they stay
        assert acc.N == 4 + 1 + 7 + 9
        # the calls rendered different frames: the same pattern under the last uniforms is another image
        again = AM.colours(rm, oracle, r, u, pats["grid2"])
        assert (again.view(np.uint32) != first.view(np.uint32)).any()


# ---- 5. other dispatches in between leave the sum alone -----------------------------------------------
def test_other_dispatches_in_between(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 1)
    u_on = with_aa(u, True)
    pats = refine_patterns(rm)
    g2, a7 = pats["grid2"], pats["abs7"]
    with renderer(rm, W, H) as fresh:
        fresh.dispatch_adaptive(u_on, 16)
        want_adaptive = images(fresh)
        both = rm.custom_pattern(list(g2.dx[:4]) + list(a7.dx[:7]), list(g2.dy[:4]) + list(a7.dy[:7]))
        fresh.dispatch_pattern(u, both)
        want_both = images(fresh)
    with renderer(rm, W, H) as r:
        r.dispatch_accumulate(u, g2)
        same_frame(images(r), pattern_frame(rm, W, H, g2, "grid2", 1, 0), "the first call")
        S = r.read_accum()
        r.dispatch(u_on)
        same_frame(images(r), refs(rm, W, H, 1, 0)["B"], "rm_dispatch with AA on")
        r.dispatch_pattern(u, pats["rgss"])
        same_frame(images(r), pattern_frame(rm, W, H, pats["rgss"], "rgss", 1, 0), "rm_dispatch_pattern")
        r.dispatch_adaptive(u_on, 16)
        same_frame(images(r), want_adaptive, "rm_dispatch_adaptive")
        assert r.accum_samples() == 4
        bits_equal(r.read_accum(), S, "the sum after the other dispatches")
        r.dispatch_accumulate(u, a7)  # continues as if they had not happened
        same_frame(images(r), want_both, "the next accumulating call")
        assert r.accum_samples() == 11 and (r.read_accum()[..., 3] == np.float32(11)).all()


# ---- 6. one colour output -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_single_output_contexts(rm, gpu, name):
    W, H = 37, 23
    u = main_u(rm, 1)
    pats = refine_patterns(rm)
    calls = (pats["grid3"], pats["jitter1"], pats["abs7"])  # three rounds, the one-sample kernel, two rounds

    def run(r):
        for p in calls:
            r.dispatch_accumulate(u, p)
        return r.read_accum()

    with renderer(rm, W, H, scene_of(rm, name)) as r:
        S = run(r)
        want = images(r)
    with renderer(rm, W, H, scene_of(rm, name), outputs=rm.RM_OUT_RGBA8) as r:
        bits_equal(run(r), S, "rgba8 only: sum image")
        assert r.read_rgba8().tobytes() == want[0].tobytes()
    with renderer(rm, W, H, scene_of(rm, name), outputs=rm.RM_OUT_RGBA32F) as r:
        bits_equal(run(r), S, "rgba32f only: sum image")
        np.testing.assert_array_equal(r.read_rgba32f().view(np.uint32), want[1].view(np.uint32))


# ---- 7. the caller's image and stream -------------------------------------------------------------------
def test_caller_output_and_stream(rm, gpu):
    import torch
    W, H = 37, 23
    u = main_u(rm, 1)
    g2, rg = rm.sample_pattern(rm.RM_PATTERN_GRID2), rm.sample_pattern(rm.RM_PATTERN_RGSS)
    with renderer(rm, W, H) as r:
        r.dispatch_accumulate(u, g2)
        want_4 = r.read_rgba8()
        r.dispatch_accumulate(u, rg)
        want_8 = r.read_rgba8()
        assert want_4.tobytes() != want_8.tobytes()
        dev = torch.device("cuda", r.device)
        s, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
        out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
        torch.cuda.synchronize()
        try:
            with torch.cuda.stream(s):
                r.set_stream(s.cuda_stream)
                r.set_output_rgba8(out.data_ptr())
                assert r.output_rgba8_ptr() == out.data_ptr()
                r.dispatch_accumulate(u, g2, restart=True)  # another pattern than the last: its table is uploaded on s
                first = out.clone()
                r.dispatch_accumulate(u, rg)
                r.wait_output(s2.cuda_stream)
                with torch.cuda.stream(s2):
                    second = out.clone()
                s2.synchronize()
            s.synchronize()
            assert first.cpu().numpy().tobytes() == want_4.tobytes()
            assert second.cpu().numpy().tobytes() == want_8.tobytes()
            assert r.read_rgba8().tobytes() == want_8.tobytes()
        finally:
            r.synchronize()
            r.set_output_rgba8(None)
            r.set_stream(None)
        r.dispatch_accumulate(u, g2, restart=True)
        assert r.read_rgba8().tobytes() == want_4.tobytes()


# ---- 8. the sum image: its device pointer and rm_read_accum ----------------------------------------
class DeviceImage:
    """A [H][W][4] float32 device image at `ptr`, for torch.as_tensor."""

    def __init__(self, ptr, H, W):
        self.__cuda_array_interface__ = {"shape": (H, W, 4), "typestr": "<f4", "data": (ptr, False), "version": 2}


def test_device_pointer_and_read_accum(rm, gpu):
    import torch
    W, H = 37, 23
    u = main_u(rm, 1)
    with renderer(rm, W, H) as r:
        ptr = r.accum_ptr()  # allocated on first use, whatever N is
        assert ptr != 0 and ptr % 16 == 0
        r.dispatch_accumulate(u, rm.RM_PATTERN_GRID3)
        r.dispatch_accumulate(u, rm.halton_pattern(9, 1))
        assert r.accum_ptr() == ptr
        dev = torch.device("cuda", r.device)
        s2 = torch.cuda.Stream(device=dev)
        r.wait_output(s2.cuda_stream)
        with torch.cuda.stream(s2):
            got = torch.as_tensor(DeviceImage(ptr, H, W), device=dev).clone()
        s2.synchronize()
        S = r.read_accum()
        bits_equal(got.cpu().numpy(), S, "rm_get_accum against rm_read_accum")
        assert (S[..., 3] == np.float32(10)).all()
        # a caller's shader resolves the frame as rgb / w
        with np.errstate(all="ignore"):
            bits_equal(S[..., :3] / S[..., 3:], r.read_rgba32f()[..., :3], "rgb / w")
        bits_equal(r.read_accum(flip_y=True), S[::-1], "flip_y")
        pitch = W * 16 + 32
        buf = np.full((H, pitch // 4), np.float32(-7.0))
        assert rm.lib().rm_read_accum(r.handle, buf.ctypes.data, pitch, 0) == rm.RM_OK
        bits_equal(buf[:, :W * 4].reshape(H, W, 4), S, "row pitch")
        assert (buf[:, W * 4:] == -7.0).all()
        assert rm.lib().rm_read_accum(r.handle, buf.ctypes.data, W * 16 - 4, 0) == rm.RM_ERR_INVALID


# ---- 9. rm_scene_specialize: the generic table code renders, the same values ----------------------
def test_specialised_context_gives_the_same_values(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 2)
    scene = scene_of(rm, "floor-table")
    pats = refine_patterns(rm)

    def run(r):
        out = []
        for pname in ("grid3", "jitter1", "abs7"):
            r.dispatch_accumulate(u, pats[pname])
            out.append((images(r), r.read_accum()))
        return out

    with renderer(rm, W, H, scene) as r:
        want = run(r)
    with renderer(rm, W, H, scene, specialize=True) as r:
        r.dispatch(u)  # the specialised frame kernel is in use
        for k, ((frame, S), (wframe, wS)) in enumerate(zip(run(r), want)):
            same_frame(frame, wframe, f"specialised, call {k}")
            bits_equal(S, wS, f"specialised, call {k}: sum image")


# ---- 10. timing ------------------------------------------------------------------------------------------------
def test_one_timed_launch_per_call(rm, gpu):
    with renderer(rm, 37, 23) as r:
        r.enable_timing(True)
        _, n0 = r.kernel_time_ms()
        r.dispatch_accumulate(main_u(rm, 1), rm.RM_PATTERN_GRID4)
        ms, n1 = r.kernel_time_ms()
        assert n1 - n0 == 1 and ms > 0.0
        r.dispatch_accumulate(None, rm.halton_pattern(16, 1))  # a new table: the upload is outside the count
        r.dispatch_accumulate(None, rm.halton_pattern(16, 1))
        r.dispatch_accumulate(None, rm.RM_PATTERN_GRID3, restart=True)
        _, n2 = r.kernel_time_ms()
        assert n2 - n1 == 3
        assert r.frame_phases()["render_ms"] > 0.0


# ---- 11. refusals ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["counters", "nshards", "gbuffer", "graph", "ngpus", "communicator"])
def test_refused_contexts(rm, gpu, kind):
    W, H = 64, 48
    u = main_u(rm, 1)
    p = rm.sample_pattern(rm.RM_PATTERN_GRID2)
    L = rm.lib()
    kw = {"counters": dict(counters=True), "nshards": dict(nshards=2, shard=0, row_block=8),
          "gbuffer": dict(outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER), "graph": {},
          "ngpus": dict(ngpus=1, row_block=8), "communicator": dict(row_block=8, shard=0, nshards=1)}[kind]
    with rm.Renderer(W, H, **kw) as r:
        if kind == "communicator":
            r.comm_init(rm.comm_unique_id(), 1, 0)
        if kind == "graph":
            r.graph_enable(True)
            r.graph_dispatch(u)
        else:
            r.dispatch(u)
        before = r.read_rgba8()
        for flags in (0, rm.RM_ACCUM_RESTART):
            assert L.rm_dispatch_accumulate(r.handle, C.byref(p), flags) == rm.RM_ERR_STATE
            assert "rm_dispatch_accumulate" in L.rm_last_error(r.handle).decode()
        # the sum image's pointer is refused on the same contexts, and nothing is written
        ptr = C.c_void_p(0x1234)
        assert L.rm_get_accum(r.handle, C.byref(ptr)) == rm.RM_ERR_STATE
        assert "rm_get_accum" in L.rm_last_error(r.handle).decode() and ptr.value == 0x1234
        assert r.accum_samples() == 0
        assert r.read_rgba8().tobytes() == before.tobytes()
        if kind == "graph":  # and with the graph off again the call works
            r.graph_enable(False)
            r.dispatch_accumulate(u, rm.custom_pattern([0.0], [0.0]))
            assert r.read_rgba8().tobytes() == before.tobytes() and r.accum_samples() == 1


def test_refused_calls_leave_the_sum_alone(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 1)
    L = rm.lib()
    dst = np.full((H, W, 4), np.float32(-7.0))
    with renderer(rm, W, H) as r:
        r.dispatch(u)  # a frame, and still no sum
        assert L.rm_read_accum(r.handle, dst.ctypes.data, 0, 0) == rm.RM_ERR_STATE
        assert "rm_read_accum" in L.rm_last_error(r.handle).decode() and (dst == -7.0).all()
        r.dispatch_accumulate(u, rm.RM_PATTERN_RGSS)
        r.dispatch_accumulate(u, rm.halton_pattern(4, 7))
        before, S = images(r), r.read_accum()
        ok = rm.sample_pattern(rm.RM_PATTERN_GRID3)

        def unchanged(what):
            assert r.accum_samples() == 11, what
            bits_equal(r.read_accum(), S, what)
            same_frame(images(r), before, what)

        assert L.rm_dispatch_accumulate(r.handle, None, 0) == rm.RM_ERR_INVALID
        unchanged("a null pattern")
        for flags in (2, 3, 1 << 31):
            assert L.rm_dispatch_accumulate(r.handle, C.byref(ok), flags) == rm.RM_ERR_INVALID, flags
            msg = L.rm_last_error(r.handle).decode()
            assert "rm_dispatch_accumulate" in msg and "flags" in msg, msg
            unchanged(f"flags {flags}")
        for field, bad, word in (("struct_size", 136, "struct_size"), ("flags", 2, "flags"), ("n", 0, "n must"),
                                 ("n", 17, "n must")):
            p = rm.rm_sample_pattern.from_buffer_copy(ok)
            setattr(p, field, bad)
            for flags in (0, rm.RM_ACCUM_RESTART):
                assert L.rm_dispatch_accumulate(r.handle, C.byref(p), flags) == rm.RM_ERR_INVALID, field
                msg = L.rm_last_error(r.handle).decode()
                assert "rm_dispatch_accumulate" in msg and word in msg, msg
            unchanged(field)
        for v in (float("nan"), float("inf"), 16.5):
            p = rm.rm_sample_pattern.from_buffer_copy(ok)
            p.dy[8] = v
            assert L.rm_dispatch_accumulate(r.handle, C.byref(p), 0) == rm.RM_ERR_INVALID, v
            assert "offset" in L.rm_last_error(r.handle).decode()
            unchanged(f"offset {v}")
        r.accum_reset()
        assert L.rm_read_accum(r.handle, dst.ctypes.data, 0, 0) == rm.RM_ERR_STATE  # N == 0 again
        assert (dst == -7.0).all()
        same_frame(images(r), before, "rm_accum_reset does no device work")
