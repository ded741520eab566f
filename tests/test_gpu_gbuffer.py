"""The fused G-buffer output on the GPU (RM_OUT_GBUFFER, rm_read_gbuffer,
rm_set_output_gbuffer): every pixel's primary hit, written by the
frame kernels themselves.

A record is compared bit for bit as uint32 (a NaN equal to a NaN) with the CPU
oracle's raymarch / get_normal of the pixel's ray and with a RM_TRACE_HIT |
RM_TRACE_NORMAL ray query of the same ray on the same context; the colour images
of a G-buffer context are compared byte for byte with a plain context's.

The pixel's ray (glsl:301-313): uv = (2 p - dims) / dims in float32, and with AA
on the first sample's offset 0.25 / dims added in float32, then castRay.

Main frame: rm_sweep_uniforms(60, 120, 1, aa, 0) at 130 x 67 (several 8x8 and 4x4
tiles, ragged in both directions); its primary rays hit every id {0, 1, 4, 5, 6, 7}
and miss 3,565 pixels with AA off and 3,603 with AA on (the CPU oracle's count).
"""
import ctypes as C

import numpy as np
import pytest

from frames import ALL, renderer
from records import gbuf_rays, oracle_gbuffer, records_equal
from scenes import scene_of
from uniforms import main_u, off_sweep_uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32
W0, H0 = 130, 67
SHAPES = [(130, 67), (37, 23), (1, 1)]
FIELDS = ("t", "id", "normal", "albedo")
HITN = 2  # RM_TRACE_HIT | RM_TRACE_NORMAL
MISSES = {False: 3565, True: 3603}


def miss_record(rm):
    m = np.zeros(1, rm.GBUFFER_DTYPE)
    m["t"], m["id"] = -1.0, -1
    return m[0]


def render_gbuf(rm, u, W, H, scene=None, outputs=ALL, **kw):
    with renderer(rm, W, H, scene, outputs, **kw) as r:
        r.dispatch(u)
        out = {"gbuf": r.read_gbuffer()}
        if outputs & rm.RM_OUT_RGBA8:
            out["rgba8"] = r.read_rgba8()
        if outputs & rm.RM_OUT_RGBA32F:
            out["rgba32f"] = r.read_rgba32f()
        return out


# ---- 1. the colour images are what they are without the bit ---------------------------
@pytest.mark.parametrize("which", ["builtin", "random0", "random1", "floor0"])
def test_colour_untouched(rm, gpu, which):
    scene = scene_of(rm, which)
    with renderer(rm, W0, H0, scene) as plain, renderer(rm, W0, H0, scene, ALL) as g:
        for aa in (False, True):
            for bounces in (0, 2):
                for shadow in (0, 1):
                    u = main_u(rm, bounces, shadow, aa)
                    plain.dispatch(u)
                    g.dispatch(u)
                    what = f"{which} aa{int(aa)} b{bounces} s{shadow}"
                    assert g.read_rgba8().tobytes() == plain.read_rgba8().tobytes(), what
                    np.testing.assert_array_equal(g.read_rgba32f().view(np.uint32),
                                                  plain.read_rgba32f().view(np.uint32), err_msg=what)
                    assert (g.read_gbuffer()["t"] != F32(-1.0)).any(), what


# ---- 2. against the oracle ---------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_against_the_oracle(rm, oracle, gpu, shape, aa):
    W, H = shape
    u = main_u(rm, aa=aa)
    g = render_gbuf(rm, u, W, H)["gbuf"].reshape(-1)
    want = oracle_gbuffer(rm, oracle, u, W, H, aa).reshape(-1)
    miss = want["t"] == F32(-1.0)
    print(f"{W}x{H} aa={aa}: ids {sorted(set(want['id'].tolist()))}, {miss.sum()} misses")
    if shape == (W0, H0):
        assert sorted(set(want["id"].tolist())) == [-1, 0, 1, 4, 5, 6, 7]
        assert miss.sum() == MISSES[aa]
        # (the same condition on the G-buffer itself)
        assert sorted(set(g["id"].tolist())) == [-1, 0, 1, 4, 5, 6, 7] and (g["t"] == F32(-1.0)).any()
    records_equal(g, want, FIELDS, f"{W}x{H} aa={aa} vs oracle")
    assert g[miss].tobytes() == miss_record(rm).tobytes() * int(miss.sum()), "a miss: t -1, id -1, zeros"


# ---- 3. against ray queries ----------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
@pytest.mark.parametrize("which", ["builtin", "random0", "random1", "floor0"])
def test_against_ray_queries(rm, oracle, gpu, which, aa):
    scene = scene_of(rm, which)
    u = main_u(rm, aa=aa)
    for W, H in SHAPES:
        with renderer(rm, W, H, scene, ALL) as r:
            r.dispatch(u)
            g = r.read_gbuffer()
            o, d = gbuf_rays(oracle, u, W, H, aa)
            tr = r.trace(o, d, HITN)
            records_equal(g, tr, FIELDS, f"{which} {W}x{H} aa={aa} vs trace")
            assert not tr["color"].any()
            if not aa:  # the pixel's one ray is the ray rm_pick casts
                for px, py in {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)}:
                    p = np.asarray(r.pick(px, py)).reshape(1)
                    records_equal(g[py:py + 1, px], p, FIELDS, f"{which} pick {px},{py}")


@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
def test_default_table_equals_builtin(rm, gpu, aa):
    u = main_u(rm, 2, aa=aa)
    a = render_gbuf(rm, u, W0, H0)
    b = render_gbuf(rm, u, W0, H0, scene=rm.default_scene())
    records_equal(b["gbuf"], a["gbuf"], FIELDS, "default table vs built-in")
    assert b["rgba8"].tobytes() == a["rgba8"].tobytes()
    np.testing.assert_array_equal(b["rgba32f"].view(np.uint32), a["rgba32f"].view(np.uint32))


# ---- 4. rm_scene_specialize ------------------------------------------------------------------
@pytest.mark.parametrize("which", ["default_table", "random0"])
def test_specialize_changes_nothing(rm, gpu, which):
    scene = scene_of(rm, which)
    u = main_u(rm, 2, aa=True)
    with rm.Renderer(W0, H0, outputs=ALL) as r:
        r.set_scene(scene)
        r.dispatch(u)
        before = (r.read_gbuffer().tobytes(), r.read_rgba8().tobytes(), r.read_rgba32f().tobytes())
        r.specialize_scene(True)
        assert r.scene_kernel_waves() == 0
        r.dispatch(u)
        assert (r.read_gbuffer().tobytes(), r.read_rgba8().tobytes(), r.read_rgba32f().tobytes()) == before
        r.set_scene(scene)  # a table set with the switch on
        assert r.scene_kernel_waves() == 0
        r.dispatch(main_u(rm, 2))
        r.dispatch(u)
        assert (r.read_gbuffer().tobytes(), r.read_rgba8().tobytes(), r.read_rgba32f().tobytes()) == before


# ---- 5. uniforms off the sweep ---------------------------------------------------------------
@pytest.mark.parametrize("i", range(17), ids=[f"case{i}" for i in range(16)] + ["nan_camera"])
def test_off_sweep_uniforms(rm, oracle, gpu, i):
    u, (W, H) = off_sweep_uniforms(rm, i)
    assert (W, H) == (67, 41)
    aa = bool(u.AA)
    with rm.Renderer(W, H, outputs=ALL) as r, rm.Renderer(W, H, outputs=3) as plain:
        r.dispatch(u)
        plain.dispatch(u)
        g = r.read_gbuffer()
        o, d = gbuf_rays(oracle, u, W, H, aa)
        with np.errstate(all="ignore"):
            records_equal(g, r.trace(o, d, HITN), FIELDS, f"case {i} vs trace")
        assert r.read_rgba8().tobytes() == plain.read_rgba8().tobytes()
        assert r.read_rgba32f().tobytes() == plain.read_rgba32f().tobytes()


# ---- 6. shards ---------------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
@pytest.mark.parametrize("which", ["builtin", "random0"])
def test_shards_assemble(rm, gpu, which, aa):
    W, H, R, N = W0, 67, 8, 3
    scene = scene_of(rm, which)
    u = main_u(rm, aa=aa)
    full = render_gbuf(rm, u, W, H, scene=scene)["gbuf"]
    cap = C.c_int32(0)
    rm.lib().rm_shard_rows(H, R, 0, N, 0, None, C.byref(cap))
    got = np.zeros_like(full)
    seen = np.zeros(H, bool)
    npad = 0
    for s in range(N):
        part = render_gbuf(rm, u, W, H, scene=scene, row_block=R, shard=s, nshards=N)["gbuf"]
        assert part.shape == (cap.value, W)
        for lr in range(cap.value):
            gr = rm.lib().rm_shard_to_global(H, R, 0, N, s, lr)
            if gr >= 0:
                got[gr] = part[lr]
                seen[gr] = True
            else:  # a padding row
                assert part[lr].tobytes() == miss_record(rm).tobytes() * W, (s, lr)
                npad += 1
    assert seen.all() and npad == N * cap.value - H and npad > 0
    assert got.tobytes() == full.tobytes()


# ---- 7. device interop --------------------------------------------------------------------------
def test_interop(rm, gpu):
    import torch
    W, H = 37, 23
    u = main_u(rm)
    ref = render_gbuf(rm, u, W, H)["gbuf"]
    lib = rm.lib()
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.cuda.Stream(device=dev)
    with rm.Renderer(W, H, outputs=ALL) as r:
        own = r.output_gbuffer_ptr()
        assert own and own % 16 == 0
        try:
            with torch.cuda.stream(s):
                r.set_stream(s.cuda_stream)
                buf = torch.full((H * W * 8 + 8,), -7.25, dtype=torch.float32, device=dev)
                assert buf.data_ptr() % 16 == 0
                assert lib.rm_set_output_gbuffer(r.handle, buf.data_ptr() + 8) == rm.RM_ERR_INVALID
                assert lib.rm_last_error(r.handle)
                assert r.output_gbuffer_ptr() == own
                r.set_output_gbuffer(buf.data_ptr())
                assert r.output_gbuffer_ptr() == buf.data_ptr()
                r.dispatch(u)
                back = buf.cpu()  # ordered after the dispatch on the same stream
                h = back.numpy()
                assert (h[H * W * 8:] == F32(-7.25)).all(), "the sentinel after the last record"
                assert h[:H * W * 8].tobytes() == ref.tobytes()
                # readback reads the caller's image: tight, flipped, pitched
                assert r.read_gbuffer().tobytes() == ref.tobytes()
                assert r.read_gbuffer(flip_y=True).tobytes() == ref[::-1].tobytes()
                pitch = W * 32 + 48
                out = np.zeros((H, pitch), np.uint8)
                assert lib.rm_read_gbuffer(r.handle, out.ctypes.data, pitch, 1) == rm.RM_OK
                assert out[:, :W * 32].tobytes() == ref[::-1].tobytes() and not out[:, W * 32:].any()
                assert lib.rm_read_gbuffer(r.handle, out.ctypes.data, W * 32 - 4, 0) == rm.RM_ERR_INVALID
                # rm_wait_output orders another stream after the G-buffer's writes
                s2 = torch.cuda.Stream(device=dev)
                buf.fill_(0.0)
                r.dispatch(u)
                r.wait_output(s2.cuda_stream)
                with torch.cuda.stream(s2):
                    again = buf.clone()
                s2.synchronize()
                assert again.cpu().numpy()[:H * W * 8].tobytes() == ref.tobytes()
                # NULL restores the context's own buffer
                r.set_output_gbuffer(None)
                assert r.output_gbuffer_ptr() == own
                buf.fill_(3.0)
                r.dispatch(u)
                assert r.read_gbuffer().tobytes() == ref.tobytes()
                assert (buf.cpu().numpy() == F32(3.0)).all(), "the caller's buffer is left alone"
        finally:
            r.synchronize()
            r.set_stream(None)


# ---- 8. refusals ---------------------------------------------------------------------------------
def test_refusals(rm, gpu):
    lib = rm.lib()
    G = rm.RM_OUT_GBUFFER
    for kw in (dict(counters=True), dict(ngpus=1), dict(ngpus=2)):
        with pytest.raises(rm.RMError) as e:
            rm.Renderer(32, 16, outputs=G | rm.RM_OUT_RGBA8, **kw)
        assert e.value.code == rm.RM_ERR_INVALID and "RM_OUT_GBUFFER" in str(e.value), kw
    u = main_u(rm)
    px = np.zeros((16, 32), rm.GBUFFER_DTYPE)
    with rm.Renderer(32, 16, outputs=G | rm.RM_OUT_RGBA8) as r:
        h = r.handle
        assert lib.rm_read_gbuffer(h, px.ctypes.data, 0, 0) == rm.RM_ERR_STATE  # nothing dispatched
        assert lib.rm_last_error(h)
        assert not px.tobytes().strip(b"\0")
        frames = (rm.rm_uniforms * 2)(u, u)
        ident = C.create_string_buffer(rm.COMM_ID_BYTES)
        for what, call in (("rm_dispatch_frames", lambda: lib.rm_dispatch_frames(h, frames, 2)),
                           ("rm_graph_enable", lambda: lib.rm_graph_enable(h, 1)),
                           ("rm_graph_dispatch", lambda: lib.rm_graph_dispatch(h)),
                           ("rm_comm_init", lambda: lib.rm_comm_init(h, ident, 2, 0))):
            assert call() == rm.RM_ERR_STATE, what
            msg = lib.rm_last_error(h).decode()
            assert what in msg and "G-buffer" in msg, (what, msg)
        assert lib.rm_read_gbuffer(h, None, 0, 0) == rm.RM_ERR_INVALID
        # the context still renders afterwards
        r.dispatch(u)
        assert r.read_gbuffer().tobytes() == render_gbuf(rm, u, 32, 16)["gbuf"].tobytes()
    with rm.Renderer(32, 16, outputs=3) as r:  # without the bit
        r.dispatch(u)
        assert lib.rm_read_gbuffer(r.handle, px.ctypes.data, 0, 0) == rm.RM_ERR_STATE
        assert lib.rm_last_error(r.handle)
        assert lib.rm_set_output_gbuffer(r.handle, None) == rm.RM_ERR_STATE
        p = C.c_void_p(1)
        assert lib.rm_get_output_gbuffer(r.handle, C.byref(p)) == rm.RM_OK and not p.value
        assert lib.rm_get_output_gbuffer(r.handle, None) == rm.RM_ERR_INVALID
        assert not px.tobytes().strip(b"\0")


# ---- 9. the G-buffer alone --------------------------------------------------------------------------
@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
@pytest.mark.parametrize("which", ["builtin", "random0"])
def test_gbuffer_alone(rm, gpu, which, aa):
    scene = scene_of(rm, which)
    u = main_u(rm, 2, aa=aa)
    want = render_gbuf(rm, u, W0, H0, scene=scene)["gbuf"]
    with renderer(rm, W0, H0, scene, rm.RM_OUT_GBUFFER) as r:
        r.dispatch(u)
        assert r.read_gbuffer().tobytes() == want.tobytes()
        with pytest.raises(rm.RMError) as e:
            r.read_rgba8()
        assert e.value.code == rm.RM_ERR_STATE
        with pytest.raises(rm.RMError):
            r.read_rgba32f()
