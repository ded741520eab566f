"""Ray queries on the GPU (rm_trace_rays, rm_trace_rays_device, rm_pick).

Expected values are the oracle's single-function entry points called per ray
(rmo_raymarch, rmo_get_normal, rmo_softshadow, rmo_render_ray, rmo_cast_ray).
Geometry (t, id, material, albedo, normals, shadow factors) is compared bit for
bit as uint32, a NaN equal to a NaN; colours within 2e-6 (DESIGN §5's RGBA32F bar:
pow is the only operation that differs), NaN masks equal.

The ray sets (aimed, random, edge), the comparisons and the oracle per ray are
tests/records.py's; uniforms: the defaults with iTime = 1 unless a test says otherwise.
"""
import ctypes as C

import numpy as np
import pytest

from records import (F32, FLAG_SETS, INF, SETS, aimed_rays, bits_equal, colors_close, edge_rays, hit_fields_equal,
                     oracle_colors, oracle_march, oracle_normals, pixel_rays, random_rays, zeros)
from scenes import scene_of
from uniforms import default_u

pytestmark = pytest.mark.gpu

AIMED_IDS = [0, 1, 4, 5, 6, 7, -1]  # of records.aimed_rays()


@pytest.fixture(scope="module")
def ctx(rm, gpu):
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F) as r:
        yield r


# ---- 0. the sets cover the scene (a condition on the oracle's answers alone) -----------
def test_ray_sets_cover_the_scene(rm, oracle, gpu):
    u = default_u(rm)
    o, d = aimed_rays()
    assert list(oracle_march(rm, oracle, u, o, d, False)["id"]) == AIMED_IDS
    o, d = random_rays()
    ids = oracle_march(rm, oracle, u, o, d, False)["id"]
    assert set(ids.tolist()) == {-1, 0, 1, 4, 5, 6, 7}, np.unique(ids, return_counts=True)
    assert [int((ids == k).sum()) for k in (-1, 0, 1, 4, 5, 6, 7)] == [477, 8, 13, 7, 2, 7, 486]
    refl = oracle_march(rm, oracle, u, o, d, True)
    assert int((refl["id"] == -1).sum()) == 489 and int((refl["id"] != ids).sum()) == 12
    o, d = edge_rays()
    e = oracle_march(rm, oracle, u, o, d, False)
    assert (e["id"][5], float(e["t"][5])) == (7, 5.5)  # (1e20, 0, 0) going down: the floor
    assert e["id"][0] == -1                           # rd = 0: a miss at the step cap


# ---- 1. HIT and HIT | REFLECTED --------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("reflected", [False, True], ids=["raymarch", "reflected"])
def test_hit_bit_exact(rm, oracle, ctx, name, reflected):
    u = default_u(rm)
    o, d = SETS[name]()
    ctx.set_uniforms(u)
    got = ctx.trace(o, d, rm.RM_TRACE_REFLECTED if reflected else rm.RM_TRACE_HIT)
    hit_fields_equal(got, oracle_march(rm, oracle, u, o, d, reflected), name)
    assert zeros(got["normal"]) and zeros(got["color"])


# ---- 2. scaled directions: t is the parameter along rd as given ------------------------
@pytest.mark.parametrize("scale", [1e-3, 0.5, 3.0, 1e3])
def test_scaled_directions(rm, oracle, ctx, scale):
    u = default_u(rm)
    o, d = random_rays()
    d = d * F32(scale)
    assert d.dtype == F32
    ctx.set_uniforms(u)
    for reflected in (False, True):
        got = ctx.trace(o, d, rm.RM_TRACE_REFLECTED if reflected else rm.RM_TRACE_HIT)
        hit_fields_equal(got, oracle_march(rm, oracle, u, o, d, reflected), f"x{scale} refl={reflected}")


# ---- 3. NORMAL -------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("reflected", [False, True], ids=["raymarch", "reflected"])
def test_normals_bit_exact(rm, oracle, ctx, name, reflected):
    u = default_u(rm)
    o, d = SETS[name]()
    ctx.set_uniforms(u)
    got = ctx.trace(o, d, rm.RM_TRACE_NORMAL | (rm.RM_TRACE_REFLECTED if reflected else 0))
    want = oracle_march(rm, oracle, u, o, d, reflected)
    hit_fields_equal(got, want, name)
    bits_equal(got["normal"], oracle_normals(oracle, u, o, d, want["t"]), f"{name} normal")
    assert zeros(got["normal"][want["t"] == F32(-1.0)]) and zeros(got["color"])


# ---- 4. SHADOW -------------------------------------------------------------------------
def shadow_rays(rm):
    o, d = random_rays()
    rng = np.random.default_rng(2)
    p = rng.uniform([-30, -5.5, -35], [20, -3.5, 20], (1000, 3)).astype(F32)
    light = np.array(list(default_u(rm).light.position), F32)
    return np.concatenate([o, p]), np.concatenate([d, light - p])  # rd = light - point, unnormalised


@pytest.mark.parametrize("mode", [0, 1], ids=["soft", "hard"])
def test_shadow_bit_exact(rm, oracle, ctx, mode):
    u = default_u(rm, shadow_mode=mode)
    o, d = shadow_rays(rm)
    eo, ed = edge_rays()
    o, d = np.concatenate([o, eo]), np.concatenate([d, ed])
    k = INF if mode == rm.RM_SHADOW_HARD else 2.0
    want = np.array([oracle.softshadow(u, o[i], d[i], k)[0] for i in range(len(o))], F32)
    assert len(np.unique(want[~np.isnan(want)])) > (2 if mode == 0 else 1), "the set exercises the shadow"
    ctx.set_uniforms(u)
    got = ctx.trace(o, d, rm.RM_TRACE_SHADOW)
    bits_equal(got["t"], want, f"softshadow k={k}")
    for f in ("id", "material", "albedo", "normal", "color"):
        assert zeros(got[f]), f


# ---- 5. SHADE --------------------------------------------------------------------------
@pytest.mark.parametrize("bounces", [0, 2, 5])
@pytest.mark.parametrize("mode", [0, 1], ids=["soft", "hard"])
def test_shade(rm, oracle, ctx, bounces, mode):
    u = default_u(rm, bounces, mode)
    ctx.set_uniforms(u)
    for name in sorted(SETS):
        o, d = SETS[name]()
        got = ctx.trace(o, d, rm.RM_TRACE_SHADE)
        hit_fields_equal(got, oracle_march(rm, oracle, u, o, d, False), name)
        colors_close(got["color"], oracle_colors(oracle, u, o, d), f"{name} b{bounces} s{mode}")
        assert zeros(got["normal"])


# ---- 6. ray counts ---------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_ray_counts(rm, ctx, n):
    import torch
    u = default_u(rm, 1)
    o, d = random_rays()
    ctx.set_uniforms(u)
    flags = rm.RM_TRACE_SHADE | rm.RM_TRACE_NORMAL
    full = ctx.trace(o, d, flags)
    lib = rm.lib()
    # host path: a buffer with room for 64 more records, filled with a sentinel
    buf = np.full((n + 64) * 12, 0xABABABAB, np.uint32)
    rc = lib.rm_trace_rays(ctx.handle, o.ctypes.data, d.ctypes.data, n, flags, buf.ctypes.data)
    assert rc == rm.RM_OK
    assert (buf[n * 12:] == 0xABABABAB).all()
    np.testing.assert_array_equal(buf[:n * 12], full[:n].view(np.uint32).reshape(-1))
    # device path: the kernel's own stores stop at n
    dev = torch.device("cuda", torch.cuda.current_device())
    to, td = torch.from_numpy(o).to(dev), torch.from_numpy(d).to(dev)
    hits = torch.full(((n + 64), 12), -7.25, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    rc = lib.rm_trace_rays_device(ctx.handle, to.data_ptr(), td.data_ptr(), n, flags, hits.data_ptr())
    assert rc == rm.RM_OK
    ctx.synchronize()
    h = hits.cpu().numpy()
    assert (h[n:] == F32(-7.25)).all()
    np.testing.assert_array_equal(h[:n].view(np.uint32).reshape(-1), full[:n].view(np.uint32).reshape(-1))


# ---- 7. frame consistency --------------------------------------------------------------
def frame_equals_trace(rm, oracle, r, u, scene=None):
    """The context's own dispatch (RGBA32F) equals a SHADE trace of every pixel's ray."""
    W, H = r.width, r.height
    r.dispatch(u)
    img = r.read_rgba32f()
    o, d = pixel_rays(oracle, u, W, H)
    got = r.trace(o, d, rm.RM_TRACE_SHADE)
    bits_equal(got["color"].reshape(H, W, 3), img[..., :3], "trace vs frame")
    assert (img[..., 3] == 1.0).all()
    return got, img


def test_frame_consistency(rm, oracle, ctx):
    u = rm.sweep_uniforms(60, 120, 1, False, 0)
    got, _ = frame_equals_trace(rm, oracle, ctx, u)
    assert len(set(got["id"].tolist())) >= 3, "the frame shows several objects"


# ---- 8. rm_pick ------------------------------------------------------------------------
def test_pick(rm, oracle, ctx):
    u = rm.sweep_uniforms(60, 120, 1, False, 0)
    ctx.set_uniforms(u)
    W, H = ctx.width, ctx.height
    o, d = pixel_rays(oracle, u, W, H)
    ref = ctx.trace(o, d, rm.RM_TRACE_HIT | rm.RM_TRACE_NORMAL).reshape(H, W)
    for px, py in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)]:
        got = ctx.pick(px, py)
        assert got.tobytes() == ref[py, px].tobytes(), (px, py, got, ref[py, px])
    hit = rm.rm_ray_hit()
    for px, py in [(-1, 0), (0, -1), (W, 0), (0, H), (1 << 30, 1 << 30)]:
        assert rm.lib().rm_pick(ctx.handle, px, py, C.byref(hit)) == rm.RM_ERR_INVALID, (px, py)
    assert rm.lib().rm_pick(ctx.handle, 0, 0, None) == rm.RM_ERR_INVALID


# ---- 9. tables -------------------------------------------------------------------------
def test_default_table_equals_builtin(rm, ctx, gpu):
    u = default_u(rm, 2)
    ro, rd = random_rays()
    eo, ed = edge_rays()
    o, d = np.concatenate([ro, eo]), np.concatenate([rd, ed])
    ctx.set_uniforms(u)
    want = {f: ctx.trace(o, d, f) for f in FLAG_SETS}
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA32F) as t:
        t.set_scene(rm.default_scene())
        t.set_uniforms(u)
        before = {}
        for f in FLAG_SETS:
            before[f] = t.trace(o, d, f)
            bits_equal(before[f].view(np.uint32).reshape(-1, 12), want[f].view(np.uint32).reshape(-1, 12),
                       f"flags {f}")
        # with the table's specialised kernels on, queries still trace through the generic code
        t.specialize_scene(True)
        for f in FLAG_SETS:
            assert t.trace(o, d, f).tobytes() == before[f].tobytes(), f"specialised, flags {f}"
        t.dispatch(u)  # (and frames render with the specialised kernels next to them)
        assert t.trace(o, d, 4).tobytes() == before[4].tobytes()


@pytest.mark.parametrize("which", ["random0", "random1", "random2", "random3", "floor0"])
def test_tables_against_their_frames_and_the_oracle(rm, oracle, gpu, which):
    scene = scene_of(rm, which)
    u = rm.sweep_uniforms(60, 120, 1, False, 0)
    W, H = 37, 23
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA32F) as t:
        t.set_scene(scene)
        got, _ = frame_equals_trace(rm, oracle, t, u)
    ref = oracle.render(u, W, H, scene=scene, want_counts=False)["rgba32f"]
    colors_close(got["color"].reshape(H, W, 3), ref[..., :3], which)


# ---- 10. the device path ---------------------------------------------------------------
def test_device_path(rm, ctx):
    import torch
    u = default_u(rm, 1)
    ro, rd = random_rays()
    eo, ed = edge_rays()
    o, d = np.concatenate([ro, eo]), np.concatenate([rd, ed])
    ctx.set_uniforms(u)
    flags = rm.RM_TRACE_SHADE | rm.RM_TRACE_NORMAL
    host = ctx.trace(o, d, flags)
    ctx.dispatch(u)
    img = ctx.read_rgba32f()
    dev = torch.device("cuda", torch.cuda.current_device())
    s = torch.cuda.Stream(device=dev)
    try:
        with torch.cuda.stream(s):
            ctx.set_stream(torch.cuda.current_stream().cuda_stream)
            to = torch.from_numpy(o).to(dev)
            td = torch.from_numpy(d).to(dev)
            ctx.dispatch(u)
            hits = ctx.trace(to, td, flags)  # asynchronous, on torch's current stream
            assert hits.shape == (len(o), 12) and hits.dtype == torch.float32 and hits.device == to.device
            back = hits.cpu()  # ordered after the trace on the same stream
        got = back.numpy().view(np.uint32)
        np.testing.assert_array_equal(got, host.view(np.uint32).reshape(-1, 12))
        # the image dispatched before the trace reads back unchanged after it
        np.testing.assert_array_equal(ctx.read_rgba32f().view(np.uint32), img.view(np.uint32))
        with pytest.raises(ValueError):
            ctx.trace(to[:, :2], td[:, :2])
    finally:
        ctx.synchronize()
        ctx.set_stream(None)


# ---- 11. validation --------------------------------------------------------------------
def test_validation(rm, oracle, ctx):
    lib = rm.lib()
    u = rm.sweep_uniforms(60, 120, 1, False, 0)
    ctx.set_uniforms(u)
    o, d = aimed_rays()
    hits = np.zeros(len(o) + 1, rm.RAY_HIT_DTYPE)
    po, pd, ph, n = o.ctypes.data, d.ctypes.data, hits.ctypes.data, len(o)
    INV = rm.RM_ERR_INVALID
    for fn in (lib.rm_trace_rays, lib.rm_trace_rays_device):
        assert fn(ctx.handle, None, pd, n, 0, ph) == INV
        assert fn(ctx.handle, po, None, n, 0, ph) == INV
        assert fn(ctx.handle, po, pd, n, 0, None) == INV
        assert fn(ctx.handle, po, pd, -1, 0, ph) == INV
        assert fn(ctx.handle, po, pd, 1 << 31, 0, ph) == INV
        for flags in (16, 1 << 31, 8 | 1, 8 | 2, 8 | 4, 4 | 1, 4 | 2 | 1):
            assert fn(ctx.handle, po, pd, n, flags, ph) == INV, flags
        assert fn(ctx.handle, None, None, 0, 0, None) == rm.RM_OK  # n == 0: nothing read or written
        assert lib.rm_last_error(ctx.handle)
    assert lib.rm_trace_rays_device(ctx.handle, po, pd, n, 0, ph // 16 * 16 + 4) == INV  # misaligned hits_dev
    assert not hits.tobytes().strip(b"\0"), "a refused call writes nothing"
    with rm.Renderer(32, 16, ngpus=1) as m:  # a multi-device context: out of scope
        assert lib.rm_trace_rays(m.handle, po, pd, n, 0, ph) == rm.RM_ERR_STATE
        assert lib.rm_trace_rays_device(m.handle, po, pd, n, 0, ph) == rm.RM_ERR_STATE
        assert lib.rm_pick(m.handle, 0, 0, C.cast(ph, C.POINTER(rm.rm_ray_hit))) == rm.RM_ERR_STATE
    # the context still renders, and traces, correctly afterwards
    frame_equals_trace(rm, oracle, ctx, u)
    hit_fields_equal(ctx.trace(o, d), oracle_march(rm, oracle, u, o, d, False), "after the refusals")


def test_counting_context_and_timing(rm, oracle, gpu):
    """A context with cfg.counters traces with the production code and leaves its
    counters alone; with timing on a trace launch is bracketed like a render launch."""
    u = default_u(rm, 1)
    o, d = aimed_rays()
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA32F, counters=True) as r:
        r.dispatch(u)
        cnt = r.counters()
        got = r.trace(o, d, rm.RM_TRACE_SHADE)
        assert r.counters() == cnt
        hit_fields_equal(got, oracle_march(rm, oracle, u, o, d, False), "counting context")
        r.synchronize()
        r.kernel_time_ms(reset=True)
        r.enable_timing(True)
        r.trace(o, d)
        r.trace(o, d, rm.RM_TRACE_SHADOW)
        ms, launches = r.kernel_time_ms()
        assert launches == 2 and ms > 0.0
