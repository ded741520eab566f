"""SDF field queries on the GPU (rm_sdf_points, rm_sdf_points_device, rm_sdf_grid,
rm_sdf_grid_device).

Expected values: for the built-in scene the oracle's rmo_sdf / rmo_get_normal per
point; for runtime tables tests/sdf_model.py, the numpy restatement of the
oracle's table sdf that tests/test_sdf_model.py pins to the oracle.  Every field is
compared bit for bit as uint32, a NaN equal to a NaN.  Uniforms: the defaults with
iTime = 1 unless a test says otherwise.
"""
import ctypes as C

import numpy as np
import pytest

import sdf_model as M
from grids import desc, grid_points
from records import bits_equal, pixel_rays, records_equal, zeros
from scenes import random_scene, scene_of
from uniforms import default_u

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN, INF = float("nan"), float("inf")
FIELDS = ("t", "id", "material", "albedo", "normal", "color")


def all_points():
    return np.concatenate([M.seeded_points(), M.edge_points()])


@pytest.fixture(scope="module")
def ctx(rm, gpu):
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F) as r:
        yield r


# ---- 1. the seeded set against the oracle ----------------------------------------------
@pytest.mark.parametrize("itime", [1.0, 0.0, 4.5])
def test_seeded_points_bit_exact(rm, oracle, ctx, itime):
    u = default_u(rm, itime=itime)
    pts = M.seeded_points()
    want = M.oracle_records(rm, oracle, u, pts, normal=True)
    if itime == 1.0:  # the set's coverage, a condition on the oracle's answers alone
        assert [int((want["id"] == k).sum()) for k in (0, 1, 4, 5, 6, 7)] == [208, 181, 179, 157, 157, 1118]
        assert int((want["t"] < 0).sum()) == 186
    ctx.set_uniforms(u)
    got = ctx.sdf(pts, rm.RM_SDF_NORMAL)
    records_equal(got, want, FIELDS, f"NORMAL iTime {itime}")
    got = ctx.sdf(pts)
    records_equal(got, M.oracle_records(rm, oracle, u, pts), FIELDS, f"VALUE iTime {itime}")
    assert zeros(got["normal"]) and zeros(got["color"])


# ---- 2. edge points: fast and literal lanes in one wave --------------------------------
@pytest.mark.parametrize("itime", [1.0, 4.5])
def test_edge_points_bit_exact(rm, oracle, ctx, itime):
    u = default_u(rm, itime=itime)
    pts = M.edge_points()
    want = M.oracle_records(rm, oracle, u, pts, normal=True)
    assert np.isnan(want["normal"][[14, 15]]).all(), "zero gradient far from the origin: a NaN normal"
    assert np.isnan(want["t"][[3, 5]]).all() and (want["id"][[3, 5]] == 7).all(), "a NaN distance: the last entry"
    ctx.set_uniforms(u)
    records_equal(ctx.sdf(pts, rm.RM_SDF_NORMAL), want, FIELDS, "edge NORMAL")
    records_equal(ctx.sdf(pts), M.oracle_records(rm, oracle, u, pts), FIELDS, "edge VALUE")


# ---- 3. counts -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 130])
def test_point_counts(rm, ctx, n):
    import torch
    pts = all_points()[1880:]  # 120 seeded points, then the 16 edge points: n = 130 reaches them
    assert len(pts) == 136
    ctx.set_uniforms(default_u(rm))
    lib = rm.lib()
    for flags in (rm.RM_SDF_VALUE, rm.RM_SDF_NORMAL):
        full = ctx.sdf(pts, flags)
        assert zeros(full["color"]) and (flags or zeros(full["normal"]))
        want = full[:n].view(np.uint32).reshape(-1)
        buf = np.full((n + 64) * 12, 0xABABABAB, np.uint32)
        assert lib.rm_sdf_points(ctx.handle, pts.ctypes.data, n, flags, buf.ctypes.data) == rm.RM_OK
        assert (buf[n * 12:] == 0xABABABAB).all()
        np.testing.assert_array_equal(buf[:n * 12], want)
        dev = torch.device("cuda", torch.cuda.current_device())
        tp = torch.from_numpy(pts).to(dev)
        out = torch.full(((n + 64), 12), -7.25, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        assert lib.rm_sdf_points_device(ctx.handle, tp.data_ptr(), n, flags, out.data_ptr()) == rm.RM_OK
        ctx.synchronize()
        h = out.cpu().numpy()
        assert (h[n:] == F32(-7.25)).all()
        np.testing.assert_array_equal(h[:n].view(np.uint32).reshape(-1), want)


# ---- 4. tables -------------------------------------------------------------------------
def test_default_table_equals_builtin(rm, ctx, gpu):
    pts = all_points()
    ctx.set_uniforms(default_u(rm))
    with rm.Renderer(37, 23) as t:
        t.set_scene(rm.default_scene())
        t.set_uniforms(default_u(rm))
        for flags in (rm.RM_SDF_VALUE, rm.RM_SDF_NORMAL):
            want = ctx.sdf(pts, flags)
            got = t.sdf(pts, flags)
            records_equal(got, want, FIELDS, f"default table, flags {flags}")
            t.specialize_scene(True)  # queries still run the generic table code
            assert t.sdf(pts, flags).tobytes() == got.tobytes()
            t.specialize_scene(False)


@pytest.mark.parametrize("which", ["random0", "random1", "random2", "random3", "floor0", "big30"])
def test_tables_against_the_model(rm, gpu, which):
    scene = scene_of(rm, which)
    assert which != "big30" or len(scene) == 30
    pts = all_points()
    with rm.Renderer(37, 23) as t:
        t.set_scene(scene)
        t.set_uniforms(default_u(rm))
        want = M.sdf_records(rm, scene, 1.0, pts, normal=True)
        got = t.sdf(pts, rm.RM_SDF_NORMAL)
        records_equal(got, want, FIELDS, f"{which} NORMAL")
        val = t.sdf(pts)
        records_equal(val, M.sdf_records(rm, scene, 1.0, pts), FIELDS, f"{which} VALUE")
        # rm_scene_specialize on: which code a query runs depends on the context having a
        # table, not on the table, so the switch is thrown where the compile it starts is
        # short (the random tables' takes 15-20 s each; the default table's is in the test above)
        if which in ("floor0", "big30"):
            t.specialize_scene(True)
            assert t.sdf(pts, rm.RM_SDF_NORMAL).tobytes() == got.tobytes(), "unchanged with rm_scene_specialize on"
            assert t.sdf(pts).tobytes() == val.tobytes()


@pytest.mark.parametrize("order", [(11, 12), (12, 11)])
def test_tie_goes_to_the_later_entry(rm, gpu, order):
    scene = [rm.primitive(rm.PRIM_SPHERE, (1.0, 0.5, -3.0), (2.0,), (0.2, 0.4, 0.6), id=i) for i in order]
    scene.append(rm.primitive(rm.PRIM_PLANE, (0.0, 0.0, 0.0), (0.0, 1.0, 0.0, 5.5), (0.5, 0.5, 0.5), id=7,
                              material=0.0, paint=1))
    pts = np.random.default_rng(3).uniform([-6, -5, -10], [8, 6, 4], (500, 3)).astype(F32)
    want = M.sdf_records(rm, scene, 1.0, pts)
    near = want["id"] != 7
    assert near.sum() > 100 and (want["id"][near] == order[1]).all()
    with rm.Renderer(37, 23) as t:
        t.set_scene(scene)
        t.set_uniforms(default_u(rm))
        got = t.sdf(pts)
        records_equal(got, want, FIELDS, f"tie {order}")
        dist, ids = t.sdf_grid((-6, -5, -10), (0.5, 0.5, 0.5), (28, 22, 28), ids=True)
        gp = grid_points((-6, -5, -10), (0.5, 0.5, 0.5), (28, 22, 28))
        gw = M.sdf_records(rm, scene, 1.0, gp)
        bits_equal(dist.reshape(-1), gw["t"], "tie grid dist")
        bits_equal(ids.reshape(-1), gw["id"], "tie grid ids")
        assert order[0] not in set(ids.reshape(-1).tolist())


# ---- 5. consistency with ray queries ---------------------------------------------------
@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
def test_hit_points_of_a_trace(rm, oracle, gpu, table):
    u = rm.sweep_uniforms(60, 120, 1, False, 0)
    W, H = 37, 23
    o, d = pixel_rays(oracle, u, W, H)
    with rm.Renderer(W, H) as r:
        if table:
            r.set_scene(random_scene(rm, 1))
        r.set_uniforms(u)
        hits = r.trace(o, d, rm.RM_TRACE_HIT | rm.RM_TRACE_NORMAL)
        hit = hits["t"] != F32(-1.0)
        assert hit.sum() > 200
        t = hits["t"][hit]
        p = o[hit] + d[hit] * t[:, None]  # float32: a multiply, then an add
        assert p.dtype == F32
        got = r.sdf(p, rm.RM_SDF_NORMAL)
    for f in ("id", "material", "albedo", "normal"):
        bits_equal(got[f], hits[f][hit], f"trace vs sdf {f}")
    assert (got["t"] < F32(1e-6) * t).all()


# ---- 6. grids --------------------------------------------------------------------------
def expected_grid(rm, oracle, u, scene, pts):
    """(dist, ids) by the oracle (the built-in scene, small grids) or the model."""
    if scene is None and len(pts) <= 4096:
        w = M.oracle_records(rm, oracle, u, pts)
    else:
        w = M.sdf_records(rm, scene if scene is not None else rm.default_scene(), u.iTime, pts)
    return w["t"], w["id"]


GRIDS = [((-30.0, -6.0, -34.0), (7.5, 6.0, 12.0), (1, 1, 1)),
         ((-30.0, -6.0, -34.0), (11.0, 6.0, 40.0), (5, 3, 2)),
         ((-10.0, -6.0, -14.0), (3.5, 4.0, 6.0), (4, 4, 4)),
         ((-30.0, -6.0, -34.0), (6.0, 3.0, 11.0), (9, 6, 5)),
         ((-32.0, 0.5, -10.0), (0.8, 1.0, 1.0), (65, 1, 1)),
         ((-32.0, -5.0, -10.0), (0.4, 5.5, 1.0), (131, 2, 1)),
         ((-5.0, -7.0, -10.0), (1.0, 0.0003, 1.0), (1, 70000, 1)),   # past the 65,535 launch-grid limits
         ((-5.0, 0.0, -36.0), (1.0, 1.0, 0.0007), (1, 1, 70000)),
         ((-30.0, -6.0, -34.0), (0.0, 3.0, 11.0), (9, 6, 5)),        # a step of 0
         ((22.0, 12.0, 16.0), (-6.0, -3.0, -11.0), (9, 6, 5)),       # negative steps
         ((NAN, -6.0, -34.0), (6.0, 3.0, 11.0), (9, 6, 5)),          # a NaN origin
         ((-30.0, INF, -34.0), (6.0, 3.0, 1e38), (8, 3, 5))]         # infinite coordinates, 16-byte stores


@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
@pytest.mark.parametrize("g", range(len(GRIDS)))
def test_grids(rm, oracle, gpu, g, table):
    origin, step, dims = GRIDS[g]
    u = default_u(rm)
    scene = random_scene(rm, 1) if table else None
    pts = grid_points(origin, step, dims)
    with rm.Renderer(37, 23) as r:
        if table:
            r.set_scene(scene)
        r.set_uniforms(u)
        dist, ids = r.sdf_grid(origin, step, dims, ids=True)
        assert dist.shape == ids.shape == (dims[2], dims[1], dims[0])
        rec = r.sdf(pts)
        bits_equal(dist.reshape(-1), rec["t"], "grid vs points: dist")
        bits_equal(ids.reshape(-1), rec["id"], "grid vs points: ids")
        wd, wi = expected_grid(rm, oracle, u, scene, pts)
        bits_equal(dist.reshape(-1), wd, "grid dist")
        bits_equal(ids.reshape(-1), wi, "grid ids")
        # dist only, ids only
        only = r.sdf_grid(origin, step, dims)
        assert only.tobytes() == dist.tobytes()
        i2 = np.full(ids.shape, -99, np.int32)
        assert rm.lib().rm_sdf_grid(r.handle, C.byref(desc(rm, origin, step, dims)), None, i2.ctypes.data) == rm.RM_OK
        assert i2.tobytes() == ids.tobytes()


def test_zero_dims_write_nothing(rm, ctx):
    lib = rm.lib()
    dist, ids = np.full(8, -7.25, F32), np.full(8, -99, np.int32)
    for dims in [(0, 2, 2), (2, 0, 2), (2, 2, 0), (0, 0, 0), (0, 1 << 24, 1 << 24)]:
        g = desc(rm, (0, 0, 0), (1, 1, 1), dims)
        assert lib.rm_sdf_grid(ctx.handle, C.byref(g), dist.ctypes.data, ids.ctypes.data) == rm.RM_OK, dims
        assert lib.rm_sdf_grid_device(ctx.handle, C.byref(g), dist.ctypes.data, ids.ctypes.data) == rm.RM_OK, dims
        # nothing to do: no pointer is looked at (as n == 0 for points), null or misaligned
        assert lib.rm_sdf_grid(ctx.handle, C.byref(g), None, None) == rm.RM_OK, dims
        assert lib.rm_sdf_grid_device(ctx.handle, C.byref(g), None, None) == rm.RM_OK, dims
        assert lib.rm_sdf_grid_device(ctx.handle, C.byref(g), dist.ctypes.data + 1, None) == rm.RM_OK, dims
    assert (dist == F32(-7.25)).all() and (ids == -99).all()
    # (a bad dim beside a zero dim is still refused)
    assert lib.rm_sdf_grid(ctx.handle, C.byref(desc(rm, (0, 0, 0), (1, 1, 1), (0, -1, 2))), None, None) == rm.RM_ERR_INVALID
    assert ctx.sdf_grid((0, 0, 0), (1, 1, 1), (3, 0, 2)).shape == (2, 0, 3)
    import torch
    td = ctx.sdf_grid((0, 0, 0), (1, 1, 1), (3, 0, 2), device=True)
    assert td.shape == (2, 0, 3) and td.dtype == torch.float32 and td.is_cuda
    td, ti = ctx.sdf_grid((0, 0, 0), (1, 1, 1), (0, 4, 2), ids=True, device=True)
    assert td.shape == ti.shape == (2, 4, 0) and ti.dtype == torch.int32 and ti.device == td.device
    assert td.device.index == ctx.device == torch.cuda.current_device()


@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
def test_grid_of_2_to_26_rows(rm, gpu, table):
    """(1, 4, 2^24): 2^26 one-point rows, more (row, x-block) pairs than one-wave workgroups
    fit a dispatch (its work-item count is 32 bits: 2^26 - 1 workgroups of 64), so the
    workgroups take them with a grid stride.  The outputs stay on the device (256 MB each),
    prefilled with sentinels no answer can be: every element is written, and 24,563 of them
    (both ends and a stride through the middle, every workgroup's turn of the stride among
    them) equal rm_sdf_points on the numpy float32 coordinates and the model."""
    import torch
    dims = (1, 4, 1 << 24)
    n = dims[1] * dims[2]
    origin, step = (-5.0, -6.0, -36.0), (1.0, 5.0, 3e-6)
    scene = random_scene(rm, 1) if table else None
    dev = torch.device("cuda", torch.cuda.current_device())
    pick = np.concatenate([np.arange(4096), np.arange(4096, n - 4096, 4099), np.arange(n - 4096, n)])
    assert len(pick) == 24563 and pick[-4097] > 3 * (1 << 24)  # into the fourth turn of the 2^24 workgroups
    iz, iy = pick // dims[1], pick % dims[1]
    pts = np.stack([np.full(len(pick), F32(origin[0]) + F32(0.0) * F32(step[0]), F32),
                    F32(origin[1]) + iy.astype(F32) * F32(step[1]),
                    F32(origin[2]) + iz.astype(F32) * F32(step[2])], axis=1)
    assert pts.dtype == F32
    with rm.Renderer(37, 23) as r:
        if table:
            r.set_scene(scene)
        r.set_uniforms(default_u(rm))
        dist = torch.full((n,), NAN, dtype=torch.float32, device=dev)
        ids = torch.full((n,), -99, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        g = desc(rm, origin, step, dims)
        assert rm.lib().rm_sdf_grid_device(r.handle, C.byref(g), dist.data_ptr(), ids.data_ptr()) == rm.RM_OK
        r.synchronize()
        assert not bool(torch.isnan(dist).any()) and not bool((ids == -99).any()), "every element written"
        tp = torch.from_numpy(pick).to(dev)
        gd, gi = dist[tp].cpu().numpy(), ids[tp].cpu().numpy()
        rec = r.sdf(pts)
    bits_equal(gd, rec["t"], "2^26 rows: dist against the points call")
    bits_equal(gi, rec["id"], "2^26 rows: ids against the points call")
    want = M.sdf_records(rm, scene if table else rm.default_scene(), 1.0, pts)
    bits_equal(gd, want["t"], "2^26 rows: dist against the model")
    bits_equal(gi, want["id"], "2^26 rows: ids against the model")
    assert table or len(set(gi.tolist())) >= 2


@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
@pytest.mark.parametrize("dims", [(4, 4, 4), (9, 6, 5), (131, 2, 1), (256, 3, 2)])
@pytest.mark.parametrize("off", [0, 1], ids=["aligned", "plus4bytes"])
def test_grid_device_buffers(rm, gpu, dims, off, table):
    """Torch buffers, aligned (16-byte stores where nx allows) and 4 bytes past a 16-byte
    boundary, with sentinels on both sides."""
    import torch
    origin, step = (-30.0, -6.0, -34.0), (0.2, 3.0, 11.0)
    n = dims[0] * dims[1] * dims[2]
    dev = torch.device("cuda", torch.cuda.current_device())
    with rm.Renderer(37, 23) as r:
        if table:
            r.set_scene(random_scene(rm, 1))
        r.set_uniforms(default_u(rm))
        wd, wi = r.sdf_grid(origin, step, dims, ids=True)
        dbuf = torch.full((n + 12,), -7.25, dtype=torch.float32, device=dev)
        ibuf = torch.full((n + 12,), -99, dtype=torch.int32, device=dev)
        assert dbuf.data_ptr() % 16 == 0 and ibuf.data_ptr() % 16 == 0
        lo = 4 + off
        torch.cuda.synchronize()
        g = desc(rm, origin, step, dims)
        rc = rm.lib().rm_sdf_grid_device(r.handle, C.byref(g), dbuf.data_ptr() + 4 * lo, ibuf.data_ptr() + 4 * lo)
        assert rc == rm.RM_OK
        r.synchronize()
        d, i = dbuf.cpu().numpy(), ibuf.cpu().numpy()
        assert (d[:lo] == F32(-7.25)).all() and (d[lo + n:] == F32(-7.25)).all()
        assert (i[:lo] == -99).all() and (i[lo + n:] == -99).all()
        assert d[lo:lo + n].tobytes() == wd.tobytes() and i[lo:lo + n].tobytes() == wi.tobytes()
        # one output aligned, the other not: both still right
        dbuf.fill_(-7.25)
        torch.cuda.synchronize()
        rc = rm.lib().rm_sdf_grid_device(r.handle, C.byref(g), dbuf.data_ptr() + 16, ibuf.data_ptr() + 4 * lo)
        assert rc == rm.RM_OK
        r.synchronize()
        assert dbuf.cpu().numpy()[4:4 + n].tobytes() == wd.tobytes()
        # Renderer.sdf_grid(device=True)
        td, ti = r.sdf_grid(origin, step, dims, ids=True, device=True)
        r.synchronize()
        assert td.shape == (dims[2], dims[1], dims[0]) and td.dtype == torch.float32 and ti.dtype == torch.int32
        assert td.cpu().numpy().tobytes() == wd.tobytes() and ti.cpu().numpy().tobytes() == wi.tobytes()


# ---- 7. plumbing -----------------------------------------------------------------------
def test_torch_stream_and_untouched_images(rm, gpu):
    import torch
    u = default_u(rm)
    pts = all_points()
    dev = torch.device("cuda", torch.cuda.current_device())
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F | rm.RM_OUT_GBUFFER) as r:
        r.set_uniforms(u)
        host = r.sdf(pts, rm.RM_SDF_NORMAL)
        hd, hi = r.sdf_grid((-30, -6, -34), (6, 3, 11), (9, 6, 5), ids=True)
        r.dispatch(u)
        img8, img32, gb = r.read_rgba8(), r.read_rgba32f(), r.read_gbuffer()
        s = torch.cuda.Stream(device=dev)
        try:
            with torch.cuda.stream(s):
                r.set_stream(torch.cuda.current_stream().cuda_stream)
                tp = torch.from_numpy(pts).to(dev)
                r.dispatch(u)
                out = r.sdf(tp, rm.RM_SDF_NORMAL)  # asynchronous, on torch's current stream
                td, ti = r.sdf_grid((-30, -6, -34), (6, 3, 11), (9, 6, 5), ids=True, device=True)
                assert out.shape == (len(pts), 12) and out.dtype == torch.float32 and out.device == tp.device
                back, bd, bi = out.cpu(), td.cpu(), ti.cpu()  # ordered after the queries on the same stream
            np.testing.assert_array_equal(back.numpy().view(np.uint32), host.view(np.uint32).reshape(-1, 12))
            assert bd.numpy().tobytes() == hd.tobytes() and bi.numpy().tobytes() == hi.tobytes()
            # the images dispatched before the queries read back unchanged after them
            assert r.read_rgba8().tobytes() == img8.tobytes()
            assert r.read_rgba32f().tobytes() == img32.tobytes()
            assert r.read_gbuffer().tobytes() == gb.tobytes()
            with pytest.raises(ValueError):
                r.sdf(tp[:, :2])
        finally:
            r.synchronize()
            r.set_stream(None)


def test_counting_context_timing_and_shards(rm, oracle, gpu):
    u = default_u(rm)
    pts = M.edge_points()
    want = M.oracle_records(rm, oracle, u, pts, normal=True)
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA32F, counters=True) as r:
        r.dispatch(u)
        cnt = r.counters()
        records_equal(r.sdf(pts, rm.RM_SDF_NORMAL), want, FIELDS, "counting context")
        r.sdf_grid((0, 0, 0), (1, 1, 1), (5, 3, 2))
        assert r.counters() == cnt
        r.synchronize()
        r.kernel_time_ms(reset=True)
        r.enable_timing(True)
        r.sdf(pts)
        assert r.kernel_time_ms()[1] == 1
        r.sdf_grid((0, 0, 0), (1, 1, 1), (5, 3, 2))
        ms, launches = r.kernel_time_ms()
        assert launches == 2 and ms > 0.0
    with rm.Renderer(37, 23, row_block=4, shard=1, nshards=3) as r:  # evaluates locally
        r.set_uniforms(u)
        records_equal(r.sdf(pts, rm.RM_SDF_NORMAL), want, FIELDS, "sharded context")


def test_refusals(rm, oracle, ctx):
    lib = rm.lib()
    u = default_u(rm)
    ctx.set_uniforms(u)
    pts = M.edge_points()
    n = len(pts)
    out = np.zeros(n + 1, rm.RAY_HIT_DTYPE)
    pp, po = pts.ctypes.data, out.ctypes.data
    INV = rm.RM_ERR_INVALID

    def refused(rc, code=INV):
        assert rc == code, rc
        assert lib.rm_last_error(ctx.handle)

    for fn in (lib.rm_sdf_points, lib.rm_sdf_points_device):
        refused(fn(ctx.handle, None, n, 0, po))
        refused(fn(ctx.handle, pp, n, 0, None))
        refused(fn(ctx.handle, pp, -1, 0, po))
        refused(fn(ctx.handle, pp, 1 << 31, 0, po))
        for flags in (1, 4, 8, 16, 1 << 31, 2 | 1):
            refused(fn(ctx.handle, pp, n, flags, po))
        assert fn(ctx.handle, None, 0, 0, None) == rm.RM_OK  # n == 0: nothing read or written
    refused(lib.rm_sdf_points_device(ctx.handle, pp, n, 0, po // 16 * 16 + 4))  # misaligned out_dev
    dist, ids = np.zeros(64, F32), np.zeros(64, np.int32)
    pd, pi = dist.ctypes.data, ids.ctypes.data
    for fn in (lib.rm_sdf_grid, lib.rm_sdf_grid_device):
        refused(fn(ctx.handle, None, pd, pi))
        refused(fn(ctx.handle, C.byref(desc(rm, (0, 0, 0), (1, 1, 1), (2, 2, 2))), None, None))
        for dims in [(-1, 2, 2), (2, -1, 2), (2, 2, -1), ((1 << 24) + 1, 1, 1), (1, 1, (1 << 24) + 1),
                     (1 << 16, 1 << 15, 1), (1 << 11, 1 << 10, 1 << 10), (1 << 24, 1 << 24, 1 << 24)]:
            refused(fn(ctx.handle, C.byref(desc(rm, (0, 0, 0), (1, 1, 1), dims)), pd, pi))
    assert not out.tobytes().strip(b"\0") and not dist.any() and not ids.any(), "a refused call writes nothing"
    with rm.Renderer(32, 16, ngpus=1) as m:  # a multi-device context: out of scope
        g = desc(rm, (0, 0, 0), (1, 1, 1), (2, 2, 2))
        assert lib.rm_sdf_points(m.handle, pp, n, 0, po) == rm.RM_ERR_STATE
        assert lib.rm_sdf_points_device(m.handle, pp, n, 0, po) == rm.RM_ERR_STATE
        assert lib.rm_sdf_grid(m.handle, C.byref(g), pd, pi) == rm.RM_ERR_STATE
        assert lib.rm_sdf_grid_device(m.handle, C.byref(g), pd, pi) == rm.RM_ERR_STATE
        assert lib.rm_last_error(m.handle)
    # the context still answers correctly afterwards
    records_equal(ctx.sdf(pts, rm.RM_SDF_NORMAL), M.oracle_records(rm, oracle, u, pts, normal=True), FIELDS, "after the refusals")
