"""SDF mesh extraction on the GPU (rm_sdf_mesh, rm_sdf_mesh_device).

Expected values: tests/sdf_mesh_model.py, the contract's surface-nets rule in numpy
float32, run on the context's own rm_sdf_grid volume (the contract's d), or for a
non-reference table on tests/sdf_model.py's distances.  Positions, indices and
counts are compared bit for bit, a NaN equal to a NaN; attributes against
rm_sdf_points at the positions.  Uniforms: the defaults with the grid's iTime.
"""
import ctypes as C

import numpy as np
import pytest

import sdf_mesh_model as MM
import sdf_model as M
from grids import GRIDS, desc, grid_points, step3
from records import bits_equal
from scenes import floor_last_scene, random_scene
from uniforms import default_u

pytestmark = pytest.mark.gpu

F32 = np.float32
NAN = float("nan")
FIELDS = ("t", "id", "material", "albedo", "normal", "color")
FLOOR = ((-10.3, -6.2, -3.1), (0.25, 0.5, 0.25), (130, 3, 5))  # 129 cells a row: three waves, a ragged third
GUARD = 0xABABABAB


def mesh_equal(got, want, what):
    """(pos, quads) pairs, bit for bit."""
    assert got[0].shape == want[0].shape and got[1].shape == want[1].shape, (what, got[0].shape, got[1].shape,
                                                                             want[0].shape, want[1].shape)
    bits_equal(got[0], want[0], f"{what}: pos")
    np.testing.assert_array_equal(got[1], want[1], err_msg=f"{what}: indices")


def model_on_own_volume(r, origin, step, dims):
    return MM.mesh(r.sdf_grid(origin, step, dims), origin, step)


def raw_mesh(rm, r, g, flags, vcap, qcap, attr=True, pad=8):
    """rm_sdf_mesh into buffers with `pad` guard records behind the capacities.
    Returns rc, counts, pos words, attr words or None, index words."""
    per = 6 if flags & rm.RM_MESH_TRIANGLES else 4
    pos = np.full((vcap + pad) * 3, GUARD, np.uint32)
    att = np.full((vcap + pad) * 12, GUARD, np.uint32) if attr else None
    idx = np.full((qcap + pad) * per, GUARD, np.uint32)
    n = rm.rm_sdf_mesh_counts(1 << 40, 1 << 40)
    rc = rm.lib().rm_sdf_mesh(r.handle, C.byref(g), flags, pos.ctypes.data if vcap else None,
                              att.ctypes.data if attr and vcap else None, vcap, idx.ctypes.data if qcap else None, qcap,
                              C.byref(n))
    return rc, (int(n.vertices), int(n.quads)), pos, att, idx


@pytest.fixture(scope="module")
def ctx(rm, gpu):
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F) as r:
        yield r


@pytest.fixture(scope="module")
def table_ctx(rm, gpu):
    with rm.Renderer(37, 23) as t:
        t.set_scene(rm.default_scene())
        yield t


# ---- 1. the mesh, bit for bit ----------------------------------------------------------
@pytest.mark.parametrize("g", GRIDS, ids=[g[0] for g in GRIDS])
def test_objects_bit_exact(rm, ctx, table_ctx, g):
    _, origin, step, dims, itime, nv, nq, _ = g
    got = {}
    for name, r in (("builtin", ctx), ("table", table_ctx)):
        r.set_uniforms(default_u(rm, itime=itime))
        pos, quads, attr = r.sdf_mesh(origin, step3(step), dims, attrs=False)
        assert attr is None and pos.dtype == F32 and quads.dtype == np.uint32
        assert (len(pos), len(quads)) == (nv, nq), name
        mesh_equal((pos, quads), model_on_own_volume(r, origin, step3(step), dims), f"{g[0]} {name}")
        got[name] = (pos, quads)
    mesh_equal(got["table"], got["builtin"], f"{g[0]}: the default table against the built-in scene")


def test_a_random_table_against_the_model(rm, gpu):
    scene = random_scene(rm, 1)
    origin, step, dims = (-20.0, -7.0, -37.0), (1.0, 1.0, 1.0), (41, 15, 39)
    d = M.sdf_table(scene, 1.0, grid_points(origin, step, dims))[0].reshape(dims[2], dims[1], dims[0])
    want = MM.mesh(d, origin, step)
    assert len(want[0]) > 300 and len(want[1]) > 300
    with rm.Renderer(37, 23) as t:
        t.set_scene(scene)
        t.set_uniforms(default_u(rm))
        pos, quads, _ = t.sdf_mesh(origin, step, dims, attrs=False)
        mesh_equal((pos, quads), want, "random table 1")
        # rm_scene_specialize on: the generic table code still.  Thrown on a table whose
        # compile is short (test_gpu_sdf.py test_tables_against_the_model)
        t.set_scene(floor_last_scene(rm, 0))
        pos, quads, _ = t.sdf_mesh(origin, step, dims, attrs=False)
        assert len(pos) > 300
        t.specialize_scene(True)
        p2, q2, _ = t.sdf_mesh(origin, step, dims, attrs=False)
        assert p2.tobytes() == pos.tobytes() and q2.tobytes() == quads.tobytes()


def test_blend_differs_between_two_times(rm, ctx):
    _, origin, step, dims, _, _, _, _ = GRIDS[1]
    meshes = []
    for itime in (1.0, 2.5):
        ctx.set_uniforms(default_u(rm, itime=itime))
        pos, quads, _ = ctx.sdf_mesh(origin, step3(step), dims, attrs=False)
        mesh_equal((pos, quads), model_on_own_volume(ctx, origin, step3(step), dims), f"blend at iTime {itime}")
        meshes.append(pos)
    assert meshes[0].tobytes() != meshes[1].tobytes()


def test_floor_sheet_across_a_wave_border(rm, ctx, table_ctx):
    origin, step, dims = FLOOR
    for r in (ctx, table_ctx):
        r.set_uniforms(default_u(rm))
        pos, quads, _ = r.sdf_mesh(origin, step, dims, attrs=False)
        want = model_on_own_volume(r, origin, step, dims)
        assert (len(want[0]), len(want[1])) == (516, 384)  # 129 x 4 cells under the sheet; 128 x 3 interior y edges
        mesh_equal((pos, quads), want, "floor sheet")


def test_past_one_scan_round(rm, ctx):
    """(129, 129, 65) points: 3 x 129 x 65 = 25,155 waves against the scan's 16,384 a round,
    nearly all of them empty; sphere id 0 sits in the middle."""
    origin, step, dims = (8.6, -5.0, -13.2), (0.1, 0.1, 0.1), (129, 129, 65)
    ctx.set_uniforms(default_u(rm, itime=0.0))
    pos, quads, _ = ctx.sdf_mesh(origin, step, dims, attrs=False)
    want = model_on_own_volume(ctx, origin, step, dims)
    assert len(want[0]) > 5000 and len(want[1]) > 5000
    mesh_equal((pos, quads), want, "past one scan round")
    # wave 16,384, where the second round starts, is in slice iz = 42 (z = -9.0): the surface
    # lies on both sides of it
    assert pos[:, 2].min() < -9.5 and pos[:, 2].max() > -8.5


def test_past_one_round_of_chunk_sums(rm, gpu):
    """(2, 4100, 4100) points: 16,810,000 one-row waves in 1,027 scan chunks, against the
    1,024 chunk sums a round of k_mesh_scan_chunks; the floor sheet passes through every z
    slice, the last 8 of them in the second round.  With nx = 2 no edge across the floor is
    interior: vertices only.  The fault this guards (a wrong base for chunks 1,024 and up)
    shows at no smaller grid.  A context of its own, closed with the test: the per-wave
    arrays take 840 MB and the volume 134 MB, which no other test should keep."""
    origin, step, dims = (-0.5, -5.75, -20.0), (1.0, 0.5, 0.01), (2, 4100, 4100)
    with rm.Renderer(37, 23) as r:
        r.set_uniforms(default_u(rm))
        pos, quads, _ = r.sdf_mesh(origin, step, dims, attrs=False)
        want = model_on_own_volume(r, origin, step, dims)
    assert (len(want[0]), len(want[1])) == (4099, 0)
    mesh_equal((pos, quads), want, "past one round of chunk sums")


# ---- 2. triangles, attributes ----------------------------------------------------------
def test_triangles_are_the_split_of_quads(rm, ctx):
    _, origin, step, dims, itime, _, nq, _ = GRIDS[2]
    ctx.set_uniforms(default_u(rm, itime=itime))
    pos, quads, _ = ctx.sdf_mesh(origin, step3(step), dims, attrs=False)
    tpos, tris, _ = ctx.sdf_mesh(origin, step3(step), dims, attrs=False, triangles=True)
    assert tris.shape == (nq, 6) and nq >= 2  # (odd and even quads store in different orders)
    assert tpos.tobytes() == pos.tobytes()
    np.testing.assert_array_equal(tris, MM.triangles(quads))


@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
def test_attributes_equal_the_point_query(rm, ctx, table_ctx, table):
    r = table_ctx if table else ctx
    for g in (GRIDS[1], GRIDS[3]):
        _, origin, step, dims, itime, nv, _, _ = g
        r.set_uniforms(default_u(rm, itime=itime))
        for normals in (False, True):
            pos, _, attr = r.sdf_mesh(origin, step3(step), dims, normals=normals)
            assert attr.dtype == rm.RAY_HIT_DTYPE and len(attr) == nv == len(pos)
            want = r.sdf(pos, rm.RM_SDF_NORMAL if normals else rm.RM_SDF_VALUE)
            for f in FIELDS:
                bits_equal(attr[f], want[f], f"{g[0]} normals={normals} {f}")
            assert not attr["color"].any() and (normals or not attr["normal"].any())
            assert normals is False or np.isfinite(attr["normal"]).all()
    assert set(attr["id"].tolist()) == {5}  # the torus


# ---- 3. capacities ---------------------------------------------------------------------
def test_capacities(rm, ctx):
    _, origin, step, dims, itime, nv, nq, _ = GRIDS[0]
    ctx.set_uniforms(default_u(rm, itime=itime))
    g = desc(rm, origin, step3(step), dims)
    pos, quads, attr = ctx.sdf_mesh(origin, step3(step), dims, normals=True)
    wp, wq, wa = pos.view(np.uint32).reshape(-1), quads.reshape(-1), attr.view(np.uint32).reshape(-1)
    # count only
    n = rm.rm_sdf_mesh_counts()
    assert rm.lib().rm_sdf_mesh(ctx.handle, C.byref(g), 0, None, None, 0, None, 0, C.byref(n)) == rm.RM_OK
    assert (n.vertices, n.quads) == (nv, nq)
    for flags in (rm.RM_MESH_NORMAL, rm.RM_MESH_NORMAL | rm.RM_MESH_TRIANGLES):
        per = 6 if flags & rm.RM_MESH_TRIANGLES else 4
        wi = MM.triangles(quads).reshape(-1) if per == 6 else wq
        for vcap, qcap in ((nv, nq), (nv + 5, nq + 5), (nv - 1, nq - 1), (nv - 1, nq), (0, nq), (nv, 0), (1, 1)):
            rc, counts, p, a, i = raw_mesh(rm, ctx, g, flags, vcap, qcap)
            assert rc == rm.RM_OK and counts == (nv, nq), (vcap, qcap)
            kv, kq = min(vcap, nv), min(qcap, nq)
            np.testing.assert_array_equal(p[:kv * 3], wp[:kv * 3])
            np.testing.assert_array_equal(a[:kv * 12], wa[:kv * 12])
            np.testing.assert_array_equal(i[:kq * per], wi[:kq * per])
            assert (p[kv * 3:] == GUARD).all() and (a[kv * 12:] == GUARD).all() and (i[kq * per:] == GUARD).all(), \
                (vcap, qcap)
    # attr == NULL
    rc, counts, p, a, i = raw_mesh(rm, ctx, g, 0, nv, nq, attr=False)
    assert rc == rm.RM_OK and counts == (nv, nq) and a is None
    np.testing.assert_array_equal(p[:nv * 3], wp)
    np.testing.assert_array_equal(i[:nq * 4], wq)


# ---- 4. the device call ----------------------------------------------------------------
def test_device_call_on_a_torch_stream(rm, gpu):
    import torch
    _, origin, step, dims, itime, nv, nq, _ = GRIDS[1]
    u = default_u(rm, itime=itime)
    dev = torch.device("cuda", torch.cuda.current_device())
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F | rm.RM_OUT_GBUFFER) as r:
        r.set_uniforms(u)
        pos, quads, attr = r.sdf_mesh(origin, step3(step), dims, normals=True)
        assert (len(pos), len(quads)) == (nv, nq)
        r.dispatch_adaptive_edges(u)
        img8, img32, gb, mask, refined = r.read_rgba8(), r.read_rgba32f(), r.read_gbuffer(), r.read_aa_mask(), r.aa_refined()
        assert refined > 0
        g = desc(rm, origin, step3(step), dims)
        s = torch.cuda.Stream(device=dev)
        try:
            with torch.cuda.stream(s):
                r.set_stream(torch.cuda.current_stream().cuda_stream)
                for vcap, qcap, flags in ((nv + 9, nq + 9, rm.RM_MESH_NORMAL), (nv - 3, nq - 2, rm.RM_MESH_NORMAL | rm.RM_MESH_TRIANGLES),
                                          (0, 0, 0)):
                    per = 6 if flags & rm.RM_MESH_TRIANGLES else 4
                    # offset buffers, still 16-byte aligned: 4 guard records (48, 192, 16 per B) before, more behind
                    tp = torch.full(((vcap + 16) * 3,), -7.25, dtype=torch.float32, device=dev)
                    ta = torch.full(((vcap + 16) * 12,), -7.25, dtype=torch.float32, device=dev)
                    ti = torch.full(((qcap + 16) * per,), -99, dtype=torch.int32, device=dev)
                    tc = torch.full((4,), -5, dtype=torch.int64, device=dev)
                    off = lambda t, words: t.data_ptr() + 4 * words
                    assert off(tp, 12) % 16 == 0 and off(ta, 48) % 16 == 0 and off(ti, 4 * per) % 16 == 0
                    rc = rm.lib().rm_sdf_mesh_device(r.handle, C.byref(g), flags, off(tp, 12) if vcap else None,
                                                     off(ta, 48) if vcap else None, vcap, off(ti, 4 * per) if qcap else None,
                                                     qcap, tc.data_ptr() + 8)
                    assert rc == rm.RM_OK
                    hp, ha, hi, hc = tp.cpu().numpy(), ta.cpu().numpy(), ti.cpu().numpy(), tc.cpu().numpy()  # ordered after it
                    assert hc.tolist() == [-5, nv, nq, -5]
                    kv, kq = min(vcap, nv), min(qcap, nq)
                    wi = (MM.triangles(quads) if per == 6 else quads).reshape(-1)[:kq * per].view(np.int32)
                    assert hp[12:12 + kv * 3].tobytes() == pos[:kv].tobytes()
                    assert ha[48:48 + kv * 12].tobytes() == attr[:kv].tobytes()
                    np.testing.assert_array_equal(hi[4 * per:4 * per + kq * per], wi)
                    assert (hp[:12] == F32(-7.25)).all() and (hp[12 + kv * 3:] == F32(-7.25)).all()
                    assert (ha[:48] == F32(-7.25)).all() and (ha[48 + kv * 12:] == F32(-7.25)).all()
                    assert (hi[:4 * per] == -99).all() and (hi[4 * per + kq * per:] == -99).all()
                # Renderer.sdf_mesh(device=True)
                dp, di, da, dc = r.sdf_mesh(origin, step3(step), dims, normals=True, device=True, max_vertices=nv + 7,
                                            max_quads=nq + 1)
                assert dp.shape == (nv + 7, 3) and di.shape == (nq + 1, 4) and da.shape == (nv + 7, 12)
                assert dc.cpu().tolist() == [nv, nq]
                assert dp[:nv].cpu().numpy().tobytes() == pos.tobytes()
                assert da[:nv].cpu().numpy().tobytes() == attr.tobytes()
                assert di[:nq].cpu().numpy().view(np.uint32).tobytes() == quads.tobytes()
                with pytest.raises(ValueError):
                    r.sdf_mesh(origin, step3(step), dims, device=True)
            # the images, the G-buffer and the AA mask read back unchanged after the calls
            assert r.read_rgba8().tobytes() == img8.tobytes()
            assert r.read_rgba32f().tobytes() == img32.tobytes()
            assert r.read_gbuffer().tobytes() == gb.tobytes()
            assert r.read_aa_mask().tobytes() == mask.tobytes() and r.aa_refined() == refined
        finally:
            r.synchronize()
            r.set_stream(None)


def test_device_wrapper_on_the_contexts_own_stream(rm, gpu):
    """Renderer.sdf_mesh(device=True) without set_stream: the library writes on the context's
    own non-blocking stream, which nothing orders against torch's current one.  The wrapper
    therefore queues no torch kernel on its outputs (a fill of the counts could land after the
    library's write); torch's stream is kept busy here so that such a fill would be late."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device())
    busy = torch.ones(1 << 26, dtype=torch.float32, device=dev)
    with rm.Renderer(37, 23) as r:
        for g in (GRIDS[1], GRIDS[3]):
            _, origin, step, dims, itime, nv, nq, _ = g
            r.set_uniforms(default_u(rm, itime=itime))
            pos, quads, attr = r.sdf_mesh(origin, step3(step), dims, normals=True)
            for _ in range(8):
                busy.mul_(1.0)  # 256 MB each way per kernel, queued on torch's stream
            dp, di, da, dc = r.sdf_mesh(origin, step3(step), dims, normals=True, device=True, max_vertices=nv + 3,
                                        max_quads=nq + 3)
            r.synchronize()
            torch.cuda.synchronize()
            assert dc.cpu().tolist() == [nv, nq], g[0]
            assert dp[:nv].cpu().numpy().tobytes() == pos.tobytes()
            assert di[:nq].cpu().numpy().view(np.uint32).tobytes() == quads.tobytes()
            assert da[:nv].cpu().numpy().tobytes() == attr.tobytes()
        # a grid without a cell: the counts are written all the same
        for _ in range(8):
            busy.mul_(1.0)
        dp, di, da, dc = r.sdf_mesh((0, 0, 0), (1, 1, 1), (5, 1, 5), device=True, max_vertices=4, max_quads=4)
        r.synchronize()
        torch.cuda.synchronize()
        assert dc.cpu().tolist() == [0, 0]


# ---- 5. degenerate grids ---------------------------------------------------------------
def test_degenerate_grids(rm, ctx):
    import torch
    ctx.set_uniforms(default_u(rm))
    dev = torch.device("cuda", torch.cuda.current_device())
    cases = [((0, 0, 0), (1, 1, 1), (0, 5, 5)), ((0, 0, 0), (1, 1, 1), (5, 1, 5)), ((0, 0, 0), (1, 1, 1), (5, 5, 0)),
             ((0, 0, 0), (1, 1, 1), (1, 1, 1)), ((0, 0, 0), (1, 1, 1), (1 << 24, 1, 127)),
             ((-5.0, -6.2, -5.0), (NAN, 0.5, 1.0), (9, 4, 7)),       # a NaN step: a NaN volume, all outside
             ((NAN, -6.2, -5.0), (1.0, 0.5, 1.0), (9, 4, 7)),
             ((-5.0, -9.0, -5.0), (1.0, 0.5, 1.0), (70, 6, 5))]      # below the floor: all inside
    for origin, step, dims in cases:
        g = desc(rm, origin, step, dims)
        rc, counts, p, a, i = raw_mesh(rm, ctx, g, rm.RM_MESH_NORMAL, 4, 4)
        assert rc == rm.RM_OK and counts == (0, 0), (origin, step, dims)
        assert (p == GUARD).all() and (a == GUARD).all() and (i == GUARD).all()
        tc = torch.full((2,), -5, dtype=torch.int64, device=dev)
        torch.cuda.synchronize()
        assert rm.lib().rm_sdf_mesh_device(ctx.handle, C.byref(g), 0, None, None, 0, None, 0, tc.data_ptr()) == rm.RM_OK
        ctx.synchronize()
        assert tc.cpu().tolist() == [0, 0], (origin, step, dims)
        pos, quads, attr = ctx.sdf_mesh(origin, step, dims)
        assert pos.shape == (0, 3) and quads.shape == (0, 4) and attr.shape == (0,)
    if min(cases[-1][2]) >= 2:
        assert (ctx.sdf_grid(*cases[-1]) < 0).all()


# ---- 6. plumbing -----------------------------------------------------------------------
def test_timing_counts_one_launch(rm, gpu):
    _, origin, step, dims, itime, nv, nq, _ = GRIDS[0]
    g = desc(rm, origin, step3(step), dims)
    with rm.Renderer(37, 23) as r:
        r.set_uniforms(default_u(rm, itime=itime))
        r.synchronize()
        r.kernel_time_ms(reset=True)
        r.enable_timing(True)
        rc, counts, *_ = raw_mesh(rm, r, g, rm.RM_MESH_NORMAL, nv, nq)
        assert rc == rm.RM_OK and counts == (nv, nq)
        ms, launches = r.kernel_time_ms()
        assert launches == 1 and ms > 0.0
        import torch
        tc = torch.zeros(2, dtype=torch.int64, device=torch.device("cuda", torch.cuda.current_device()))
        torch.cuda.synchronize()
        assert rm.lib().rm_sdf_mesh_device(r.handle, C.byref(g), 0, None, None, 0, None, 0, tc.data_ptr()) == rm.RM_OK
        r.synchronize()
        assert r.kernel_time_ms()[1] == 2 and tc.cpu().tolist() == [nv, nq]


def test_shards_and_counters_give_the_plain_mesh(rm, ctx):
    _, origin, step, dims, itime, nv, nq, _ = GRIDS[1]
    u = default_u(rm, itime=itime)
    ctx.set_uniforms(u)
    want = ctx.sdf_mesh(origin, step3(step), dims, normals=True)
    with rm.Renderer(37, 23, row_block=4, shard=1, nshards=3) as r:  # runs locally
        r.set_uniforms(u)
        got = r.sdf_mesh(origin, step3(step), dims, normals=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA32F, counters=True) as r:
        r.dispatch(u)
        cnt = r.counters()
        got = r.sdf_mesh(origin, step3(step), dims, normals=True)
        assert all(a.tobytes() == b.tobytes() for a, b in zip(got, want))
        assert r.counters() == cnt
    assert (len(want[0]), len(want[1])) == (nv, nq)


def test_refusals(rm, ctx):
    lib = rm.lib()
    _, origin, step, dims, itime, nv, nq, _ = GRIDS[0]
    ctx.set_uniforms(default_u(rm, itime=itime))
    g = C.byref(desc(rm, origin, step3(step), dims))
    pos = np.zeros((nv + 1) * 3, F32)
    attr = np.zeros(nv + 1, rm.RAY_HIT_DTYPE)
    idx = np.zeros((nq + 1) * 6, np.uint32)
    cnt = np.zeros(4, np.uint64)
    pp, pa, pi, pc = pos.ctypes.data, attr.ctypes.data, idx.ctypes.data, cnt.ctypes.data
    assert pp % 16 == 0 and pa % 16 == 0 and pi % 16 == 0 and pc % 8 == 0
    INV = rm.RM_ERR_INVALID

    def refused(rc, code=INV):
        assert rc == code, rc
        assert lib.rm_last_error(ctx.handle)

    for fn in (lib.rm_sdf_mesh, lib.rm_sdf_mesh_device):
        h = ctx.handle
        refused(fn(h, None, 0, pp, pa, nv, pi, nq, pc))
        refused(fn(h, g, 0, pp, pa, nv, pi, nq, None))
        for flags in (4, 8, 16, 1 << 31, 3 | 4):
            refused(fn(h, g, flags, pp, pa, nv, pi, nq, pc))
        refused(fn(h, g, 0, pp, pa, -1, pi, nq, pc))
        refused(fn(h, g, 0, pp, pa, nv, pi, -1, pc))
        refused(fn(h, g, 0, None, pa, nv, pi, nq, pc))
        refused(fn(h, g, 0, pp, pa, nv, None, nq, pc))
        for bad in [(-1, 2, 2), (2, -1, 2), (2, 2, -1), ((1 << 24) + 1, 2, 2), (2, 2, (1 << 24) + 1),
                    (1 << 16, 1 << 15, 1), (1 << 11, 1 << 10, 1 << 10), (1 << 24, 1 << 24, 1 << 24), (0, -1, 2)]:
            refused(fn(h, C.byref(desc(rm, (0, 0, 0), (1, 1, 1), bad)), 0, pp, pa, nv, pi, nq, pc))
    h = ctx.handle
    refused(lib.rm_sdf_mesh_device(h, g, 0, pp + 4, pa, nv, pi, nq, pc))
    refused(lib.rm_sdf_mesh_device(h, g, 0, pp, pa + 8, nv, pi, nq, pc))
    refused(lib.rm_sdf_mesh_device(h, g, 0, pp, pa, nv, pi + 4, nq, pc))
    refused(lib.rm_sdf_mesh_device(h, g, 0, pp, pa, nv, pi, nq, pc + 4))
    assert not pos.any() and not idx.any() and not cnt.any() and not attr.tobytes().strip(b"\0"), \
        "a refused call writes nothing"
    with rm.Renderer(32, 16, ngpus=1) as m:  # a multi-device context: out of scope
        n = rm.rm_sdf_mesh_counts()
        assert lib.rm_sdf_mesh(m.handle, g, 0, pp, pa, nv, pi, nq, C.byref(n)) == rm.RM_ERR_STATE
        assert lib.rm_sdf_mesh_device(m.handle, g, 0, pp, pa, nv, pi, nq, pc) == rm.RM_ERR_STATE
        assert lib.rm_last_error(m.handle)
    assert not pos.any() and not idx.any() and not cnt.any()
    # the context still answers correctly afterwards
    got = ctx.sdf_mesh(origin, step3(step), dims, attrs=False)
    assert (len(got[0]), len(got[1])) == (nv, nq)
