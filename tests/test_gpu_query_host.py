"""The host layer the query families share (rm_api_query.hip):
the staging buffers of their synchronous host paths and the bracket of a timed launch.

No expected values of the queries themselves: those are test_gpu_trace.py's,
test_gpu_sdf.py's and test_gpu_sdf_mesh.py's.  Here a context that has served other
calls is compared, bit for bit, with a fresh one that has not, and the launches a timed
context counts with the calls made.  33 x 19 contexts, the built-in scene and
default_scene() as a table; uniforms: the defaults with iTime = 1.
"""
import ctypes as C

import numpy as np
import pytest

from uniforms import default_u

pytestmark = pytest.mark.gpu

F32 = np.float32
BOX = ([-30, -5, -35], [20, 15, 20])  # the scene's box (tests/records.py random_rays)
SPHERE = (15.0, 0.0, -10.0)
IDS = {0, 1, 4, 5, 6, 7}              # every object and the floor (tests/test_gpu_trace.py AIMED_IDS)
MESH_GRID = ((10.4, -4.6, -14.1), (0.9, 0.9, 0.9), (12, 10, 9))  # around the sphere
ID_GRID = ((10.0, -4.0, -14.0), (1.2, 1.2, 1.2), (9, 7, 5))      # through it


def make_ctx(rm, table):
    r = rm.Renderer(33, 19)
    if table:
        r.set_scene(rm.default_scene())
    r.set_uniforms(default_u(rm))
    return r


def rays(rng, n):
    o = rng.uniform(*BOX, (n, 3)).astype(F32)
    d = rng.normal(size=(n, 3))
    return o, (d / np.linalg.norm(d, axis=1, keepdims=True)).astype(F32)


def words(x):
    return np.ascontiguousarray(x).view(np.uint32)


def hit_and_miss(hit, what):
    assert hit.any() and not hit.all(), f"{what}: {int(hit.sum())} of {hit.size} inputs hit"


# ---- 1. the shared staging buffers ---------------------------------------------------------
@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
def test_shared_staging_serves_every_family(rm, gpu, table):
    """Ray queries, field queries and the mesh extraction stage through one pair of buffers.
    Bytes per input: a point 12, a record 48, a ray 24 (origins, then dirs at a 256-byte
    boundary).  The sequence grows both buffers past their first 64 KiB and then serves
    smaller calls of every family from the grown ones: every result is, bit for bit, a fresh
    context's.  A ray hits when its id is not -1, a point when it lies inside an object
    (t < 0); the calls of one input take one that hits."""
    rng = np.random.default_rng(11)
    sphere = np.array([SPHERE], F32)
    up = (np.array([[0, 10, 15]], F32), np.array([[0, 1, 0]], F32))
    aim = np.array(SPHERE, np.float64) - up[0][0]
    one_ray = (up[0], (aim / np.linalg.norm(aim)).astype(F32)[None, :])
    pts = rng.uniform(*BOX, (6000, 3)).astype(F32)
    r3000, r70 = rays(rng, 3000), rays(rng, 70)
    calls = [
        ("trace 1", lambda r: (r.trace(*one_ray),)),
        ("sdf 6000", lambda r: (r.sdf(pts, rm.RM_SDF_NORMAL),)),
        ("trace 3000", lambda r: (r.trace(*r3000, rm.RM_TRACE_HIT | rm.RM_TRACE_NORMAL),)),
        ("sdf_grid", lambda r: r.sdf_grid(*ID_GRID, ids=True)),
        ("sdf_mesh", lambda r: r.sdf_mesh(*MESH_GRID)),
        ("trace 70", lambda r: (r.trace(*r70),)),
        ("sdf 1", lambda r: (r.sdf(sphere),)),
    ]
    with make_ctx(rm, table) as shared:
        got = {name: call(shared) for name, call in calls}
    for name, call in calls:
        with make_ctx(rm, table) as fresh:
            want = call(fresh)
        assert len(got[name]) == len(want)
        for g, w in zip(got[name], want):
            assert g.shape == w.shape and g.dtype == w.dtype, name
            np.testing.assert_array_equal(words(g), words(w), err_msg=name)
    # the comparisons were of hits and of misses, of every id
    assert got["trace 1"][0]["id"][0] == 0 and got["sdf 1"][0]["t"][0] < 0
    hit_and_miss(got["sdf 6000"][0]["t"] < 0, "sdf 6000")
    assert set(got["sdf 6000"][0]["id"].tolist()) == IDS
    hit_and_miss(got["trace 3000"][0]["id"] != -1, "trace 3000")
    assert set(got["trace 3000"][0]["id"].tolist()) == IDS | {-1}
    hit_and_miss(got["sdf_grid"][0] < 0, "sdf_grid")
    assert len(set(got["sdf_grid"][1].reshape(-1).tolist())) > 1
    pos, quads, attr = got["sdf_mesh"]
    assert len(pos) > 50 and len(quads) > 50 and len(attr) == len(pos)
    hit_and_miss(got["trace 70"][0]["id"] != -1, "trace 70")


# ---- 2. the bracket of a timed launch ------------------------------------------------------
def mesh_once(rm, r):
    """One rm_sdf_mesh call with room for every cell (Renderer.sdf_mesh makes two: a
    count-only one first); returns the counts."""
    origin, step, dims = MESH_GRID
    g = rm.rm_sdf_grid_desc((C.c_float * 3)(*origin), (C.c_float * 3)(*step), (C.c_int32 * 3)(*dims))
    cells = (dims[0] - 1) * (dims[1] - 1) * (dims[2] - 1)
    pos = np.empty((cells, 3), F32)
    attr = np.empty(cells, rm.RAY_HIT_DTYPE)
    idx = np.empty((3 * cells, 4), np.uint32)
    n = rm.rm_sdf_mesh_counts()
    rc = rm.lib().rm_sdf_mesh(r.handle, C.byref(g), 0, pos.ctypes.data, attr.ctypes.data, cells, idx.ctypes.data,
                              3 * cells, C.byref(n))
    assert rc == 0, rc
    return int(n.vertices), int(n.quads)


@pytest.mark.parametrize("table", [False, True], ids=["builtin", "table"])
def test_timed_launches_are_counted_once_each(rm, gpu, table):
    """Every bracket counts one launch and a batch its frames: a dispatch, a batch of 3,
    a trace, a point query, a grid query, a mesh and an adaptive dispatch are 9.  Reading
    the time releases the pairs, and the next round reuses them."""
    rng = np.random.default_rng(12)
    o, d = rays(rng, 5)
    pts = rng.uniform(*BOX, (5, 3)).astype(F32)
    u = default_u(rm)
    with make_ctx(rm, table) as r:
        r.enable_timing(True)
        for _ in range(2):
            r.dispatch(u)
            r.dispatch_frames([u, u, u])
            r.trace(o, d)
            r.sdf(pts)
            r.sdf_grid((10.0, -4.0, -14.0), (2.0, 2.0, 2.0), (4, 4, 4))
            nv, nq = mesh_once(rm, r)
            assert nv > 50 and nq > 50
            r.dispatch_adaptive(u, threshold=8)
            ms, launches = r.kernel_time_ms(reset=True)
            assert launches == 9 and ms > 0.0, (launches, ms)
            assert r.kernel_time_ms()[1] == 0
