"""tests/sdf_mesh_model.py, the numpy restatement of rm_sdf_mesh's surface-nets rule
(include/rm_api.h), pinned on hand-made volumes and on the default
table's distances by tests/sdf_model.py (which test_sdf_model.py pins to the
oracle).  The GPU tests compare librm with this model bit for bit."""
import numpy as np
import pytest

import sdf_mesh_model as MM
import sdf_model as M
from grids import GRIDS, grid_points

F32 = np.float32
NAN, INF = float("nan"), float("inf")

def table_volume(scene, itime, origin, step, dims):
    d = M.sdf_table(scene, itime, grid_points(origin, step, dims))[0]
    return d.reshape(dims[2], dims[1], dims[0])


def test_one_negative_corner():
    d = np.ones((2, 2, 2), F32)
    d[0, 0, 0] = -1.0
    pos, quads = MM.mesh(d, (0, 0, 0), (1, 1, 1))
    want = (F32(0.0) + F32(0.5) + F32(0.0) + F32(0.0)) / F32(3.0)  # one crossing per axis, t = 0.5
    assert pos.dtype == F32 and pos.shape == (1, 3) and quads.shape == (0, 4)
    assert pos.tobytes() == np.array([[want] * 3], F32).tobytes()
    assert abs(float(want) - 1 / 6) < 1e-7


def test_centre_negative():
    d = np.ones((3, 3, 3), F32)
    d[1, 1, 1] = -1.0
    pos, quads = MM.mesh(d, (-1, -1, -1), (1, 1, 1))
    assert pos.shape == (8, 3) and quads.shape == (6, 4) and quads.dtype == np.uint32
    # the vertices in cell order: three crossings half an edge from the centre, one per axis
    s = F32(0.5) / F32(3.0)
    want = [(x, y, z) for z in (-s, s) for y in (-s, s) for x in (-s, s)]
    assert pos.tobytes() == np.array(want, F32).tobytes()
    closed, referenced, euler, vol = MM.topology(pos, quads)
    assert closed and referenced and euler == 2 and vol == pytest.approx(1 / 27, rel=1e-6)
    # every quad wound outward: its normal points away from the centre
    P = pos.astype(np.float64)
    for q in quads:
        nrm = np.cross(P[q[1]] - P[q[0]], P[q[2]] - P[q[0]])
        assert np.dot(nrm, P[q].mean(axis=0)) > 0
    # emission order: point order, then axis; the first is the z edge below the centre (B inside)
    assert quads[0].tolist() == [0, 2, 3, 1] and quads[-1].tolist() == [4, 5, 7, 6]
    np.testing.assert_array_equal(MM.triangles(quads)[0], [0, 2, 3, 0, 3, 1])


def test_nan_zeros_and_infinity_are_outside():
    for outside in (NAN, 0.0, -0.0, INF):
        d = np.full((3, 3, 3), outside, F32)
        pos, quads = MM.mesh(d, (0, 0, 0), (1, 1, 1))
        assert len(pos) == 0 and len(quads) == 0
        d[1, 1, 1] = -1.0
        pos, quads = MM.mesh(d, (0, 0, 0), (1, 1, 1))
        assert pos.shape == (8, 3) and quads.shape == (6, 4)
        if outside == INF:
            # the inside point is A of the last cell's crossings: t = dA / (dA - inf) = +0, on it;
            # it is B of the first cell's: t = inf / (inf - dB) = inf / inf, a NaN
            assert (pos[7] == F32(1.0)).all() and np.isnan(pos[0]).all()
        elif outside != outside:
            assert np.isnan(pos).all()
        else:  # t = 1 from the inside point, 0 from the outside point: on the outside point
            assert np.allclose(np.abs(pos - 1), 1 / 3, rtol=1e-6)
    allin = np.full((4, 3, 5), -2.0, F32)
    assert [len(a) for a in MM.mesh(allin, (0, 0, 0), (1, 1, 1))] == [0, 0]
    d = np.full((3, 3, 3), -INF, F32)  # inside everywhere but one NaN: 8 active cells again
    d[1, 1, 1] = NAN
    pos, quads = MM.mesh(d, (0, 0, 0), (1, 1, 1))
    assert pos.shape == (8, 3) and quads.shape == (6, 4) and np.isnan(pos).all()


@pytest.mark.parametrize("shape", [(1, 3, 3), (3, 1, 3), (3, 3, 1), (1, 1, 1), (0, 3, 3)])
def test_a_dim_below_two_has_no_cell(shape):
    d = -np.ones(shape, F32)
    pos, quads = MM.mesh(d, (0, 0, 0), (1, 1, 1))
    assert pos.shape == (0, 3) and quads.shape == (0, 4)


def test_boundary_edges_emit_nothing():
    """A sheet through a 4x3x4 grid: quads only around the edges one point inside the border."""
    d = np.ones((4, 3, 4), F32)
    d[:, 0, :] = -1.0  # inside below y = 0.5
    pos, quads = MM.mesh(d, (0, 0, 0), (1, 1, 1))
    assert len(pos) == 9 and len(quads) == 4  # 3 x 3 cells of the lower layer, 2 x 2 interior y edges
    assert not MM.topology(pos, quads)[0]  # an open border


@pytest.mark.parametrize("g", GRIDS, ids=[g[0] for g in GRIDS])
def test_default_table_objects(rm, g):
    _, origin, step, dims, itime, nv, nq, chi = g
    d = table_volume(rm.default_scene(), itime, origin, (step,) * 3, dims)
    pos, quads = MM.mesh(d, origin, (step,) * 3)
    assert (len(pos), len(quads)) == (nv, nq)
    closed, referenced, euler, vol = MM.topology(pos, quads)
    assert closed, "every directed quad edge once, its reverse once"
    assert referenced and euler == chi and vol > 0.0
    assert np.isfinite(pos).all()
    lo, hi = np.array(origin, F32), np.array(origin, F32) + F32(step) * (np.array(dims, F32) - 1)
    assert (pos >= lo).all() and (pos <= hi).all()


def test_blend_moves_with_itime(rm):
    _, origin, step, dims, _, _, _, _ = GRIDS[1]
    a = MM.mesh(table_volume(rm.default_scene(), 1.0, origin, (step,) * 3, dims), origin, (step,) * 3)
    b = MM.mesh(table_volume(rm.default_scene(), 2.5, origin, (step,) * 3, dims), origin, (step,) * 3)
    assert a[0].tobytes() != b[0].tobytes()
