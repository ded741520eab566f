"""tests/sdf_model.py, the numpy restatement of the oracle's table sdf, equals the
oracle itself bit for bit on the table the oracle can evaluate both ways: the
default table is the built-in scene (oracle.sdf / oracle.get_normal).  This pins
the yardstick test_gpu_sdf.py measures the table kernels with; it needs no
field-query code."""
import numpy as np
import pytest

import sdf_model as M


@pytest.mark.parametrize("itime", [0.0, 1.0, 4.5])
def test_model_equals_the_oracle_on_the_default_table(rm, oracle, itime):
    u = rm.default_uniforms()
    u.iTime = itime
    pts = np.concatenate([M.seeded_points(), M.edge_points()])
    want = M.oracle_records(rm, oracle, u, pts, normal=True)
    got = M.sdf_records(rm, rm.default_scene(), itime, pts, normal=True)
    for f in ("t", "id", "material", "albedo", "normal"):
        M.bits_equal(got[f], want[f], f"iTime {itime} {f}")


def test_the_seeded_set_covers_the_scene(rm, oracle):
    u = rm.default_uniforms()
    u.iTime = 1.0
    want = M.oracle_records(rm, oracle, u, M.seeded_points())
    assert [int((want["id"] == k).sum()) for k in (0, 1, 4, 5, 6, 7)] == [208, 181, 179, 157, 157, 1118]
    assert int((want["t"] < 0).sum()) == 186
    e = M.oracle_records(rm, oracle, u, M.edge_points(), normal=True)
    zero_grad = [14, 15]  # (1e5, 1e5, 1e5), (3e5, -2e5, 1e5): the 0.001 offsets vanish
    assert np.isnan(e["normal"][zero_grad]).all() and np.isfinite(e["t"][zero_grad]).all()
