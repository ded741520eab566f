"""The production march's uniform step loop: the supersampled
frame kernels take a march's steps in a wave-uniform loop and go through the lanes' exit
code only on a step where a lane leaves or a segment ends.  The frames here are the ones
on which that hand-over can go wrong:

  down      a camera low over the floor, pitched so that every ray heads down and the top
            row grazes: waves of downward rays only, whose lanes leave together, and one
            lane at a time along the top rows; the grazing rows march past both segment
            ends (steps 16 and 64) to the step cap;
  horizon   the horizon inside a 4-pixel tile row: waves of upward and downward rays;
  grazing   a camera 0.2 above the floor: rays still marching at steps 16 and 64, so the
            loop meets the segment end and the step-cap check, and hits after them;
  in_ball   a camera inside the objects' ball, next to the torus: the culling block is
            due on the first step of a segment and on the step a lane hits;
  w         a camera vector with w != 0: Frame::unit_rd false, the other primary march;
  bounce    a camera close to a sphere: most lanes reflect.

64x32 and 36x20 frames (the second no multiple of the 4x4 tile), supersampled, 3 bounces.
Every case compares the counting build with the oracle at test_gpu_parity's bar (exact
counters and per-pixel sdf counts, equal NaN masks, RGBA32F |d| <= 2e-6, RGBA8 |d| <= 1)
and the production image with the counting build's bit for bit.  The frames' own
properties (hits and misses in every frame, and what each case is about) are checked on
the CPU with the oracle, per sample ray.
"""
import math

import numpy as np
import pytest

from frames import compare, render
from uniforms import aim

SIZES = [(64, 32), (36, 20)]
C_ALL, R_ALL = np.array((-5.0, 0.0, -10.0)), 23.001  # the objects' ball (rm_scene.hpp)


def _down(u):
    # the top row's rays are level at tan(pitch) = 1.281 (cast_ray's uv scale); 1.29 leaves
    # them about 0.2 degrees below the horizon: from 1.5 above the floor they run to the cap
    p, pos = math.atan(1.29), (0.0, -4.0, 30.0)
    aim(u, pos, (pos[0], pos[1] - math.sin(p), pos[2] - math.cos(p)))


def _w(u):
    u.camera.dir[3] = -0.25


CASES = {
    "down": _down,
    "horizon": lambda u: aim(u, (0.0, -3.0, 40.0), (-5.0, -0.5, -10.0)),
    "grazing": lambda u: aim(u, (0.0, -5.3, 60.0), (-5.0, -5.6, -10.0)),
    "in_ball": lambda u: aim(u, (1.0, 2.5, 9.0), (-5.0, 0.0, 10.0)),
    "w": _w,
    "bounce": lambda u: aim(u, (15.0, 0.3, -6.0), (15.0, 0.0, -10.0)),
}


def _uniforms(rm, name):
    u = rm.sweep_uniforms(60, 120, 3, True, 0)
    CASES[name](u)
    return u


_facts = {}


def _frame_facts(rm, oracle, name, W, H):
    """Per sample ray of the frame, from the oracle: the primary hit's id (-1: a miss), the
    primary march's sdf evaluations, and whether the ray heads down; [H, W, 4] each."""
    key = (name, W, H)
    if key not in _facts:
        u = _uniforms(rm, name)
        uvx, uvy = rm.pattern_uv_table(rm.sample_pattern(rm.RM_PATTERN_REFERENCE), W, H)
        o, d = np.empty((H, W, 4, 3), np.float32), np.empty((H, W, 4, 3), np.float32)
        for py in range(H):
            for px in range(W):
                for s in range(4):
                    o[py, px, s], d[py, px, s] = oracle.cast_ray(u, float(uvx[px, s]), float(uvy[py, s]))
        o2, d2 = o.reshape(-1, 3), d.reshape(-1, 3)
        ids = oracle.trace_rays(u, o2, d2)["id"].reshape(H, W, 4)
        steps = oracle.march_steps(u, o2, d2).reshape(H, W, 4)
        _facts[key] = (ids, steps, d[..., 1] <= 0.0, u)
    return _facts[key]


def _mixed_tiles(down, W, H):
    """4x4-pixel tiles (one wave each) that hold upward and downward rays."""
    n = 0
    for ty in range(0, H, 4):
        for tx in range(0, W, 4):
            b = down[ty:ty + 4, tx:tx + 4]
            n += int(b.any() and not b.all())
    return n


@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(CASES))
def test_frames_hold_their_cases(rm, oracle, name, size):
    W, H = size
    ids, steps, down, u = _frame_facts(rm, oracle, name, W, H)
    hit, obj = ids >= 0, (ids >= 0) & (ids != 7)
    assert hit.any() and (~hit).any(), f"{name}: hits {hit.sum()}, misses {(~hit).sum()}"
    if name == "down":
        assert down.all() and (ids[hit] == 7).all()
        # the segment ends inside marches that go on: to a hit, and to the cap
        assert ((steps > 64) & hit).any() and (steps[~hit] == 512).all()
    if name == "horizon":
        assert _mixed_tiles(down, W, H) >= W // 4  # a whole tile row
    if name == "grazing":
        assert ((steps > 16) & (steps <= 64) & hit & down).any() and ((steps > 64) & hit & down).any()
        assert ((steps > 64) & ~hit & down).any()
    if name == "in_ball":
        pos = np.array(list(u.camera.pos)[:3])
        assert np.linalg.norm(pos - C_ALL) < R_ALL and (ids == 5).any()  # the torus in view
    if name == "w":
        assert obj.any() and _mixed_tiles(down, W, H) > 0
    if name == "bounce":
        assert obj.sum() > ids.size // 2, f"{obj.sum()} of {ids.size} rays reflect"


@pytest.mark.gpu
@pytest.mark.parametrize("size", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("name", list(CASES))
def test_production_equals_counting(rm, oracle, gpu, name, size):
    W, H = size
    u = _uniforms(rm, name)
    label = f"{name} {W}x{H}"
    if name == "w":
        with rm.Renderer(W, H) as r:
            r.set_uniforms(u)
            assert r.debug_frame_flags()["unit_rd"] == 0, "Frame::unit_rd"
    ref = oracle.render(u, W, H)
    k = rm.RM_KERNEL_PIXEL
    counted = render(rm, u, W, H, kernel=k)
    compare(ref, counted, label)
    prod = render(rm, u, W, H, kernel=k, counters=False)
    np.testing.assert_array_equal(prod["rgba32f"].view(np.uint32), counted["rgba32f"].view(np.uint32),
                                  err_msg=f"{label}: production RGBA32F against the counting build's, bitwise")
    np.testing.assert_array_equal(np.isnan(prod["rgba32f"]), np.isnan(counted["rgba32f"]),
                                  err_msg=f"{label}: NaN masks")
    np.testing.assert_array_equal(prod["rgba8"], counted["rgba8"], err_msg=f"{label}: RGBA8")
