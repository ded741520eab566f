"""The hit's clearance on the GPU (rm_scene.hpp "the hit's clearance", DESIGN.md
§4.4 item 22): the plane-only normal and the plane-only shadow steps 0 and 1 of
floor hits, on uniforms aimed at their thresholds.

Bar: test_gpu_parity's stress bar -- exact counters and per-pixel sdf counts, NaN
masks equal to the oracle's, RGBA32F |d| <= 2e-6, RGBA8 |d| <= 1, and the
production image bit-equal to the counting image.  The counting build evaluates
the full scene wherever a lane's claim holds and turns any difference into NaN,
so the NaN mask is the proof's check; the production build takes the fast paths.

Frames of 67x41 and 37x23 (ragged against the 4x4x4 and 8x8 tiles: waves mix
floor, object and sky lanes), AA on and off, 0 and 3 bounces, both shadow modes.
"""
import math

import numpy as np
import pytest

from frames import compare, production_equals_counting, render
from records import bits_equal, gbuf_rays
from uniforms import CASES as FUZZ_CASES
from uniforms import H, W, aim
from uniforms import _uniforms as fuzz_uniforms

pytestmark = pytest.mark.gpu

F32 = np.float32

# (name, sweep frame, camera (pos, lookAt) or None, light or None, iTime or None)
UNIFORMS = [
    ("sweep0", 0, None, None, None),
    ("sweep60", 60, None, None, None),
    ("sweep119", 119, None, None, None),
    # 0.5 above the floor beside the point under sphere 0 (15, 0, -10) r 3: clearance
    # ~2.5 directly under it, falling across one tile
    ("cam_under_sphere0", 60, ((19.0, -5.0, -10.0), (15.0, -5.5, -10.0)), None, None),
    # under the torus ring (centre (-5, 0, 10), lowest point y = -3) and under the
    # capsule's low end (-5.1, -1.9, -30.1) r 1: clearances near 2 r_1
    ("cam_under_torus", 60, ((-5.0, -5.0, 13.5), (-5.0, -5.5, 10.0)), None, None),
    ("cam_under_capsule", 60, ((-2.0, -5.0, -27.0), (-5.1, -5.5, -30.1)), None, None),
    # shadow rays grazing the floor: |rd'| large against rd'.y, t_1 |rd'| large
    ("light_grazing", 60, None, (10.0, -5.3, 5.0), None),
    # r_1 beyond any clearance: only step 0 and the normal can take the fast path
    ("light_1e3", 60, None, (600.0, 500.0, -600.0), None),
    ("light_on_floor", 60, None, (3.0, -5.5, 2.0), None),
    ("light_below_floor", 60, None, (0.0, -7.0, 0.0), None),
    ("itime_0", 60, None, None, 0.0),
    ("itime_blend1", 60, None, None, math.pi / 2),
    ("itime_blend0", 60, None, None, 3 * math.pi / 2),
    # above the blend looking (all but) straight down: reflected rays hit the floor next to it
    ("cam_above_blend", 60, ((-5.0, 14.0, -10.0), (-5.0, 0.0, -10.2)), None, None),
]
# (W, H, aa, bounces, shadow mode): two per uniform, alternating, every value of
# every axis in both halves
COMBOS = [[(67, 41, True, 3, 0), (37, 23, False, 0, 1)],
          [(67, 41, False, 3, 1), (37, 23, True, 0, 0)]]
FRAMES = [(u, c) for j, u in enumerate(UNIFORMS) for c in COMBOS[j % 2]]


def _build(rm, case, combo):
    name, frame, cam, light, itime = case
    W, H, aa, bounces, sm = combo
    u = rm.sweep_uniforms(frame, 120, bounces, aa, sm)
    if cam is not None:
        aim(u, cam[0], cam[1])
    if light is not None:
        for i in range(3):
            u.light.position[i] = light[i]
    if itime is not None:
        u.iTime = itime
    return u


def _bar(rm, oracle, u, W, H, label):
    ref = oracle.render(u, W, H)
    got = render(rm, u, W, H, kernel=rm.RM_KERNEL_PIXEL)
    compare(ref, got, label)
    production_equals_counting(rm, u, W, H, rm.RM_KERNEL_PIXEL, got, label)
    return got


@pytest.mark.parametrize("case,combo", FRAMES,
                         ids=[f"{u[0]}-{c[0]}x{c[1]}_aa{int(c[2])}_b{c[3]}_s{c[4]}" for u, c in FRAMES])
def test_threshold_uniforms(rm, oracle, gpu, case, combo):
    W, H = combo[:2]
    got = _bar(rm, oracle, _build(rm, case, combo), W, H, f"{case[0]} {combo}")
    if case[0].startswith("cam_under"):
        # the frame is what it is meant to be: mostly floor, with an object in view
        n = got["sdf_counts"].size
        assert (got["sdf_counts"] > 0).sum() > n // 2


def test_trace_and_frame_agree_on_normals_and_shadows(rm, oracle, gpu):
    """A frame's own normals (render: the claimed path) against a ray query of every
    pixel's ray (no claim), bit for bit; and the shadow factor of every floor pixel,
    through a SHADOW query of the ray render forms, against the oracle's."""
    W, H = 67, 41
    # beside sphere 0, looking along its far side: floor lit, shadowed and in penumbra
    case = ("cam_beside_sphere0", 60, ((23.0, -3.0, -6.0), (23.0, -6.5, -20.0)), None, None)
    u = _build(rm, case, (W, H, False, 0, 0))
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA32F | rm.RM_OUT_GBUFFER) as r:
        r.dispatch(u)
        g = r.read_gbuffer().reshape(-1)
        o, d = gbuf_rays(oracle, u, W, H, False)
        hit = r.trace(o, d, rm.RM_TRACE_HIT | rm.RM_TRACE_NORMAL)
        bits_equal(hit["t"], g["t"], "t")
        bits_equal(hit["id"], g["id"], "id")
        bits_equal(hit["normal"], g["normal"], "normal: trace vs the frame's G-buffer")
        floor = g["id"] == 7
        assert floor.sum() > W * H // 2
        # render's shadow ray: ro' = pos + 0.02 normal, rd' = light - pos (float32, its order)
        pos = o[floor] + d[floor] * g["t"][floor][:, None]
        ro = pos + g["normal"][floor] * F32(0.02)
        rd = np.array(list(u.light.position), F32)[None, :] - pos
        assert ro.dtype == F32 and rd.dtype == F32
        sh = r.trace(ro, rd, rm.RM_TRACE_SHADOW)["t"]
    want = np.array([oracle.softshadow(u, ro[i], rd[i], 2.0)[0] for i in range(len(ro))], F32)
    bits_equal(sh, want, "shadow factor: trace vs oracle")
    assert len(np.unique(want)) > 3, "the frame has lit, shadowed and penumbra floor"


# ---- fuzz: test_gpu_fuzz_uniforms' cases with the camera just above the floor ---------
NFUZZ = 64


def _low_case(i):
    c = dict(FUZZ_CASES[i])
    rng = np.random.default_rng(9000 + i)
    x, _, z = c["pos"]
    y = float(rng.uniform(-5.4, -3.0))
    look = np.array(c["look"])
    f = look - np.array((x, y, z))
    if np.linalg.norm(f) <= 1.0 or abs(f[1]) / np.linalg.norm(f) >= 0.98:  # the generator's own rule
        look = look + np.array((10.0, 0.0, 0.0))
    c["pos"], c["look"] = (x, y, z), tuple(map(float, look))
    return c


@pytest.mark.parametrize("i", range(NFUZZ))
def test_low_camera_fuzz(rm, oracle, gpu, i):
    assert len(FUZZ_CASES) >= NFUZZ
    c = _low_case(i)
    u = fuzz_uniforms(rm, c)
    if i % 2:
        # the generator's cameras have no yAxis (rm.Camera before its lookAt()): every
        # row of a frame is the same.  Every other case gets the axis of its own basis,
        # cross(dir, xAxis), so that its rows differ.
        x, f = np.array(list(u.camera.xAxis)[:3], np.float64), np.array(list(u.camera.dir)[:3], np.float64)
        y = np.cross(f, x)
        for k in range(3):
            u.camera.yAxis[k] = y[k]
    _bar(rm, oracle, u, W, H, f"low camera case {i} {c}")
