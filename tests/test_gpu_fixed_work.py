"""The once-per-wave and once-per-hit code of the frame kernels (DESIGN.md §4.4 item
23): cast_ray's lean form on Frame::unit_rd frames, the v_med3 quantise, the wave
vote around the shading's roots and the host's light-in-ball flag, which the
supersampled frame kernels take; and the frames on which a switch to the downward
step loop at a march's segment ends was measured and not adopted (the segment
ends themselves stay under test).

Frames of 64x48: with supersampling 192 one-wave workgroups (a 4x4 pixel tile with
its 4 samples each), without it 48 of k_pixel's 8x8 tiles.  Every case runs three
comparisons:
  * the counting build against the oracle at test_gpu_parity's bar (exact counters
    and per-pixel sdf counts, equal NaN masks, RGBA32F |d| <= 2e-6, RGBA8 |d| <= 1);
  * the production image against the counting build's, RGBA32F bit for bit (so the
    production image meets the same bar).  The counting kernels keep the plain forms:
    this comparison is the one that sets the lean forms against them;
  * RGBA8 against round(clamp(x, 0, 1) * 255), NaN -> 0, formed in numpy from the
    same context's RGBA32F image, exactly.
"""
import math

import numpy as np
import pytest

from frames import compare, render
from uniforms import aim

pytestmark = pytest.mark.gpu

W, H = 64, 48
F32 = np.float32


def _flags(rm, u):
    """(Frame::unit_rd, Frame::light_ball) of a frame with these uniforms."""
    with rm.Renderer(W, H) as r:
        r.set_uniforms(u)
        f = r.debug_frame_flags()
    return f["unit_rd"], f["light_ball"]


def _three(rm, oracle, u, label, w=W, h=H):
    ref = oracle.render(u, w, h)
    k = rm.RM_KERNEL_PIXEL
    counted = render(rm, u, w, h, kernel=k)
    compare(ref, counted, label)
    prod = render(rm, u, w, h, kernel=k, counters=False)
    np.testing.assert_array_equal(prod["rgba32f"].view(np.uint32), counted["rgba32f"].view(np.uint32),
                                  err_msg=f"{label}: production RGBA32F against the counting build's, bitwise")
    np.testing.assert_array_equal(np.isnan(prod["rgba32f"]), np.isnan(counted["rgba32f"]),
                                  err_msg=f"{label}: NaN masks")
    for name, img in (("counting", counted), ("production", prod)):
        np.testing.assert_array_equal(img["rgba8"], rm.quantize_rgba8(img["rgba32f"]),
                                      err_msg=f"{label}: {name} RGBA8 against its own RGBA32F")
    return counted, prod


# ---- cast_ray -------------------------------------------------------------------
def _scaled(s):
    def f(u):
        for k in range(3):
            u.camera.xAxis[k] *= s
            u.camera.yAxis[k] *= s
            u.camera.dir[k] *= s
    return f


def _w(vec, v):
    def f(u):
        getattr(u.camera, vec)[3] = v
    return f


# (name, sweep frame, change, Frame::unit_rd).  unit_rd_check bounds |v|^2 against the
# float error of v and against 2^-80; it does not ask for |v| = 1 (rd is v / |v|), so a
# basis scaled by 2 passes it and takes the lean form at twice the size.  2^-45 brings
# |v|^2 to about 2^-90: below the check's 2^-80 and above sqrt_vote's 2^-96 (the vote
# passes); 2^-50 brings it to about 2^-100, below both.
CAMERAS = [
    ("sweep0", 0, None, 1),
    ("sweep60", 60, None, 1),
    ("sweep119", 119, None, 1),
    ("xaxis_w", 60, _w("xAxis", 0.5), 0),
    ("dir_w", 30, _w("dir", -0.25), 0),
    ("scaled_2", 60, _scaled(2.0), 1),
    ("scaled_2^-45", 60, _scaled(2.0 ** -45), 0),
    ("scaled_2^-50", 60, _scaled(2.0 ** -50), 0),
]


@pytest.mark.parametrize("aa", [True, False], ids=["aa", "noaa"])
@pytest.mark.parametrize("case", CAMERAS, ids=lambda c: c[0])
def test_cast_ray(rm, oracle, gpu, case, aa):
    name, frame, change, unit = case
    u = rm.sweep_uniforms(frame, 120, 3 if aa else 1, aa, 0)
    if change:
        change(u)
    assert _flags(rm, u)[0] == unit, f"{name}: Frame::unit_rd"
    counted, _ = _three(rm, oracle, u, f"{name} aa={aa}")
    assert (counted["sdf_counts"] > 0).all()


# ---- the light flag ---------------------------------------------------------------
# The objects' ball: R_ALL = 23.001 around (-5, 0, -10); the flag is |light - C|^2 <=
# R_ALL^2 (1 - 2^-10), so a light at distance R_ALL exactly is outside.
LIGHTS = [
    ("inside", (-5.0, 22.9, -10.0), 1),
    ("sweep", None, 1),
    ("outside", (-5.0, 23.1, -10.0), 0),
    ("boundary", (-5.0, 23.001, -10.0), 0),
    ("inf", (-5.0, math.inf, -10.0), 0),
    ("nan", (math.nan, 5.0, -10.0), 0),
]


@pytest.mark.parametrize("sm", [0, 1], ids=["soft", "hard"])
@pytest.mark.parametrize("case", LIGHTS, ids=lambda c: c[0])
def test_light_flag(rm, oracle, gpu, case, sm):
    name, light, flag = case
    u = rm.sweep_uniforms(60, 120, 3, True, sm)
    if light is not None:
        for k in range(3):
            u.light.position[k] = light[k]
    assert _flags(rm, u)[1] == flag, f"{name}: Frame::light_ball"
    _three(rm, oracle, u, f"light {name} sm={sm}")


# ---- quantise ---------------------------------------------------------------------
# light colours that take pixels below 0, above 1, to infinity and to NaN.  The infinite
# colour is the ambient one: an infinite specular colour multiplies pow(x, 32), which
# underflows to 0 on the GPU (exp2(32 log2 x)) where powf keeps a denormal,
# and inf * 0 is NaN where inf * denormal is inf: pow's known difference, not quantise's.
COLOURS = [
    ("negative", "diffuse", (-1.0, -0.5, -2.0)),
    ("negative_ambient", "ambient", (-0.2, -0.2, 0.3)),
    ("above_1", "diffuse", (3.0, 2.0, 4.0)),
    ("inf", "ambient", (math.inf, 0.2, math.inf)),
    ("nan", "ambient", (math.nan, 0.2, 0.2)),
]


@pytest.mark.parametrize("case", COLOURS, ids=lambda c: c[0])
def test_quantize(rm, oracle, gpu, case):
    name, field, col = case
    u = rm.sweep_uniforms(60, 120, 1, True, 0)
    for k in range(3):
        getattr(u.light, field)[k] = col[k]
    _, prod = _three(rm, oracle, u, f"colour {name}")
    x = prod["rgba32f"][..., :3]
    if name == "above_1":
        assert (x > 1.0).any() and (prod["rgba8"][..., :3] == 255).any()
    if name in ("inf", "nan", "negative"):
        assert (~np.isfinite(x)).any(), "the frame holds the values the case is about"
    if name == "inf":
        assert np.isposinf(x).any() and (prod["rgba8"][..., :3][np.isposinf(x)] == 255).all()


# ---- marches across the horizon, past the segment ends -------------------------------
def _horizon_camera(u):
    """Pitched slightly down and rolled by 12 degrees: the horizon crosses the tile rows
    at a slant, with the spheres, the blend and the torus in view."""
    aim(u, (6.0, 1.0, 32.0), (-1.0, -2.5, -6.0))
    a = math.radians(12.0)
    x = np.array(list(u.camera.xAxis)[:3], np.float64)
    y = np.array(list(u.camera.yAxis)[:3], np.float64)
    for k in range(3):
        u.camera.xAxis[k] = math.cos(a) * x[k] + math.sin(a) * y[k]
        u.camera.yAxis[k] = -math.sin(a) * x[k] + math.cos(a) * y[k]


@pytest.mark.parametrize("bounces", [3, 5])
def test_downward_loop_switch(rm, oracle, gpu, bounces):
    u = rm.sweep_uniforms(60, 120, bounces, True, 0)
    _horizon_camera(u)
    counted, _ = _three(rm, oracle, u, f"horizon b={bounces}")
    # Reflected marches run past step 16 (the first segment end): against the same frame
    # without bounces a pixel's count grows by its 4 samples' reflected steps, 4 per bounce
    # normal and at most 32 steps of the two bounce shadows.  More than that plus 16 steps
    # for each of the 4 x bounces reflected marches leaves one march with more than 16.
    u0 = rm.sweep_uniforms(60, 120, 0, True, 0)
    _horizon_camera(u0)
    base = render(rm, u0, W, H, kernel=rm.RM_KERNEL_PIXEL)
    extra = counted["sdf_counts"].astype(np.int64) - base["sdf_counts"].astype(np.int64)
    assert extra.max() > 4 * (4 * bounces + 32) + 4 * bounces * 16, extra.max()
    # the horizon is in the frame, and not along a tile row: sky and floor in most rows
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_GBUFFER) as r:
        r.dispatch(u0)
        ids = r.read_gbuffer()["id"]
    sky = ids == -1
    rows = sky.any(axis=1) & (ids == 7).any(axis=1)
    # (pixel rows holding both: more than two of the sample kernel's 4-pixel tile rows; the
    # objects: more than a 4x4 tile's worth of pixels)
    assert rows.sum() > 8 and ((ids >= 0) & (ids != 7)).sum() > 16


# ---- the kernels that share the code ----------------------------------------------
def test_batched_gbuffer_and_pattern_kernels(rm, gpu):
    u = rm.sweep_uniforms(60, 120, 3, True, 0)
    _horizon_camera(u)
    u2 = rm.sweep_uniforms(20, 120, 3, True, 0)
    both = rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F

    def plain(v):
        with rm.Renderer(W, H, outputs=both) as r:
            r.dispatch(v)
            return r.read_rgba8(), r.read_rgba32f()

    ref, ref2 = plain(u), plain(u2)

    def same(got8, got32, want, what):
        np.testing.assert_array_equal(got8, want[0], err_msg=f"{what}: RGBA8")
        np.testing.assert_array_equal(got32.view(np.uint32), want[1].view(np.uint32), err_msg=f"{what}: RGBA32F")

    with rm.Renderer(W, H, outputs=both) as r:
        r.dispatch_frames([u, u2])
        same(r.read_frame_rgba8(0), r.read_frame_rgba32f(0), ref, "rm_dispatch_frames, frame 0")
        same(r.read_frame_rgba8(1), r.read_frame_rgba32f(1), ref2, "rm_dispatch_frames, frame 1")
    with rm.Renderer(W, H, outputs=both | rm.RM_OUT_GBUFFER) as r:
        r.dispatch(u)
        same(r.read_rgba8(), r.read_rgba32f(), ref, "G-buffer kernel")
    with rm.Renderer(W, H, outputs=both) as r:
        r.dispatch_pattern(u, rm.RM_PATTERN_REFERENCE)
        same(r.read_rgba8(), r.read_rgba32f(), ref, "rm_dispatch_pattern REFERENCE")
    # the kernels without supersampling: k_pixel, its batch and G-buffer forms, one sample at (0, 0)
    for v in (u, u2):
        v.AA = 0
    ref, ref2 = plain(u), plain(u2)
    with rm.Renderer(W, H, outputs=both) as r:
        r.dispatch_frames([u, u2])
        same(r.read_frame_rgba8(0), r.read_frame_rgba32f(0), ref, "rm_dispatch_frames without AA, frame 0")
        same(r.read_frame_rgba8(1), r.read_frame_rgba32f(1), ref2, "rm_dispatch_frames without AA, frame 1")
    with rm.Renderer(W, H, outputs=both | rm.RM_OUT_GBUFFER) as r:
        r.dispatch(u)
        same(r.read_rgba8(), r.read_rgba32f(), ref, "G-buffer kernel without AA")
