"""GPU parity: librm's HIP kernels (through the C-ABI) vs the CPU oracle.

Bar:
  * geometry is bit-exact: per-pixel sdf() call counts and the frame counters
    (rays, march/reflect/shadow steps, normals, lights) equal the oracle's;
  * RGBA8 within +-1 LSB per channel (north_star allows +-2; the only source
    of difference is pow(): ocml powf on the GPU vs glibc powf in the oracle);
  * RGBA32F within RGBA32F_TOL absolute (a few float ULPs of colours <= ~2);
  * the production build (every proof-based early exit taken) gives the
    counting build's image bit for bit.
"""
import numpy as np
import pytest

from frames import compare, production_equals_counting, render

pytestmark = pytest.mark.gpu

# (frame, bounces, AA, shadow_mode) — frame -1 is the default start-up frame D.
CASES = [
    (-1, 0, True, 0),    # the reference's default interactive state (main.cpp:27,30)
    (-1, 0, False, 1),   # BASELINE cfg 1 (hard shadow), frame D
    (0, 0, False, 1),    # cfg 1, sweep
    (119, 0, False, 1),
    (0, 1, False, 0),    # cfg 2
    (60, 1, False, 0),
    (119, 1, False, 0),
    (30, 2, True, 0),
    (0, 3, True, 0),     # cfg 3
    (60, 3, True, 0),
    (119, 3, True, 0),
    (90, 4, False, 0),
    (60, 5, True, 0),    # cfg 4
    (0, 5, False, 1),
]


@pytest.mark.parametrize("case", CASES, ids=lambda c: f"f{c[0]}_b{c[1]}_aa{int(c[2])}_s{c[3]}")
@pytest.mark.parametrize("shape", [(96, 64), (100, 70)], ids=["96x64", "100x70"])
def test_parity_vs_oracle(rm, oracle, gpu, case, shape):
    f, b, aa, sm = case
    W, H = shape
    u = rm.sweep_uniforms(f, 120, b, aa, sm)
    ref = oracle.render(u, W, H)
    k = rm.RM_KERNEL_PIXEL
    got = render(rm, u, W, H, kernel=k)
    compare(ref, got, f"{shape} {case}")
    production_equals_counting(rm, u, W, H, k, got, f"{shape} {case}")


@pytest.mark.parametrize("shape", [(1, 1), (3, 1), (1, 5), (37, 23), (65, 3), (130, 67)])
def test_ragged_shapes(rm, oracle, gpu, shape):
    W, H = shape
    u = rm.sweep_uniforms(45, 120, 2, True, 0)
    ref = oracle.render(u, W, H)
    got = render(rm, u, W, H, kernel=rm.RM_KERNEL_PIXEL)
    compare(ref, got, f"shape {shape}")
    production_equals_counting(rm, u, W, H, rm.RM_KERNEL_PIXEL, got, f"shape {shape}")


def test_rgba8_is_quantized_rgba32f(rm, gpu):
    W, H = 128, 72
    u = rm.sweep_uniforms(10, 120, 3, True, 0)
    g = render(rm, u, W, H, kernel=rm.RM_KERNEL_AUTO, counters=False)
    np.testing.assert_array_equal(g["rgba8"], rm.quantize_rgba8(g["rgba32f"]))


def test_counter_mode_does_not_change_image(rm, gpu):
    W, H = 160, 90
    u = rm.sweep_uniforms(33, 120, 3, True, 0)
    a = render(rm, u, W, H, kernel=rm.RM_KERNEL_PIXEL, counters=True)
    b = render(rm, u, W, H, kernel=rm.RM_KERNEL_PIXEL, counters=False)
    np.testing.assert_array_equal(a["rgba32f"], b["rgba32f"])


# Uniforms the sweep never reaches: the light below the floor, inside or just
# above objects, far away; the camera inside primitives.  These exercise the
# proof-based shortcuts (lazy culling along rays, the softshadow early exit,
# rm_scene.hpp) where their bounds are tight or must refuse to fire.
STRESS = [
    ("light_default", None, None),
    ("light_below_floor", (0.0, -7.0, 0.0), None),
    ("light_on_floor", (3.0, -5.49, 2.0), None),
    ("light_in_sphere0", (15.0, 0.0, -10.0), None),
    ("light_above_blend", (-5.0, 2.6, -10.0), None),
    ("light_far", (300.0, 200.0, -400.0), None),
    ("light_zenith", (0.0, 1.0e4, 0.0), None),
    ("cam_in_torus_tube", None, (-7.5, 0.0, 10.0)),
    ("cam_in_blend", None, (-5.0, 0.0, -10.0)),
    ("cam_below_floor", None, (0.0, -8.0, 15.0)),
    ("cam_far", None, (40.0, 30.0, 120.0)),
    # floor hits beyond the int range: checkers' int() saturates
    ("cam_x_3e9", None, (3.0e9, 0.0, 15.0)),
    ("cam_x_-3e9", None, (-3.0e9, 0.0, 15.0)),
    ("cam_z_3e9", None, (0.0, 0.0, 3.0e9)),
    # the round-5 exit bounds at their edges (rm_scene.hpp lin_exit_b3 / b1p,
    # shadow_exit_init): the camera on and above the objects' slab y <= 3.001,
    # the light just inside and just outside the objects' ball (R_ALL = 23.001
    # around (-5, 0, -10)), and a low light far outside it
    ("cam_on_slab", None, (0.0, 3.0, 15.0)),
    ("cam_above_slab", None, (2.0, 6.0, 14.0)),
    ("light_ball_inside", (-5.0, 22.9, -10.0), None),
    ("light_ball_outside", (-5.0, 23.1, -10.0), None),
    ("light_low_far", (100.0, 1.0, 100.0), None),
]


@pytest.mark.parametrize("case", STRESS, ids=lambda c: c[0])
@pytest.mark.parametrize("bounces,aa,sm", [(3, True, 0), (1, False, 1)])
def test_stress_uniforms(rm, oracle, gpu, case, bounces, aa, sm):
    name, light, cam = case
    W, H = 80, 48
    u = rm.sweep_uniforms(20, 120, bounces, aa, sm)
    if light is not None:
        for i in range(3):
            u.light.position[i] = light[i]
    if cam is not None:
        for i in range(3):
            u.camera.pos[i] = cam[i]
    ref = oracle.render(u, W, H)
    k = rm.RM_KERNEL_PIXEL
    got = render(rm, u, W, H, kernel=k)
    compare(ref, got, name)
    production_equals_counting(rm, u, W, H, k, got, name)
