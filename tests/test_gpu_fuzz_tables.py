"""GPU parity of runtime scene tables under seeded random uniforms: the tables of
tests/scenes.py (random entries of every type, with and without extra planes,
and reference-shaped floor-last tables) seen from the random cameras and lights
of test_gpu_fuzz_uniforms.py.

Each case: the generic table kernel's counting build against the oracle's table
mode (test_gpu_parity's bar) and its production build equal to the counting
build; for the first few cases, the hiprtc-specialised kernels (rm_jit.hip)
equal to the generic kernel bit for bit, counters and sdf counts included.
"""
import os

import numpy as np
import pytest

from frames import compare, render, same
from scenes import floor_last_scene, random_scene
from uniforms import CASES as UCASES, H, W, _uniforms

pytestmark = pytest.mark.gpu

# RM_FUZZ_TABLES widens the run
NTABLES = int(os.environ.get("RM_FUZZ_TABLES", "96"))
NSPEC = 6  # specialised cases: each compiles its table with hiprtc


def _case(rm, i):
    kind = i % 3
    if kind == 0:
        scene = random_scene(rm, 5000 + i)
    elif kind == 1:
        scene = random_scene(rm, 5000 + i, nplanes=1 + i % 4)
    else:
        scene = floor_last_scene(rm, 5000 + i)
    return scene, _uniforms(rm, UCASES[(7 * i) % len(UCASES)])


@pytest.mark.parametrize("i", range(NTABLES))
def test_random_tables_random_uniforms(rm, oracle, gpu, i):
    scene, u = _case(rm, i)
    ref = oracle.render(u, W, H, scene=scene)
    got = render(rm, u, W, H, scene=scene)
    compare(ref, got, f"table case {i}")
    prod = render(rm, u, W, H, scene=scene, counters=False)
    np.testing.assert_array_equal(prod["rgba32f"], got["rgba32f"], err_msg=f"table case {i}")
    np.testing.assert_array_equal(prod["rgba8"], got["rgba8"], err_msg=f"table case {i}")


@pytest.mark.parametrize("i", range(NSPEC))
def test_specialised_random_uniforms_equal_generic(rm, gpu, i):
    scene, u = _case(rm, i)
    for counters in (True, False):
        same(render(rm, u, W, H, scene, counters=counters, specialize=True),
             render(rm, u, W, H, scene=scene, counters=counters))
