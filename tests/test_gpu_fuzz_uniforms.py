"""GPU parity on seeded random uniforms: cameras, view directions, lights, bounce
counts, AA and shadow modes the sweep and the stress list do not reach.

Each case: librm's counting build against the oracle (bit-exact geometry, RGBA8
within 1 LSB, RGBA32F within tolerance, NaN masks equal; test_gpu_parity's bar),
the production build (every proof-based early exit taken: the lazy culling
budgets, the ball / plane / slab / projection miss exits, the shadow exit,
rm_scene.hpp) equal to the counting build bit for bit, and finally every frame
once more through rm_dispatch_frames batches (k_sample_frames / k_pixel_frames,
the kernels bench.py times) equal to its single-frame image.

About a third of the cameras sit within 4 of a primitive's centre (some inside
it, where the reference itself yields NaN), a fifth of the lights are far away
(|light| ~ 1e3) and a fifth sit close to the objects.
"""
import numpy as np
import pytest

from frames import compare, render
from uniforms import CASES, NCASES, H, W, _uniforms

pytestmark = pytest.mark.gpu

_PROD = {}  # case index -> production image (RGBA32F, RGBA8), for the batch test


@pytest.mark.parametrize("i", range(NCASES))
def test_random_uniforms(rm, oracle, gpu, i):
    c = CASES[i]
    u = _uniforms(rm, c)
    ref = oracle.render(u, W, H)
    got = render(rm, u, W, H, kernel=rm.RM_KERNEL_PIXEL)
    compare(ref, got, f"case {i} {c}")
    prod = render(rm, u, W, H, kernel=rm.RM_KERNEL_PIXEL, counters=False)
    np.testing.assert_array_equal(prod["rgba32f"], got["rgba32f"], err_msg=f"case {i}")
    np.testing.assert_array_equal(prod["rgba8"], got["rgba8"], err_msg=f"case {i}")
    _PROD[i] = (prod["rgba32f"], prod["rgba8"])


@pytest.mark.parametrize("aa", [False, True], ids=["noaa", "aa"])
def test_random_uniforms_batched(rm, gpu, aa):
    idx = [i for i, c in enumerate(CASES) if c["aa"] == aa]
    assert idx
    us = [_uniforms(rm, CASES[i]) for i in idx]
    with rm.Renderer(W, H, outputs=rm.RM_OUT_RGBA8 | rm.RM_OUT_RGBA32F,
                     kernel=rm.RM_KERNEL_PIXEL, counters=False) as r:
        single = {}
        for i, u in zip(idx, us):
            if i in _PROD:
                single[i] = _PROD[i]
            else:  # test_random_uniforms deselected: render the frame alone here
                r.dispatch(u)
                single[i] = (r.read_rgba32f(), r.read_rgba8())
        for b0 in range(0, len(idx), rm.RM_MAX_BATCH):
            bi, bu = idx[b0:b0 + rm.RM_MAX_BATCH], us[b0:b0 + rm.RM_MAX_BATCH]
            r.dispatch_frames(bu)
            r.synchronize()
            for k, i in enumerate(bi):
                np.testing.assert_array_equal(r.read_frame_rgba32f(k), single[i][0],
                                              err_msg=f"batch frame {k} (case {i})")
                np.testing.assert_array_equal(r.read_frame_rgba8(k), single[i][1],
                                              err_msg=f"batch frame {k} (case {i})")
