"""The accumulation rule on the CPU (include/rm_api.h RM_HAS_ACCUMULATION; oracle only): the
model of tests/accum_model.py, fed the oracle's colours of a 9 x 5 frame's GRID4 samples, gives
the sample-pattern model's pixel however the samples are split into calls (anchors 1 and 2),
keeps a first sample of -0.0, and writes (float)N into the sum image's w."""
import numpy as np
import pytest

import accum_model as AM
import sample_pattern_model as SPM
from uniforms import main_u

F = np.float32
W, H = 9, 5


@pytest.fixture(scope="module")
def grid4_colours(rm, oracle):
    """(16, H, W, 3): the oracle's castRay + render of every GRID4 sample, 2 bounces."""
    u = main_u(rm, 2)
    uvx, uvy = SPM.uv_table(*SPM.preset(SPM.GRID4), W, H)
    cols = np.empty((16, H, W, 3), F)
    for s in range(16):
        for py in range(H):
            for px in range(W):
                ro, rd = oracle.cast_ray(u, float(uvx[px, s]), float(uvy[py, s]))
                cols[s, py, px] = oracle.render_ray(u, ro, rd)
    cols.setflags(write=False)
    return cols


def same_bits(a, b):
    assert a.dtype == b.dtype == F and a.shape == b.shape
    nan = np.isnan(b)
    assert np.isnan(a[nan]).all() and (a.view(np.uint32) == b.view(np.uint32))[~nan].all()


@pytest.mark.parametrize("sizes", [[16], [4, 4, 4, 4], [1, 6, 9], [1] * 16], ids=["16", "4x4", "1+6+9", "16x1"])
def test_any_split_is_the_whole_patterns_pixel(grid4_colours, sizes):
    whole = SPM.pixel_sum(grid4_colours)
    acc, at = AM.Sum(), 0
    for k in sizes:
        acc.add(grid4_colours[at:at + k])
        at += k
        # after every call the frame is the prefix's pattern frame, and w is (float)N
        same_bits(acc.rgba32f(), SPM.pixel_sum(grid4_colours[:at]))
        assert acc.N == at and (acc.image()[..., 3] == F(at)).all()
    same_bits(acc.rgba32f(), whole)
    assert acc.frame()[0].tobytes() == SPM.quantize(whole).tobytes()
    same_bits(acc.image()[..., :3], acc.S)
    assert AM.run([grid4_colours[:5], grid4_colours[5:]]).N == 16


def test_the_splits_are_not_vacuous(grid4_colours):
    """The frame has pixels whose sum depends on the order, so a wrong order would show."""
    fwd = SPM.pixel_sum(grid4_colours)
    rev = SPM.pixel_sum(grid4_colours[::-1])
    assert (fwd.view(np.uint32) != rev.view(np.uint32)).any()


def test_restart_and_reset_start_from_the_first_sample(grid4_colours):
    acc = AM.run([grid4_colours[:7]])
    acc.add(grid4_colours[7:11], restart=True)
    same_bits(acc.rgba32f(), SPM.pixel_sum(grid4_colours[7:11]))
    assert acc.N == 4
    acc.reset()
    acc.add(grid4_colours[:1])
    same_bits(acc.rgba32f(), SPM.pixel_sum(grid4_colours[:1]))


def test_a_first_sample_of_minus_zero_stays_minus_zero():
    c = np.array([[-0.0, 0.0, -0.0]], F)
    acc = AM.Sum().add(c[None])
    assert np.signbit(acc.S).tolist() == [[True, False, True]]            # S = c_0, not 0 + c_0
    assert np.signbit(acc.rgba32f()[..., :3]).tolist() == [[True, False, True]]
    acc.add(c[None])  # -0 + -0 = -0, 0 + 0 = 0: still the stored sum first
    assert np.signbit(acc.S).tolist() == [[True, False, True]]
    acc.add(np.array([[[0.0, 0.0, 0.0]]], F))
    assert not np.signbit(acc.S).any()


def test_w_is_the_float_of_the_count():
    assert AM.count_f32(45) == F(45.0) and AM.count_f32(2**24) == F(2.0**24)
    # round to nearest even past 2^24: 2^24 + 1 is a tie and goes down, 2^24 + 3 goes up
    assert AM.count_f32(2**24 + 1) == F(2.0**24) and AM.count_f32(2**24 + 3) == F(2.0**24 + 4)
    acc = AM.Sum()
    for n in (1, 4, 7, 16, 1, 16):
        acc.add(np.ones((n, 2, 3), F))
    assert acc.N == 45 and (acc.image()[..., 3] == F(45.0)).all() and (acc.image()[..., :3] == F(45.0)).all()
    assert (acc.rgba32f() == F(1.0)).all()
