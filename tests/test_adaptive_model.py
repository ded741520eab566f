"""The numpy flagging model (tests/adaptive_model.py) pinned on the CPU oracle's AA-off
frames: the counts below are what the rule of include/rm_api.h gives on
rm_sweep_uniforms(60, 120, 1, 0, 0), and the GPU tests compare rm_dispatch_adaptive's
mask with the same model.  No GPU needed."""
import numpy as np
import pytest

from adaptive_model import flag_mask

# (width, height, threshold) -> flagged pixels
COUNTS = {(130, 67, 0): 8657, (130, 67, 4): 4261, (130, 67, 8): 4175, (130, 67, 16): 4058,
          (130, 67, 32): 4002, (130, 67, 255): 0, (37, 23, 16): 562}

_frames = {}


def frame(rm, oracle, W, H):
    if (W, H) not in _frames:
        img = oracle.render(rm.sweep_uniforms(60, 120, 1, False, 0), W, H, want_counts=False)["rgba8"]
        img.setflags(write=False)
        _frames[(W, H)] = img
    return _frames[(W, H)]


@pytest.mark.parametrize("W,H,thr", sorted(COUNTS))
def test_counts_on_oracle_frames(rm, oracle, W, H, thr):
    m = flag_mask(frame(rm, oracle, W, H), thr)
    assert m.shape == (H, W) and m.dtype == np.uint8 and set(np.unique(m)) <= {0, 1}
    assert int(m.sum()) == COUNTS[(W, H, thr)], (W, H, thr, int(m.sum()))


@pytest.mark.parametrize("thr", [0, 16, 255])
def test_one_pixel_has_no_neighbour(rm, oracle, thr):
    assert flag_mask(frame(rm, oracle, 1, 1), thr).sum() == 0
    assert flag_mask(np.full((1, 1, 4), 200, np.uint8), thr).sum() == 0


@pytest.mark.parametrize("thr", [0, 4, 16, 32])
def test_a_flagged_pixel_has_a_flagged_neighbour(rm, oracle, thr):
    m = flag_mask(frame(rm, oracle, 130, 67), thr).astype(bool)
    n = np.zeros_like(m)
    n[:, 1:] |= m[:, :-1]
    n[:, :-1] |= m[:, 1:]
    n[1:] |= m[:-1]
    n[:-1] |= m[1:]
    assert m.any() and (n[m]).all()


def test_rule_on_small_images():
    img = np.zeros((3, 4, 4), np.uint8)
    img[1, 2, 1] = 9  # one green pixel: it and its four neighbours differ by 9
    want = np.zeros((3, 4), np.uint8)
    for y, x in ((1, 2), (1, 1), (1, 3), (0, 2), (2, 2)):
        want[y, x] = 1
    assert (flag_mask(img, 8) == want).all()
    assert flag_mask(img, 9).sum() == 0  # strictly greater
    img[..., 3] = np.arange(12, dtype=np.uint8).reshape(3, 4) * 20  # alpha takes no part
    assert (flag_mask(img, 8) == want).all()
    assert flag_mask(np.zeros((2, 2, 4), np.uint8), 0).sum() == 0
