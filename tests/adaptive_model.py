"""The flagging rule of rm_dispatch_adaptive (include/rm_api.h) in numpy: a pixel is
flagged iff some 4-neighbour inside the frame differs from it by more than `threshold`
in R, G or B of the RGBA8 image.  Alpha takes no part."""
import numpy as np


def flag_mask(rgba8: np.ndarray, threshold: int) -> np.ndarray:
    """rgba8: (H, W, 4) uint8.  Returns the (H, W) uint8 mask of 0 / 1."""
    c = rgba8[..., :3].astype(np.int16)
    m = np.zeros(c.shape[:2], bool)
    dx = np.abs(c[:, 1:] - c[:, :-1]).max(axis=-1) > threshold  # a pixel and its right neighbour
    dy = np.abs(c[1:] - c[:-1]).max(axis=-1) > threshold        # a pixel and the one above
    m[:, 1:] |= dx
    m[:, :-1] |= dx
    m[1:] |= dy
    m[:-1] |= dy
    return m.astype(np.uint8)
