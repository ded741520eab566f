"""The flagging rule of rm_dispatch_adaptive_edges (include/rm_api.h) in numpy float32: a
pixel is flagged iff it and some 4-neighbour inside the frame satisfy a selected criterion.
Every float operation is one float32 operation in the header's order (numpy does not
contract a multiply and an add), the compares are the header's, so NaNs fall as there."""
import numpy as np

from adaptive_model import flag_mask

COLOR, ID, DEPTH, NORMAL, ALBEDO = 1, 2, 4, 8, 16
F32 = np.float32
BITS = {"ID": ID, "DEPTH": DEPTH, "NORMAL": NORMAL, "ALBEDO": ALBEDO}
# (width, height) -> flagged pixels per criterion alone, at depth_rel 0.05 and normal_cos 0.9, on the
# oracle's G-buffer of rm_sweep_uniforms(60, 120, 1, 0, 0) (tests/test_adaptive_edges_model.py)
COUNTS = {(130, 67): {"ID": 681, "DEPTH": 1921, "NORMAL": 376, "ALBEDO": 3624},
          (37, 23): {"ID": 189, "DEPTH": 439, "NORMAL": 134, "ALBEDO": 545},
          (9, 5): {"ID": 21, "DEPTH": 28, "NORMAL": 7, "ALBEDO": 37}}


def _pairs(g, edges, depth_rel, normal_cos, axis):
    """The geometric criteria for every pixel and its right (axis 1) or upper (axis 0) neighbour."""
    n = g.shape[axis]
    p, q = g.take(range(n - 1), axis), g.take(range(1, n), axis)
    f = np.zeros(p.shape, bool)
    hit = (p["t"] != F32(-1.0)) & (q["t"] != F32(-1.0))
    with np.errstate(all="ignore"):
        if edges & ID:
            f |= p["id"] != q["id"]
        if edges & DEPTH:
            f |= hit & (np.abs(p["t"] - q["t"]) > F32(depth_rel) * np.fmin(p["t"], q["t"]))
        if edges & NORMAL:
            a, b = p["normal"], q["normal"]
            dot = (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]
            assert dot.dtype == F32
            f |= hit & (dot < F32(normal_cos))
        if edges & ALBEDO:
            f |= (p["albedo"] != q["albedo"]).any(axis=-1)
    return f


def edge_mask(gbuf, rgba8, edges, color_threshold=8, depth_rel=0.05, normal_cos=0.9) -> np.ndarray:
    """gbuf: (H, W) records with fields t (f4), id (i4), normal (3 f4), albedo (3 f4), or None
    under COLOR alone; rgba8: (H, W, 4) uint8, read under COLOR.  Returns the (H, W) 0 / 1 mask."""
    shape = gbuf.shape if gbuf is not None else rgba8.shape[:2]
    m = np.zeros(shape, bool)
    if edges & (ID | DEPTH | NORMAL | ALBEDO):
        dx = _pairs(gbuf, edges, depth_rel, normal_cos, 1)
        dy = _pairs(gbuf, edges, depth_rel, normal_cos, 0)
        m[:, 1:] |= dx
        m[:, :-1] |= dx
        m[1:] |= dy
        m[:-1] |= dy
    if edges & COLOR:
        m |= flag_mask(rgba8, color_threshold).astype(bool)
    return m.astype(np.uint8)
