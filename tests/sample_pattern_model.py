"""A numpy float32 model of sample patterns (include/rm_api.h RM_HAS_SAMPLE_PATTERN): the
presets, the uv rule, the pixel's sum and the RGBA8 quantisation, written from the
header's text and independent of librm.  Every operation is one float32 operation in the
header's order (numpy float32 arithmetic is IEEE single precision, without FMA)."""
import numpy as np

F = np.float32
MAX_SAMPLES = 16
CUMULATIVE = 1
REFERENCE, GRID2, RGSS, GRID3, GRID4 = range(5)


def _grid(v):
    """{v}^2, x fastest."""
    m = len(v)
    return [v[i] for _ in range(m) for i in range(m)], [v[j] for j in range(m) for _ in range(m)]


def preset(k):
    """(flags, dx, dy) of preset k; n = len(dx)."""
    if k == REFERENCE:
        return CUMULATIVE, [.125, .375, .125, .375], [.125, .125, .375, .375]
    if k == GRID2:
        return (0,) + _grid([-.25, .25])
    if k == RGSS:
        return 0, [.125, -.375, .375, -.125], [.375, .125, -.125, -.375]
    if k == GRID3:
        return (0,) + _grid([-.34375, 0.0, .34375])
    if k == GRID4:
        return (0,) + _grid([-.375, -.125, .125, .375])
    raise ValueError(k)


def uv_axis(d, cumulative, dim):
    """The uv of every column (or row) of a `dim`-pixel axis under offsets d: (dim, n) float32."""
    dimf = F(dim)
    off = [(F(2.0) * F(x)) / dimf for x in d]
    i = np.arange(dim, dtype=np.int64)
    v0 = (2 * i - dim).astype(F) / dimf  # |2 i - dim| <= 2^16: the conversion is exact
    out = np.empty((dim, len(d)), F)
    v = v0
    for s, o in enumerate(off):
        v = (v if cumulative else v0) + o
        out[:, s] = v
    assert out.dtype == F
    return out


def uv_table(flags, dx, dy, W, H):
    cum = bool(flags & CUMULATIVE)
    return uv_axis(dx, cum, W), uv_axis(dy, cum, H)


def pixel_sum(cols):
    """cols: (n, ..., 3) float32 sample colours in sample order -> (..., 4) RGBA32F."""
    cols = np.asarray(cols, F)
    n = cols.shape[0]
    with np.errstate(all="ignore"):
        acc = cols[0].copy()
        for s in range(1, n):
            acc = acc + cols[s]
        out = acc / F(n)
    assert out.dtype == F
    return np.concatenate([out, np.ones(out.shape[:-1] + (1,), F)], axis=-1)


def quantize(rgba32f):
    """round(clamp(c, 0, 1) * 255) as the kernels store it: NaN -> 0, (uint)(v * 255 + 0.5)."""
    c = np.asarray(rgba32f, F)
    with np.errstate(invalid="ignore"):
        v = np.where(c > 0, np.where(c < 1, c, F(1.0)), F(0.0)).astype(F)
    return (v * F(255.0) + F(0.5)).astype(np.uint32).astype(np.uint8)
