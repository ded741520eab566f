"""A numpy float32 model of progressive accumulation (include/rm_api.h RM_HAS_ACCUMULATION;
a helper, not a test): the running sum over a list of calls, (float)N, the frame and its
quantisation, the sum image with its w, and the Halton patterns in Python floats.  Written
from the header's text on top of tests/sample_pattern_model.py, with nothing of the kernels
in it: every operation is one float32 (for Halton: one double) operation in the header's
order; numpy's and Python's arithmetic is IEEE without FMA."""
import numpy as np

import sample_pattern_model as SPM

F = np.float32
RESTART = 1


def count_f32(N):
    """(float)N of the int64 count: numpy's int64 -> float32 cast rounds to nearest even."""
    return np.array(N, np.int64).astype(F)[()]


class Sum:
    """The context's two pieces of state, S (..., 3) float32 and N, and the rule's steps."""

    def __init__(self):
        self.S, self.N = None, 0

    def reset(self):
        self.N = 0

    def add(self, cols, restart=False):
        """One call: cols (n, ..., 3) float32, the samples' colours in pattern order."""
        cols = np.asarray(cols, F)
        n = cols.shape[0]
        if restart:
            self.N = 0
        with np.errstate(all="ignore"):
            if self.N == 0:
                S, first = cols[0].copy(), 1  # S = c_0, not 0 + c_0
            else:
                S, first = self.S, 0          # the stored sum first
            for s in range(first, n):
                S = S + cols[s]
        assert S.dtype == F
        self.S, self.N = S, self.N + n
        return self

    def rgba32f(self):
        """out = S / (float)N, alpha 1."""
        with np.errstate(all="ignore"):
            out = self.S / count_f32(self.N)
        assert out.dtype == F
        return np.concatenate([out, np.ones(out.shape[:-1] + (1,), F)], axis=-1)

    def frame(self):
        """(rgba8, rgba32f) as tests/frames.py images reads them."""
        f32 = self.rgba32f()
        return SPM.quantize(f32), f32

    def image(self):
        """The sum image: (S.r, S.g, S.b, (float)N)."""
        return np.concatenate([self.S, np.full(self.S.shape[:-1] + (1,), count_f32(self.N), F)], axis=-1)


def run(calls):
    """The state after `calls`, each the colours (n, ..., 3) of one call's samples."""
    acc = Sum()
    for cols in calls:
        acc.add(cols)
    return acc


def split(p, sizes, custom_pattern):
    """The absolute pattern p cut into consecutive patterns of `sizes` samples."""
    assert int(p.flags) == 0 and sum(sizes) == int(p.n)
    out, at = [], 0
    for k in sizes:
        out.append(custom_pattern(list(p.dx[at:at + k]), list(p.dy[at:at + k])))
        at += k
    return out


def prefix(p, k, custom_pattern):
    """The first k samples of the absolute pattern p."""
    assert int(p.flags) == 0 and 1 <= k <= int(p.n)
    return custom_pattern(list(p.dx[:k]), list(p.dy[:k]))


def colours(rm, oracle, r, u, p):
    """c_s of every pixel under uniforms u: (n, H, W, 3) float32, the uv from
    rm_pattern_uv_table, the rays from the oracle's castRay, the colours from context r's SHADE
    trace of those rays (as tests/patterns.py model takes them).  Leaves u as r's uniforms."""
    W, H, n = r.width, r.height, int(p.n)
    uvx, uvy = rm.pattern_uv_table(p, W, H)
    o, d = np.empty((n, H, W, 3), F), np.empty((n, H, W, 3), F)
    for s in range(n):
        for py in range(H):
            for px in range(W):
                o[s, py, px], d[s, py, px] = oracle.cast_ray(u, float(uvx[px, s]), float(uvy[py, s]))
    r.set_uniforms(u)
    return r.trace(o.reshape(-1, 3), d.reshape(-1, 3), rm.RM_TRACE_SHADE)["color"].reshape(n, H, W, 3)


# ---- the Halton patterns (rm_sample_pattern_halton), in Python floats (IEEE double) -------------
def radical_inverse(i, b):
    f = 1.0 / b
    r = 0.0
    while i > 0:
        term = float(i % b) * f  # the product and the sum are separate operations
        r = r + term
        i = i // b
        f = f / float(b)
    return r


def halton(first, n):
    """(dx, dy) float32 arrays of n samples from index `first`: i = first + s + 1."""
    dx = [F(radical_inverse(first + s + 1, 2) - 0.5) for s in range(n)]
    dy = [F(radical_inverse(first + s + 1, 3) - 0.5) for s in range(n)]
    return np.array(dx, F), np.array(dy, F)
