"""The tests' own helper modules: no file imports a test module, and the shared comparers
refuse what they must.  Synthetic arrays and a stand-in context; no GPU, no oracle."""
import ast
import glob
import os
from types import SimpleNamespace

import numpy as np
import pytest

from adaptive_checks import check_frame, expected
from frames import RGBA8_TOL, RGBA32F_TOL, compare, same_frame
from records import bits_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
H, W = 3, 5


def test_no_file_imports_a_test_module():
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "tools", "*.py"))
    assert len(files) > 80
    bad = []
    for path in files:
        for node in ast.walk(ast.parse(open(path).read(), path)):
            names = ([a.name for a in node.names] if isinstance(node, ast.Import)
                     else [node.module or ""] if isinstance(node, ast.ImportFrom) else [])
            bad += [f"{os.path.relpath(path, ROOT)}:{node.lineno}: {n}" for n in names if n.split(".")[-1].startswith("test_")]
    assert not bad, "helpers live in tests/ modules whose names do not start with test_:\n" + "\n".join(bad)


def refuses(fn, *args, **kw):
    with pytest.raises(AssertionError):
        fn(*args, **kw)


def frame(seed=3):
    g = np.random.default_rng(seed)
    return g.integers(0, 256, (H, W, 4), dtype=np.uint8), g.random((H, W, 4), dtype=F32)


def flipped(a, at=(1, 2, 0)):
    """a with the lowest bit of one item flipped."""
    b = a.copy()
    b.view(np.uint32 if a.dtype.itemsize == 4 else np.uint8)[at] ^= 1
    return b


def bits_equal_cases():
    a = np.array([[1.5, -0.0, np.nan], [0.0, np.inf, -2.0]], F32)
    bits_equal(a, a.copy(), "equal, a NaN for a NaN")
    refuses(bits_equal, a, flipped(a, (0, 0)), "one bit")
    refuses(bits_equal, np.array([0.0], F32), np.array([-0.0], F32), "+0 against -0")
    refuses(bits_equal, a, np.where(np.isnan(a), F32(0.0), a), "a number for a NaN")
    refuses(bits_equal, a, a[:1], "shapes")
    i = np.array([1, -1, 7], np.int32)
    bits_equal(i, i.copy(), "integers")
    refuses(bits_equal, i, flipped(i, (2,)), "integers, one bit")


def same_frame_cases():
    f = frame()
    same_frame(f, (f[0].copy(), f[1].copy()), "equal")
    refuses(same_frame, (flipped(f[0]), f[1]), f, "one byte of rgba8")
    refuses(same_frame, (f[0], flipped(f[1])), f, "one bit of rgba32f")


def Ctx(M, c8, c32, G=None, count=None, outputs=None):
    """What check_frame reads of a context after an adaptive dispatch."""
    return SimpleNamespace(outputs=outputs or 3 | (4 if G is not None else 0), read_aa_mask=lambda: M,
                           aa_refined=lambda: int(M.sum()) if count is None else count,
                           read_rgba8=lambda: c8, read_rgba32f=lambda: c32, read_gbuffer=lambda: G)


def check_frame_cases():
    A, X = frame(1), frame(2)
    G = np.arange(H * W * 8, dtype=F32).reshape(H, W, 8)
    M = (np.arange(H * W).reshape(H, W) % 3 == 0).astype(np.uint8)
    w8, w32 = expected(M, A, X)
    assert w8[0, 0].tobytes() == X[0][0, 0].tobytes() and w8[0, 1].tobytes() == A[0][0, 1].tobytes()
    assert w32.dtype == np.uint32 and w32[0, 0].tobytes() == X[1][0, 0].tobytes()
    c32 = w32.view(F32)
    got = check_frame(Ctx(M, w8, c32, G), M, A, X, "right", G)
    assert got[0] is M and got[1] is w8 and got[2] is c32
    check_frame(Ctx(M, w8, c32), M, A, X, "a plain context, no G-buffer to compare")
    assert check_frame(Ctx(M, None, c32, outputs=2), M, A, X, "rgba32f only: rgba8 is not read")[1] is None
    refuses(check_frame, Ctx(M, flipped(w8), c32, G), M, A, X, "one byte of rgba8", G)
    refuses(check_frame, Ctx(M, w8, flipped(c32), G), M, A, X, "one bit of rgba32f", G)
    wrong = M.copy()
    wrong[1, 1] ^= 1
    refuses(check_frame, Ctx(wrong, w8, c32, G, count=int(M.sum())), M, A, X, "one mask byte", G)
    refuses(check_frame, Ctx(M * 2, w8, c32, G, count=int(M.sum())), M, A, X, "a mask that is not 0 / 1", G)
    refuses(check_frame, Ctx(M.astype(np.int8), w8, c32, G), M, A, X, "the mask's dtype", G)
    refuses(check_frame, Ctx(M, w8, c32, G, count=int(M.sum()) + 1), M, A, X, "the count", G)
    refuses(check_frame, Ctx(M, w8, c32, flipped(G)), M, A, X, "one G-buffer byte", G)


def render_of(seed=5):
    g = np.random.default_rng(seed)
    return {"rgba8": g.integers(2, 254, (H, W, 4), dtype=np.uint8), "rgba32f": g.random((H, W, 4), dtype=F32),
            "counters": {"rays": 15, "sdf_evals": 900}, "sdf_counts": g.integers(0, 99, (H, W)).astype(np.uint32)}


def changed(ref, key, fn):
    got = {k: (v.copy() if isinstance(v, np.ndarray) else dict(v)) for k, v in ref.items()}
    fn(got[key])
    return got


def compare_cases():
    ref = render_of()
    ref["rgba32f"][0, 0] = 0.0
    assert compare(ref, changed(ref, "rgba8", lambda a: None), "equal") == (0, 0.0)

    def add8(d):  # RGBA8: a difference of RGBA8_TOL = 1 either way, and of 2
        return lambda a: a.__setitem__((1, 2, 0), int(a[1, 2, 0]) + d)
    assert RGBA8_TOL == 1
    assert compare(ref, changed(ref, "rgba8", add8(1)), "rgba8 + 1")[0] == 1
    assert compare(ref, changed(ref, "rgba8", add8(-1)), "rgba8 - 1")[0] == 1
    refuses(compare, ref, changed(ref, "rgba8", add8(2)), "rgba8 + 2")
    refuses(compare, ref, changed(ref, "rgba8", add8(-2)), "rgba8 - 2")
    # RGBA32F: the float32 neighbours of RGBA32F_TOL = 2e-6, against a reference of 0
    assert RGBA32F_TOL == 2.0e-6
    t = F32(RGBA32F_TOL)
    under, over = (np.nextafter(t, F32(0)), t) if float(t) > RGBA32F_TOL else (t, np.nextafter(t, F32(1)))
    assert float(under) <= RGBA32F_TOL < float(over) and float(over) - float(under) < 1e-12

    def set32(v):
        return lambda a: a.__setitem__((0, 0, 1), v)
    assert compare(ref, changed(ref, "rgba32f", set32(under)), "just under the tolerance")[1] == float(under)
    assert compare(ref, changed(ref, "rgba32f", set32(-under)), "just under, below")[1] == float(under)
    refuses(compare, ref, changed(ref, "rgba32f", set32(over)), "just over the tolerance")
    refuses(compare, ref, changed(ref, "rgba32f", set32(-over)), "just over, below")
    # NaN and inf masks: exactly the oracle's
    with np.errstate(invalid="ignore"):
        for v in (np.nan, np.inf):
            refuses(compare, ref, changed(ref, "rgba32f", set32(v)), f"{v} where the reference is finite")
            bad = changed(ref, "rgba32f", set32(v))
            refuses(compare, bad, ref, f"finite where the reference is {v}")
            compare(bad, changed(bad, "rgba8", lambda a: None), f"{v} for {v}")
    # geometry is exact
    refuses(compare, ref, changed(ref, "sdf_counts", lambda a: a.__setitem__((2, 4), a[2, 4] + 1)), "one sdf count")
    refuses(compare, ref, changed(ref, "counters", lambda c: c.update(sdf_evals=901)), "one counter")


def test_the_comparers_reject_what_they_must():
    """The merged helpers' strictness: each case both accepted and refused as the files that
    use them rely on."""
    bits_equal_cases()
    same_frame_cases()
    check_frame_cases()
    compare_cases()
