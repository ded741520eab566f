"""The word layout of a compiled scene table (rm_scene_compile: TABLE_WORDS words per entry,
then the exit header of EXIT_WORDS words) and one entry's distance in float64, for the CPU
tests of the host table compiler and of the kernels' object bounds (a helper, not a test)."""
import numpy as np

TABLE_WORDS, TW_TYPE, TW_BALL = 24, 0, 20
EX_VALID, EX_CX, EX_R, EX_NPLANES = 0, 1, 4, 7
EX_LIP, EX_NSLOTS, EX_EVAL_MASK, EX_PLANE_MASK, EX_SLOTS, EX_BOX, EXIT_WORDS = 24, 25, 26, 27, 28, 36, 42
PLANE = 5


def as_f32(w):
    return w.view(np.float32)


def sdf64(p, prim, blend):
    """One entry's distance in float64 (glsl:83-103, 115-121), q = swizzle(p - c)."""
    q = p - np.array(prim.center[:], np.float64)
    if prim.swizzle == 1:
        q = q[:, [0, 2, 1]]
    a = np.array(prim.param[:], np.float64)
    L = lambda v: np.sqrt((v * v).sum(-1))  # noqa: E731
    if prim.type == 0:
        return [L(q) - a[0]]
    if prim.type in (1, 2):
        d = np.abs(q) - a[:3]
        box = np.minimum(d.max(-1), 0.0) + L(np.maximum(d, 0.0))
        return [box] if prim.type == 1 else [box, L(q) - a[3]]  # a blend lies between the two
    if prim.type == 3:
        l2 = np.stack([L(q[:, [0, 2]]) - a[0], q[:, 1]], -1)
        return [L(l2) - a[1]]
    pa, ba = q - a[:3], a[3:6] - a[:3]
    h = np.clip((pa * ba).sum(-1) / (ba * ba).sum(), 0.0, 1.0)
    return [L(pa - ba * h[:, None]) - a[6]]
