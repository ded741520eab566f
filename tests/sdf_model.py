"""The expected values of SDF field queries on runtime scene tables (a helper, not a test).

This module restates table_entry, sdf_table and get_normal of oracle/rm_oracle.c
in vectorised numpy float32: one numpy operation per C operation, in the same
order (numpy's float32 + - * / sqrt are the IEEE operations and are never
contracted).  blend is libm's sinf through ctypes, gmin / gmax are the GLSL
selects, normalize is v * (1 / sqrt(dot)).  It was written when the oracle
exported rmo_sdf / rmo_get_normal for the built-in scene only.
tests/test_sdf_model.py pins it to those bit for bit on the default table, and
tests/test_oracle_trace.py to the oracle's own table sdf (rmo_sdf_points:
distance, id, winner and normal) on the random, floor-last and 30-entry tables
tests/test_gpu_sdf.py uses.
"""
import ctypes as C
import ctypes.util

import numpy as np

from records import bits_equal  # noqa: F401  (M.bits_equal: tests/test_sdf_model.py, tools/stress_sdf.py)

F32 = np.float32
_libm = C.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.sinf.restype = C.c_float
_libm.sinf.argtypes = [C.c_float]

SPHERE, BOX, BLEND, TORUS, CAPSULE, PLANE = range(6)
SWIZZLE_XZY = 1
PAINT_CHECKERS = 1


def blend_of(itime):
    """sinf(iTime) / 2 + 0.5 in float32 (rctx_init)."""
    return F32(F32(_libm.sinf(float(F32(itime)))) / F32(2.0)) + F32(0.5)


def gmin(x, y):
    return np.where(y < x, y, x)


def gmax(x, y):
    return np.where(x < y, y, x)


def dot3(ax, ay, az, bx, by, bz):
    return (ax * bx + ay * by) + az * bz


def length3(x, y, z):
    return np.sqrt(dot3(x, y, z, x, y, z))


def length2(x, y):
    return np.sqrt(x * x + y * y)


def glsl_int(x):
    """int(float) as the contract defines it: truncation, saturating, NaN -> 0."""
    with np.errstate(invalid="ignore"):
        r = np.where(x >= F32(2147483648.0), np.int64(2147483647),
                     np.where(x < F32(-2147483648.0), np.int64(-2147483648),
                              np.trunc(np.where(np.isfinite(x), x, F32(0.0))).astype(np.int64)))
    return np.where(np.isnan(x), np.int64(0), r)


def checkers(p):
    a = np.fmod(glsl_int(F32(1000.0) + p[:, 0]), 2)  # C's %: the sign of the dividend
    b = np.fmod(glsl_int(F32(1000.0) + p[:, 2]), 2)
    return np.where(a != b, F32(1.0), F32(0.2)).astype(F32)


def sd_box(qx, qy, qz, bx, by, bz):
    dx, dy, dz = np.abs(qx) - bx, np.abs(qy) - by, np.abs(qz) - bz
    z = F32(0.0)
    return gmin(gmax(dx, gmax(dy, dz)), z) + length3(gmax(dx, z), gmax(dy, z), gmax(dz, z))


def table_entry(P, blend, pos):
    """One entry's distance at pos (n, 3) float32."""
    c = [F32(v) for v in P.center]
    a = [F32(v) for v in P.param]
    qx, qy, qz = pos[:, 0] - c[0], pos[:, 1] - c[1], pos[:, 2] - c[2]
    if P.swizzle == SWIZZLE_XZY:
        qy, qz = qz, qy
    if P.type == SPHERE:
        return length3(qx, qy, qz) - a[0]
    if P.type == BOX:
        return sd_box(qx, qy, qz, a[0], a[1], a[2])
    if P.type == BLEND:
        bx = sd_box(qx, qy, qz, a[0], a[1], a[2])
        sp = length3(qx, qy, qz) - a[3]
        return bx * (F32(1.0) - blend) + sp * blend
    if P.type == TORUS:
        return length2(length2(qx, qz) - a[0], qy) - a[1]
    if P.type == CAPSULE:
        pax, pay, paz = qx - a[0], qy - a[1], qz - a[2]
        bax, bay, baz = a[3] - a[0], a[4] - a[1], a[5] - a[2]
        h = gmin(gmax(dot3(pax, pay, paz, bax, bay, baz) / dot3(bax, bay, baz, bax, bay, baz), F32(0.0)), F32(1.0))
        return length3(pax - bax * h, pay - bay * h, paz - baz * h) - a[6]
    return dot3(qx, qy, qz, a[0], a[1], a[2]) + a[3]


def sdf_table(scene, itime, pos):
    """(distance, winner's index) of the opU chain in table order at pos (n, 3)."""
    pos = np.ascontiguousarray(pos, F32)
    blend = blend_of(itime)
    with np.errstate(all="ignore"):
        d = table_entry(scene[0], blend, pos).astype(F32)
        k = np.zeros(len(pos), np.int64)
        for j in range(1, len(scene)):
            dj = table_entry(scene[j], blend, pos).astype(F32)
            keep = d < dj  # opU: (d1 < d2) ? d1 : d2
            d = np.where(keep, d, dj)
            k = np.where(keep, k, j)
    assert d.dtype == F32
    return d, k


def sdf_records(rm, scene, itime, pos, normal=False):
    """The RAY_HIT_DTYPE records rm_sdf_points owes for a table."""
    pos = np.ascontiguousarray(pos, F32)
    d, k = sdf_table(scene, itime, pos)
    out = np.zeros(len(pos), rm.RAY_HIT_DTYPE)
    out["t"] = d
    out["id"] = np.array([P.id for P in scene], np.int32)[k]
    out["material"] = np.array([P.material for P in scene], F32)[k]
    col = np.array([list(P.color) for P in scene], F32)[k]
    chk = checkers(pos)
    paint = np.array([P.paint for P in scene])[k] == PAINT_CHECKERS
    out["albedo"] = np.where(paint[:, None], chk[:, None], col)
    if normal:
        out["normal"] = get_normal(scene, itime, pos)
    return out


def get_normal(scene, itime, pos):
    pos = np.ascontiguousarray(pos, F32)
    e, z = F32(0.001), F32(0.0)
    with np.errstate(all="ignore"):
        cc = sdf_table(scene, itime, pos)[0]
        vx = sdf_table(scene, itime, pos + np.array([e, z, z], F32))[0] - cc
        vy = sdf_table(scene, itime, pos + np.array([z, e, z], F32))[0] - cc
        vz = sdf_table(scene, itime, pos + np.array([z, z, e], F32))[0] - cc
        inv = F32(1.0) / np.sqrt(dot3(vx, vy, vz, vx, vy, vz))
        n = np.stack([vx * inv, vy * inv, vz * inv], axis=1)
    assert n.dtype == F32
    return n


# ---- the point sets of the sdf tests, and the oracle per point (the built-in scene) -----
NAN, INF = float("nan"), float("inf")


def seeded_points():
    """2000 seeded points through the scene's box: every id, 186 of them inside an object."""
    return np.random.default_rng(7).uniform([-32, -7, -36], [22, 12, 16], (2000, 3)).astype(F32)


def edge_points():
    """Object centres, the floor with both zeros, far points whose gradient is exactly 0,
    the predicate's border on both sides, huge, infinite and NaN points; fast and
    literal lanes alternate, so they share a wave."""
    pts = [(15, 0, -10), (1e20, 0, 0), (-25, 0, -10), (INF, 0, 0), (-5, 0, -10), (NAN, 1, 2),
           (-5, 0, 10), (0, -1e30, 0), (-5, -2, -30), (3e38, 3e38, 3e38), (0, -5.5, 0),
           (0, 0, 2.0 ** 20 + 1), (-0.0, -5.5, -0.0), (2.0 ** 20, 0, 0), (1e5, 1e5, 1e5),
           (3e5, -2e5, 1e5)]
    return np.array(pts, F32)


_cache = {}


def oracle_records(rm, O, u, pos, normal=False):
    """The RAY_HIT_DTYPE records rm_sdf_points owes for the built-in scene: oracle.sdf and
    oracle.get_normal per point.  Computed once per (uniforms, points, flag), read-only."""
    pos = np.ascontiguousarray(pos, F32)
    key = (bytes(u), pos.tobytes(), bool(normal))
    if key not in _cache:
        out = np.zeros(len(pos), rm.RAY_HIT_DTYPE)
        for i in range(len(pos)):
            h = O.sdf(u, pos[i])
            out[i]["t"], out[i]["id"], out[i]["material"] = h.hitpoint, h.id, h.material
            out[i]["albedo"] = tuple(h.color)
            if normal:
                out[i]["normal"] = O.get_normal(u, pos[i])
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]

