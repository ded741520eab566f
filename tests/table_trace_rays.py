"""The tables and ray sets of the table ray-query tests (a helper, not a test).

tests/test_oracle_trace.py states the conditions the sets must meet on the oracle's
answers alone; tests/test_gpu_table_trace.py sends them at k_table_trace.  One
seeded generator per table, 1,065 rays: 16 full waves and a ragged one.  Origins are
placed with the oracle's rmo_sdf_points at the default uniforms with iTime = 1.

  free     384  origins uniform in the box (-30, -8, -45)..(30, 20, 12) with sdf > 0.25,
                random unit directions;
  inside   128  an entry's centre (a plane's foot point) plus N(0, 0.5): d < 0 or d ~ 0
                at t = 0, under a plane or inside a solid; random unit directions;
  far      128  30 to 1,600 units from an entry's centre, log-uniform, aimed at it with
                2 units of jitter: outside the exit ball, with large slack;
  grazing  128  outside origins aimed 2 to 6 units off an entry's centre;
  axis     128  outside origins, directions +-x, +-y, +-z and (+-1, 0, +-1), exactly;
  scaled   128  the first 128 rays with rd times 2^-12, 2^-11, 2^-6, 2^-3, 2^3, 2^6,
                2^11, 2^12: both borders of trace_fast_ok exactly;
  border    32  just outside it: |rd| = 2^-12 (1 - 2^-10), 2^12 (1 + 2^-10), and |ro|_1
                one step above and below 2^20, aimed at the scene;
  edge       9  tests/records.py edge_rays(): zero, NaN, huge and infinite rays.
"""
import ctypes as C

import numpy as np

from records import edge_rays
from scenes import scene_of as table  # T.table(rm, name): the table of that name, with its own ids
from uniforms import default_u

F32 = np.float32

TABLES = (["random%d" % s for s in range(4)] + ["planes%d" % s for s in range(4)] +
          ["floor0", "floor1", "bigtable30", "bigtable32"])
GROUPS = [("free", 384), ("inside", 128), ("far", 128), ("grazing", 128), ("axis", 128),
          ("scaled", 128), ("border", 32), ("edge", 9)]
NRAYS = sum(n for _, n in GROUPS)
SCALES = [2.0 ** e for e in (-12, -11, -6, -3, 3, 6, 11, 12)]
AXES = np.array([(1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1),
                 (1, 0, 1), (1, 0, -1), (-1, 0, 1), (-1, 0, -1)], F32)
BOX_LO, BOX_HI = (-30.0, -8.0, -45.0), (30.0, 20.0, 12.0)

_rays = {}


def indexed(rm, scene):
    """A copy with every id rewritten to 100 + entry index: a wrong winner cannot hide
    behind a repeated id."""
    out = []
    for k, p in enumerate(scene):
        q = rm.rm_primitive()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
        q.id = 100 + k
        out.append(q)
    return out


def placement_uniforms(rm):
    return default_u(rm)


def fast_ok(o, d):
    """trace_fast_ok (rm_trace.hpp) in float32: |ro|_1 <= 2^20 and 2^-24 <= rd.rd <= 2^24."""
    with np.errstate(all="ignore"):
        ro1 = (np.abs(o[:, 0]) + np.abs(o[:, 1])) + np.abs(o[:, 2])
        dd = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        assert ro1.dtype == F32 and dd.dtype == F32
        return (ro1 <= F32(2.0 ** 20)) & (dd >= F32(2.0 ** -24)) & (dd <= F32(2.0 ** 24))


def _unit(v):
    v = np.asarray(v, np.float64)
    return (v / np.linalg.norm(v, axis=-1, keepdims=True)).astype(F32)


def _centres(scene):
    """Each entry's centre; for a plane (centre 0) the foot point -w n of the origin."""
    out = []
    for p in scene:
        c = np.array(list(p.center), np.float64)
        if p.type == 5:
            n = np.array(list(p.param)[:3], np.float64)
            c = c - n * float(p.param[3]) / float(n @ n)
        out.append(c)
    return np.array(out)


def rays(rm, oracle, name):
    """(origins, dirs, group) of the table's set, float32 (NRAYS, 3) twice and the group
    index of each ray.  Computed once per table, read-only."""
    if name in _rays:
        return _rays[name]
    scene = table(rm, name)
    u = placement_uniforms(rm)
    g = np.random.default_rng(7000 + TABLES.index(name))
    cen = _centres(scene)

    def outside(n):  # rejection sampling on the oracle's distance
        got = np.zeros((0, 3), F32)
        while len(got) < n:
            p = g.uniform(BOX_LO, BOX_HI, (4 * n, 3)).astype(F32)
            got = np.concatenate([got, p[oracle.sdf_points(u, p, scene)["dist"] > F32(0.25)]])
        return got[:n]

    def pick(n):
        return cen[g.integers(0, len(cen), n)]

    O, D = [], []
    # free
    O.append(outside(384))
    D.append(_unit(g.normal(size=(384, 3))))
    # inside
    O.append((pick(128) + g.normal(scale=0.5, size=(128, 3))).astype(F32))
    D.append(_unit(g.normal(size=(128, 3))))
    # far
    c = pick(128)
    r = np.exp(g.uniform(np.log(30.0), np.log(1600.0), (128, 1)))
    o = c + _unit(g.normal(size=(128, 3))).astype(np.float64) * r
    O.append(o.astype(F32))
    D.append(_unit(c + g.uniform(-2.0, 2.0, (128, 3)) - o))
    # grazing
    o = outside(128).astype(np.float64)
    c = pick(128)
    to = c - o
    side = np.cross(to, g.normal(size=(128, 3)))
    side /= np.linalg.norm(side, axis=1, keepdims=True)
    O.append(o.astype(F32))
    D.append(_unit(to + side * g.uniform(2.0, 6.0, (128, 1))))
    # axis
    O.append(outside(128))
    D.append(AXES[np.arange(128) % len(AXES)])
    # scaled
    O.append(O[0][:128])
    D.append(D[0][:128] * np.array(SCALES, F32)[np.arange(128) % len(SCALES)][:, None])
    # border
    bo = outside(16)
    bd = _unit(pick(16) - bo.astype(np.float64))
    bd[:8] *= F32(2.0 ** -12 * (1.0 - 2.0 ** -10))
    bd[8:] *= F32(2.0 ** 12 * (1.0 + 2.0 ** -10))
    big = np.zeros((16, 3), F32)
    ax = np.arange(16) % 3
    sign = np.where(np.arange(16) % 2, -1.0, 1.0)
    # |ro|_1 = 2^20 + 0.125 (one float32 step above) and 2^20 - 0.5, exactly
    big[np.arange(16), ax] = sign * np.where(np.arange(16) < 8, 2.0 ** 20, 2.0 ** 20 - 1.0)
    big[np.arange(16), (ax + 1) % 3] = np.where(np.arange(16) < 8, 0.125, 0.5)
    O += [bo, big]
    D += [bd, _unit(pick(16) - big.astype(np.float64))]
    # edge
    eo, ed = edge_rays()
    O.append(eo)
    D.append(ed)

    o, d = np.concatenate(O).astype(F32), np.concatenate(D).astype(F32)
    grp = np.repeat(np.arange(len(GROUPS)), [n for _, n in GROUPS])
    assert o.shape == d.shape == (NRAYS, 3) and len(grp) == NRAYS
    for a in (o, d, grp):
        a.setflags(write=False)
    _rays[name] = (o, d, grp)
    return _rays[name]


def permutation(name):
    """The seeded order that gives every wave a mix of the groups."""
    return np.random.default_rng(9000 + TABLES.index(name)).permutation(NRAYS)


def shadow_start_rays(u, o, d, hits, n=500):
    """The shadow rays render() casts (glsl:233-236) from the hit points of a
    HIT | NORMAL pass: ro = pos + 0.02 normal, rd = light - pos, unnormalised, all in
    float32.  The first n hits with a finite normal."""
    ok = (hits["t"] != F32(-1.0)) & np.isfinite(hits["normal"]).all(axis=1) & np.isfinite(hits["t"])
    i = np.nonzero(ok)[0][:n]
    with np.errstate(all="ignore"):
        pos = o[i] + d[i] * hits["t"][i][:, None]
        so = pos + hits["normal"][i] * F32(0.02)
        sd = np.array(list(u.light.position), F32)[None, :] - pos
    assert so.dtype == F32 and sd.dtype == F32
    return so, sd
