"""The scene tables of the tests, and the one resolver from a parametrised ID's name to its
table (a helper, not a test).  Importable without a device: `rm` is the rmarch module the
tests' fixture hands in."""
import ctypes as C

import numpy as np


def random_scene(rm, seed, nplanes=None):
    """Random table; nplanes fixes the number of plane entries (None: random types)."""
    g = np.random.default_rng(seed)
    n = int(g.integers(3, 13))
    types = [int(g.integers(0, 6)) for _ in range(n)]
    if nplanes is not None:
        types = [int(g.integers(0, 5)) for _ in range(n)] + [rm.PRIM_PLANE] * nplanes
        g.shuffle(types)
    prims = []
    for t in types:
        c = (float(g.uniform(-18, 18)), float(g.uniform(-3, 3)), float(g.uniform(-35, 0)))
        if t == rm.PRIM_SPHERE:
            par = (float(g.uniform(0.5, 4)),)
        elif t == rm.PRIM_BOX:
            par = tuple(float(x) for x in g.uniform(0.3, 3, 3))
        elif t == rm.PRIM_BLEND:
            par = tuple(float(x) for x in g.uniform(0.3, 3, 3)) + (float(g.uniform(0.5, 3)),)
        elif t == rm.PRIM_TORUS:
            par = (float(g.uniform(1, 3)), float(g.uniform(0.2, 0.8)))
        elif t == rm.PRIM_CAPSULE:
            par = tuple(float(x) for x in g.uniform(-2, 2, 6)) + (float(g.uniform(0.3, 1.5)),)
        else:
            nv = g.normal(size=3)
            nv[1] = abs(nv[1]) + 1.0
            if nplanes is not None and g.uniform() < 0.5:
                nv[1] = -nv[1]  # a ceiling: rays going up meet it, the miss exit must not fire
            nv /= np.linalg.norm(nv)
            c = (0.0, 0.0, 0.0)
            par = (float(nv[0]), float(nv[1]), float(nv[2]), float(g.uniform(4, 7)))
        prims.append(rm.primitive(
            t, c, par, tuple(float(x) for x in g.uniform(0, 1, 3)),
            id=int(g.choice([0, 1, 2, 5, 7, 7, 9])),
            material=float(g.choice([1.0, 1.0, 0.0])),
            swizzle=int(g.integers(0, 2)),
            paint=int(g.choice([0, 0, 1]))))
    return prims


def floor_last_scene(rm, seed):
    """A reference-shaped table (the specialised kernel's built-in-style march,
    rm_table.hip smarch): random bounded entries, then one axis-aligned floor
    plane q.y n_y + w as the last entry, n_y of either sign and not unit."""
    g = np.random.default_rng(1000 + seed)
    # 3..7 bounded entries (every one in a lazy slot): the 5- and 8-slot instances
    prims = random_scene(rm, seed, nplanes=0)[:3 + seed % 5]
    ny = float(g.choice([1.0, 0.5, 2.0, -1.0]))  # -1: a ceiling above the scene
    w = float(g.uniform(4, 7)) * abs(ny)
    prims.append(rm.primitive(rm.PRIM_PLANE, (0.0, 0.0, 0.0), (0.0, ny, 0.0, w), (0.5, 0.5, 0.5),
                              id=7, material=0.0, paint=1))
    return prims


def big_table(rm, n=30):
    """The reference scene's 5 objects repeated along x (40 units apart), one plane."""
    out = []
    for k in range(8):
        for p in rm.default_scene():
            if p.type == rm.PRIM_PLANE and k:
                continue
            q = rm.rm_primitive()
            C.memmove(C.byref(q), C.byref(p), C.sizeof(p))
            if q.type != rm.PRIM_PLANE:
                q.center[0] += 40.0 * k
            out.append(q)
    return out[:n]


def big_scene(rm):
    return (random_scene(rm, 4) + random_scene(rm, 5) + random_scene(rm, 6) + random_scene(rm, 7))[:30]


def scene_of(rm, name):
    """The table a parametrised ID names, with its own ids (id 7 carries the shadow rule), in
    every spelling the test files use: builtin (None: the built-in scene), default_table or
    default-table, random<k> or random-table (k = 0), floor<k> or floor-table (k = 0), planes<k>
    (random_scene(20 + k) with 1 + k planes), big30 (big_scene) and bigtable<nn> (big_table)."""
    if name == "builtin":
        return None
    if name in ("default_table", "default-table"):
        return rm.default_scene()
    if name == "big30":
        return big_scene(rm)
    if name.startswith("bigtable"):
        return big_table(rm, int(name[-2:]))
    k = 0 if name.endswith("-table") else int(name[-1])
    if name.startswith("random"):
        return random_scene(rm, k)
    if name.startswith("floor"):
        return floor_last_scene(rm, k)
    if name.startswith("planes"):
        return random_scene(rm, 20 + k, nplanes=1 + k)
    raise KeyError(f"no scene is called {name!r}")
