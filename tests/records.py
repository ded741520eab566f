"""Bit comparisons of query records, the ray sets of the ray-query tests and the oracle's
answers per ray (a helper, not a test).  Geometry is compared bit for bit as uint32, a NaN
equal to a NaN; colours within TOL (DESIGN §5's RGBA32F bar: pow is the only operation that
differs), NaN masks equal.  Importable without a device.

Ray sets (uniforms: tests/uniforms.py default_u unless a test says otherwise):
  aimed   7 unit rays from (0, 10, 15) at each object, the floor and the sky;
  random  1000 seeded rays through the scene's box (every object, the floor, misses);
  edge    rays outside the fast lanes' predicate or at its borders: rd = 0, NaN,
          1e30, 1e-3, 1e3 long; ro = 1e20, inf; on the floor; grazing it.
"""
import numpy as np

F32 = np.float32
NAN, INF = float("nan"), float("inf")
TOL = 2e-6


# ---- comparisons -----------------------------------------------------------------------
def bits_equal(a, b, what=""):
    """Equal as uint32; a NaN counts as equal to a NaN."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.shape == b.shape and a.dtype.itemsize == 4 and b.dtype.itemsize == 4, \
        f"{what}: shapes {a.shape} and {b.shape}, dtypes {a.dtype} and {b.dtype}: not the same array of 4-byte items"
    ua, ub = a.view(np.uint32), b.view(np.uint32)
    same = ua == ub
    if a.dtype.kind == "f" and b.dtype.kind == "f":
        same |= np.isnan(a) & np.isnan(b)
    bad = np.argwhere(~same)
    assert len(bad) == 0, f"{what}: {len(bad)} differ, first at {bad[0]}: {a[tuple(bad[0])]!r} vs {b[tuple(bad[0])]!r}"


def records_equal(got, want, fields, what):
    """Records with the same field names (rm_ray_hit, GBUFFER_DTYPE), field by field."""
    got, want = got.reshape(-1), want.reshape(-1)
    assert len(got) == len(want), f"{what}: {len(got)} records against {len(want)}"
    for f in fields:
        bits_equal(got[f], want[f], f"{what} {f}")


def hit_fields_equal(got, want, what):
    for f in ("t", "id", "material", "albedo"):
        bits_equal(got[f], want[f], f"{what} {f}")


def colors_close(got, want, what):
    got, want = np.asarray(got, F32), np.asarray(want, F32)
    assert (np.isnan(got) == np.isnan(want)).all(), f"{what}: NaN masks differ"
    fin = np.isfinite(want)
    assert (got[~fin & ~np.isnan(want)] == want[~fin & ~np.isnan(want)]).all(), f"{what}: infinities differ"
    err = np.abs(got[fin].astype(np.float64) - want[fin].astype(np.float64))
    print(f"{what}: max |colour error| {err.max() if err.size else 0.0:.3g} over {fin.sum()} values")
    assert (err <= TOL).all(), f"{what}: max error {err.max():.3g} > {TOL}"


def zeros(a):
    return not np.ascontiguousarray(a).view(np.uint32).any()


# ---- ray sets --------------------------------------------------------------------------
def _unit(d):
    d = np.asarray(d, np.float64)
    return (d / np.linalg.norm(d, axis=-1, keepdims=True)).astype(F32)


def aimed_rays():
    o = np.array([0, 10, 15], np.float64)
    targets = np.array([(15, 0, -10), (-25, 0, -10), (-5, 0, -10), (-2.5, 0, 10), (-4, 0, -29),
                        (3, -5.5, 3)], np.float64)
    d = np.concatenate([_unit(targets - o), np.array([[0, 1, 0]], F32)])
    return np.tile(o.astype(F32), (len(d), 1)), d


def random_rays():
    rng = np.random.default_rng(1)
    o = rng.uniform([-30, -5, -35], [20, 15, 20], (1000, 3)).astype(F32)
    d = _unit(rng.normal(size=(1000, 3)))
    return o, d


def edge_rays():
    rays = [((0, 10, 15), (0, 0, 0)),
            ((0, 10, 15), (NAN, 0, -1)),
            ((0, 0, 15), (0, 0, -1e30)),
            ((0, 0, 15), (0, 0, -1e-3)),
            ((0, 0, 15), (0, -1e3, -1e3)),
            ((1e20, 0, 0), (0, -1, 0)),
            ((INF, 0, 0), (0, -1, 0)),
            ((0, -5.5, 0), (1, 0, 0)),
            ((0, 100, 0), (1, -1e-4, 0))]
    return (np.array([r[0] for r in rays], F32), np.array([r[1] for r in rays], F32))


SETS = {"aimed": aimed_rays, "random": random_rays, "edge": edge_rays}
FLAG_SETS = [0, 1, 2, 3, 4, 6, 8]  # every valid combination of the RM_TRACE_* flags


_rays = {}


def gbuf_rays(oracle, u, W, H, aa):
    """Every pixel's G-buffer ray, [H * W, 3] origins and directions, row 0 the bottom row."""
    key = (bytes(u.camera), W, H, bool(aa))
    if key not in _rays:
        o, d = np.zeros((H, W, 3), F32), np.zeros((H, W, 3), F32)
        for py in range(H):
            for px in range(W):
                uvx = F32(px * 2 - W) / F32(W)  # glsl:301-305, in float32
                uvy = F32(py * 2 - H) / F32(H)
                if aa:  # the first sample's offsets (glsl:311-313)
                    uvx = F32(uvx + F32(0.25) / F32(W))
                    uvy = F32(uvy + F32(0.25) / F32(H))
                o[py, px], d[py, px] = oracle.cast_ray(u, float(uvx), float(uvy))
        o, d = o.reshape(-1, 3), d.reshape(-1, 3)
        o.setflags(write=False)
        d.setflags(write=False)
        _rays[key] = (o, d)
    return _rays[key]


def pixel_rays(oracle, u, W, H):
    """Every pixel's centre ray: the ray rm_pick casts, and the AA-off G-buffer's."""
    return gbuf_rays(oracle, u, W, H, False)


# ---- the oracle, per ray ---------------------------------------------------------------
_cache = {}


def oracle_march(rm, O, u, o, d, reflected):
    key = ("march", bytes(u), o.tobytes(), d.tobytes(), bool(reflected))
    if key not in _cache:
        out = np.zeros(len(o), rm.RAY_HIT_DTYPE)
        for i in range(len(o)):
            h, _ = O.raymarch(u, o[i], d[i], reflected)
            out[i]["t"], out[i]["id"], out[i]["material"] = h.hitpoint, h.id, h.material
            out[i]["albedo"] = tuple(h.color)
        out.setflags(write=False)
        _cache[key] = out
    return _cache[key]


def oracle_normals(O, u, o, d, t):
    n = np.zeros((len(o), 3), F32)
    for i in np.nonzero(t != F32(-1.0))[0]:
        with np.errstate(all="ignore"):
            pos = o[i] + d[i] * t[i]  # float32: a multiply then an add per component
        assert pos.dtype == F32, f"the hit point of ray {i} is {pos.dtype}, not float32"
        n[i] = O.get_normal(u, pos)
    return n


def oracle_colors(O, u, o, d):
    key = ("color", bytes(u), o.tobytes(), d.tobytes())
    if key not in _cache:
        c = np.array([O.render_ray(u, o[i], d[i]) for i in range(len(o))], F32).reshape(len(o), 3)
        c.setflags(write=False)
        _cache[key] = c
    return _cache[key]


def oracle_gbuffer(rm, O, u, W, H, aa=False):
    """The (H, W) G-buffer the frame owes: every pixel's ray (gbuf_rays) through raymarch, and
    get_normal at ro + rd * t in float32; a miss is t -1, id -1, zeros.  Read-only."""
    o, d = gbuf_rays(O, u, W, H, aa)
    hit = oracle_march(rm, O, u, o, d, False)
    g = np.zeros(W * H, rm.GBUFFER_DTYPE)
    g["t"], g["id"], g["albedo"] = hit["t"], hit["id"], hit["albedo"]
    g["normal"] = oracle_normals(O, u, o, d, g["t"])
    g.setflags(write=False)
    return g.reshape(H, W)
