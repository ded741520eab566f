"""The oracle's table-aware batch entry points (rmo_trace_rays, rmo_march_steps,
rmo_sdf_points), pinned on the CPU before tests/test_gpu_table_trace.py holds
k_table_trace to them:

  1. with no table rmo_trace_rays equals the per-ray entry points (rmo_raymarch,
     rmo_get_normal, rmo_softshadow, rmo_render_ray) bit for bit;
  2. rm_default_scene() as the table equals the built-in scene bit for bit, which ties
     the table path to what the reference shader pins;
  3. a SHADE trace of a frame's pixel rays equals rmo_render_scene's RGBA32F frame;
  4. tests/sdf_model.py equals rmo_sdf_points on random tables;
  5. the ray sets of tests/table_trace_rays.py meet their coverage conditions, stated
     on the oracle's answers alone, so a degenerate set fails before any GPU run.
"""
import numpy as np
import pytest

import sdf_model as M
import table_trace_rays as T
from records import (FLAG_SETS, INF, SETS, bits_equal, hit_fields_equal, oracle_colors, oracle_march, oracle_normals,
                     pixel_rays, records_equal, zeros)
from scenes import scene_of
from uniforms import default_u

F32 = np.float32
FIELDS = ("t", "id", "material", "albedo", "normal", "color")


def all_rays():
    o, d = zip(*(SETS[k]() for k in sorted(SETS)))
    return np.concatenate(o), np.concatenate(d)


# ---- 1. the batch form against the per-ray entry points ---------------------------------
@pytest.mark.parametrize("name", sorted(SETS))
@pytest.mark.parametrize("bounces", [0, 5])
@pytest.mark.parametrize("mode", [0, 1], ids=["soft", "hard"])
def test_batch_equals_per_ray(rm, oracle, name, bounces, mode):
    u = default_u(rm, bounces, mode)
    o, d = SETS[name]()
    for flags in FLAG_SETS:
        got = oracle.trace_rays(u, o, d, flags)
        what = f"{name} b{bounces} s{mode} flags {flags}"
        if flags == rm.RM_TRACE_SHADOW:
            k = INF if mode == rm.RM_SHADOW_HARD else 2.0
            want = np.array([oracle.softshadow(u, o[i], d[i], k)[0] for i in range(len(o))], F32)
            bits_equal(got["t"], want, what)
            assert all(zeros(got[f]) for f in FIELDS[1:]), what
            continue
        reflected = bool(flags & rm.RM_TRACE_REFLECTED)
        want = oracle_march(rm, oracle, u, o, d, reflected)
        hit_fields_equal(got, want, what)
        miss = want["t"] == F32(-1.0)
        assert (got["id"][miss] == -1).all() and (got["material"][miss] == 1.0).all() and zeros(got["albedo"][miss])
        if flags & rm.RM_TRACE_NORMAL:
            bits_equal(got["normal"], oracle_normals(oracle, u, o, d, want["t"]), f"{what} normal")
            assert zeros(got["normal"][miss])
        else:
            assert zeros(got["normal"])
        if flags & rm.RM_TRACE_SHADE:
            bits_equal(got["color"], oracle_colors(oracle, u, o, d), f"{what} color")
        else:
            assert zeros(got["color"])


def test_batch_arguments(rm, oracle):
    u = default_u(rm)
    o, d = SETS["aimed"]()
    for flags in (16, 1 << 31, 8 | 1, 8 | 2, 8 | 4, 4 | 1, 4 | 2 | 1):
        with pytest.raises(ValueError):
            oracle.trace_rays(u, o, d, flags)
    assert len(oracle.trace_rays(u, o[:0], d[:0])) == 0
    h, steps = zip(*(oracle.raymarch(u, o[i], d[i], r) for r in (False, True) for i in range(len(o))))
    got = np.concatenate([oracle.march_steps(u, o, d, r) for r in (False, True)])
    assert got.tolist() == list(steps)


# ---- 2. the default table against the built-in scene ------------------------------------
@pytest.mark.parametrize("itime", [0.0, 1.0, 4.5])
def test_default_table_equals_builtin(rm, oracle, itime):
    o, d = all_rays()
    for mode in (0, 1):
        u = default_u(rm, 2, mode)
        u.iTime = itime
        for flags in FLAG_SETS:
            records_equal(oracle.trace_rays(u, o, d, flags, scene=rm.default_scene()),
                          oracle.trace_rays(u, o, d, flags), FIELDS, f"iTime {itime} s{mode} flags {flags}")
    for r in (False, True):
        assert (oracle.march_steps(u, o, d, r, scene=rm.default_scene()) == oracle.march_steps(u, o, d, r)).all()
    pts = np.concatenate([M.seeded_points(), M.edge_points()])
    a, b = oracle.sdf_points(u, pts, rm.default_scene(), normal=True), oracle.sdf_points(u, pts, normal=True)
    for f in ("dist", "id", "winner", "normal"):
        bits_equal(a[f], b[f], f"iTime {itime} sdf_points {f}")
    want = M.oracle_records(rm, oracle, u, pts, normal=True)  # rmo_sdf / rmo_get_normal per point
    for f, g in (("dist", "t"), ("id", "id"), ("normal", "normal")):
        bits_equal(b[f], want[g], f"iTime {itime} sdf_points vs rmo_sdf {f}")


# ---- 3. consistency with rmo_render_scene -----------------------------------------------
@pytest.mark.parametrize("which", ["random0", "planes1", "floor0"])
def test_shade_trace_equals_the_frame(rm, oracle, which):
    scene = T.table(rm, which)
    u = rm.sweep_uniforms(60, 120, 2, False, 0)
    assert u.bounceVar == 2 and not u.AA
    W, H = 37, 23
    o, d = pixel_rays(oracle, u, W, H)
    got = oracle.trace_rays(u, o, d, rm.RM_TRACE_SHADE, scene=scene)
    img = oracle.render(u, W, H, scene=scene, want_counts=False)["rgba32f"]
    bits_equal(got["color"].reshape(H, W, 3), img[..., :3], which)
    assert len(set(got["id"].tolist())) >= 2, "the frame shows more than one id (a table's ids repeat)"


# ---- 4. tests/sdf_model.py against rmo_sdf_points ---------------------------------------
@pytest.mark.parametrize("which", ["random0", "random1", "random2", "random3", "floor0", "big30"])
def test_model_equals_the_oracle_on_tables(rm, oracle, which):
    scene = scene_of(rm, which)
    u = default_u(rm)
    pts = np.concatenate([M.seeded_points(), M.edge_points()])
    want = oracle.sdf_points(u, pts, scene, normal=True)
    got = M.sdf_records(rm, scene, 1.0, pts, normal=True)
    bits_equal(got["t"], want["dist"], f"{which} distance")
    bits_equal(got["id"], want["id"], f"{which} id")
    bits_equal(got["normal"], want["normal"], f"{which} normal")
    _, k = M.sdf_table(scene, 1.0, pts)
    assert (k == want["winner"]).all(), f"{which} winner"
    assert (np.array([p.id for p in scene], np.int32)[want["winner"]] == want["id"]).all()


# ---- 5. conditions on the ray sets of test_gpu_table_trace.py ---------------------------
_cov = {}


def coverage(rm, oracle, name):
    """Per march kind, over the rays inside trace_fast_ok: hits at t > 0, misses, rays at
    the step cap, and the winning entries (ids rewritten to 100 + entry index)."""
    if name not in _cov:
        scene = T.indexed(rm, T.table(rm, name))
        o, d, _ = T.rays(rm, oracle, name)
        fast = T.fast_ok(o, d)
        u = T.placement_uniforms(rm)
        out = {"n": int(fast.sum()), "winners": set()}
        for kind, flags, cap in (("raymarch", 0, 512), ("reflected", 1, 256)):
            h = oracle.trace_rays(u, o, d, flags, scene=scene)[fast]
            steps = oracle.march_steps(u, o, d, bool(flags), scene=scene)[fast]
            hit = h["t"] > 0
            miss = h["t"] == F32(-1.0)
            out[kind] = (int(hit.sum()), int(miss.sum()), int((steps == cap).sum()))
            out["winners"] |= set((h["id"][h["id"] >= 100] - 100).tolist())
        _cov[name] = out
    return _cov[name]


@pytest.mark.parametrize("name", T.TABLES)
def test_ray_set_conditions_per_table(rm, oracle, name):
    o, d, grp = T.rays(rm, oracle, name)
    assert len(o) == T.NRAYS == 1065 and len(o) % 64 != 0
    fast = T.fast_ok(o, d)
    by = {g: fast[grp == i] for i, (g, _) in enumerate(T.GROUPS)}
    assert all(by[g].all() for g in ("free", "inside", "far", "grazing", "axis")), "inside the predicate"
    # scaled: a float32 unit vector's rd.rd is 1 to a few ulps, so times 2^-12 or 2^12 it
    # lands on either side of the border; the other six scales are well inside
    at_border = np.isin(np.arange(128) % len(T.SCALES), (0, len(T.SCALES) - 1))
    assert by["scaled"][~at_border].all()
    assert not by["border"][:16].any() and not by["border"][16:24].any() and by["border"][24:].all()
    assert by["edge"].tolist() == [False, False, False, True, True, False, False, True, True]
    c = coverage(rm, oracle, name)
    print(name, c)
    for kind in ("raymarch", "reflected"):
        hit, miss, cap = c[kind]
        assert hit >= 0.03 * c["n"], (kind, "hits at t > 0", hit, c["n"])
        assert miss >= 0.03 * c["n"], (kind, "misses", miss, c["n"])
        assert cap >= 10, (kind, "rays at the step cap", cap)


def test_ray_set_conditions_over_all_tables(rm, oracle):
    cov = {name: coverage(rm, oracle, name) for name in T.TABLES}
    n = sum(c["n"] for c in cov.values())
    for kind in ("raymarch", "reflected"):
        assert sum(c[kind][0] for c in cov.values()) >= 0.25 * n, (kind, "hits")
        assert sum(c[kind][1] for c in cov.values()) >= 0.25 * n, (kind, "misses")
    types = set()
    for name, c in cov.items():
        scene = T.table(rm, name)
        types |= {int(scene[k].type) for k in c["winners"]}
    assert types == {0, 1, 2, 3, 4, 5}, types
    assert sum(len(c["winners"]) >= 4 for c in cov.values()) >= 5
    # the two border scales fall on both sides of the predicate
    for k in (0, len(T.SCALES) - 1):
        side = np.concatenate([T.fast_ok(*T.rays(rm, oracle, name)[:2])[T.rays(rm, oracle, name)[2] == 5]
                               [np.arange(128) % len(T.SCALES) == k] for name in T.TABLES])
        assert side.any() and not side.all(), f"scale {T.SCALES[k]}: both sides of the border"


def test_permutation_mixes_the_waves(rm, oracle):
    """Every wave of the permuted order holds fast lanes and literal-path lanes of
    several groups."""
    for name in T.TABLES:
        o, d, grp = T.rays(rm, oracle, name)
        p = T.permutation(name)
        assert sorted(p.tolist()) == list(range(T.NRAYS))
        waves = [p[i:i + 64] for i in range(0, T.NRAYS, 64)]
        assert all(len(set(grp[w].tolist())) >= 4 for w in waves)
        lit = ~T.fast_ok(o, d)
        assert sum(bool(lit[w].any() and not lit[w].all()) for w in waves) >= len(waves) // 3
