"""Ray queries on runtime scene tables (k_table_trace) against
the oracle's per-ray table entry point, rmo_trace_rays.

Twelve tables (tests/table_trace_rays.py): random ones with and without planes,
ceilings, reference-shaped ones (whose frames take smarch and whose queries alone
take the production TLazy march) and two large ones, 32 entries among them.  Each
gets 1,065 seeded rays of every class a frame never casts: origins inside entries
and under planes, far outside the exit ball, grazing the culling balls, along the
axes, far from unit length, at and just outside the borders of trace_fast_ok, and
the zero / NaN / inf rays of the literal path.  tests/test_oracle_trace.py holds
the sets to their coverage conditions on the CPU.

The bar is k_trace's (test_gpu_trace.py): t, id, material, albedo, normals and
shadow factors bit for bit as uint32, a NaN equal to a NaN; colours within 2e-6
(DESIGN §5), NaN and inf masks equal.  Every set runs in two orders, grouped and
under a seeded permutation that mixes the groups (and literal-path lanes) into
every wave: per ray the two runs agree bit for bit, so the wave votes of the lazy
culling and of the loop-variant choices change work and never values.
"""
import numpy as np
import pytest

import table_trace_rays as T
from records import bits_equal, colors_close, hit_fields_equal, zeros
from uniforms import CASES, _uniforms, default_u

pytestmark = pytest.mark.gpu

F32 = np.float32
GEOMETRY = [0, 1, 2, 3]  # HIT, REFLECTED, NORMAL, NORMAL | REFLECTED
# a case of the uniform fuzz with a light of its own near the scene
MOVED = next(c for c in CASES if c["light"] is not None and max(abs(x) for x in c["light"]) < 100.0)


def uniforms(rm, which, bounces=0, mode=0):
    """"default": the defaults at iTime 1; "moved": a fuzz case's camera and light at
    iTime 4.5, so the blend entries move too."""
    if which == "default":
        u = default_u(rm)
    else:
        u = _uniforms(rm, MOVED)
        u.iTime = 4.5
        u.AA = 0
    u.bounceVar = bounces
    u.shadow_mode = mode
    return u


_cache = {}


def oracle_hits(oracle, u, o, d, flags, scene, key):
    """The oracle's answers, once per (table, uniforms, rays, flags), read-only."""
    key = (key, bytes(u), o.tobytes(), d.tobytes(), flags)
    if key not in _cache:
        h = oracle.trace_rays(u, o, d, flags, scene=scene)
        h.setflags(write=False)
        _cache[key] = h
    return _cache[key]


@pytest.fixture(scope="module")
def ctx(rm, gpu):
    with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA32F) as r:
        yield r


def both_orders(ctx, name, o, d, flags, what):
    """Trace grouped and permuted; the permuted run, put back in order, must equal the
    grouped one in every byte (colours included).  Returns the grouped run."""
    got = ctx.trace(o, d, flags)
    if len(o) == T.NRAYS:
        p = T.permutation(name)
    else:
        p = np.random.default_rng(len(o)).permutation(len(o))
    mixed = ctx.trace(np.ascontiguousarray(o[p]), np.ascontiguousarray(d[p]), flags)
    back = np.empty_like(mixed)
    back[p] = mixed
    bits_equal(back.view(np.uint32).reshape(-1, 12), got.view(np.uint32).reshape(-1, 12),
               f"{what}: grouped vs permuted order")
    return got


def check_geometry(rm, got, want, flags, what):
    for f in ("t", "id", "material", "albedo", "normal"):
        bits_equal(got[f], want[f], f"{what} {f}")
    miss = want["t"] == F32(-1.0)
    assert zeros(got["normal"][miss]), f"{what}: a miss has no normal"
    if not flags & rm.RM_TRACE_NORMAL:
        assert zeros(got["normal"]), what
    if not flags & rm.RM_TRACE_SHADE:
        assert zeros(got["color"]), what


# ---- 1. HIT, REFLECTED, NORMAL, NORMAL | REFLECTED: ids are 100 + entry index -----------
@pytest.mark.parametrize("which", ["default", "moved"])
@pytest.mark.parametrize("name", T.TABLES)
def test_geometry_bit_exact(rm, oracle, ctx, name, which):
    scene = T.indexed(rm, T.table(rm, name))
    u = uniforms(rm, which)
    o, d, _ = T.rays(rm, oracle, name)
    ctx.set_scene(scene)
    ctx.set_uniforms(u)
    for flags in GEOMETRY:
        what = f"{name} {which} flags {flags}"
        got = both_orders(ctx, name, o, d, flags, what)
        check_geometry(rm, got, oracle_hits(oracle, u, o, d, flags, scene, (name, "indexed")), flags, what)


# ---- 2. SHADOW --------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1], ids=["soft", "hard"])
@pytest.mark.parametrize("name", T.TABLES)
def test_shadow_bit_exact(rm, oracle, ctx, name, mode):
    scene = T.table(rm, name)
    ctx.set_scene(scene)
    o, d, _ = T.rays(rm, oracle, name)
    for which in ("default", "moved"):
        u = uniforms(rm, which, mode=mode)
        # and the shadow rays render() casts, from the hit points of a HIT | NORMAL pass
        hits = oracle_hits(oracle, u, o, d, rm.RM_TRACE_NORMAL, scene, name)
        so, sd = T.shadow_start_rays(u, o, d, hits)
        assert len(so) >= 100
        ao, ad = np.concatenate([o, so]), np.concatenate([d, sd])
        want = oracle_hits(oracle, u, ao, ad, rm.RM_TRACE_SHADOW, scene, name)
        distinct = len(np.unique(want["t"][~np.isnan(want["t"])]))
        assert distinct >= (3 if mode == 0 else 2), "the set exercises the shadow"
        ctx.set_uniforms(u)
        what = f"{name} {which} shadow s{mode}"
        got = both_orders(ctx, name, ao, ad, rm.RM_TRACE_SHADOW, what)
        bits_equal(got["t"], want["t"], what)
        for f in ("id", "material", "albedo", "normal", "color"):
            assert zeros(got[f]), (what, f)


def test_shadow_exit_at_a_tiny_table(rm, oracle, ctx):
    """table_exit_T's hmin = 0.001.  In the twelve tables the exits' slack,
    2^-12 (|ro|_1 + S) with S above 20, is ten times hmin and hides it.  One sphere of
    radius 0.01 at the origin has S = 1.01 and a slack of 2.5e-4: a ray that starts
    0.0003 to 0.001 above the sphere's top and goes up owes 0.05 (its first distance is
    below 0.001), and the y-slab's exit proves nothing there only because of hmin."""
    scene = [rm.primitive(rm.PRIM_SPHERE, (0.0, 0.0, 0.0), (0.01,), (0.5, 0.5, 0.5), id=3)]
    n = 192
    gap = np.tile(np.linspace(1e-4, 2.5e-3, n // 2).astype(F32), 2)
    g = np.random.default_rng(5)
    o = np.zeros((n, 3), F32)
    o[:, 1] = F32(0.01) + gap
    d = np.tile(np.array([0, 1, 0], F32), (n, 1))
    d[n // 2:, 0] = g.uniform(-0.3, 0.3, n // 2).astype(F32)  # the second half tilted, not unit
    d[n // 2:, 2] = g.uniform(-0.3, 0.3, n // 2).astype(F32)
    ctx.set_scene(scene)
    for mode in (0, 1):
        u = uniforms(rm, "default", mode=mode)
        want = oracle.trace_rays(u, o, d, rm.RM_TRACE_SHADOW, scene=scene)
        dark = want["t"] == F32(0.05)
        assert 20 <= dark[:n // 2].sum() <= n // 2 - 20 and 20 <= dark[n // 2:].sum() <= n // 2 - 20
        ctx.set_uniforms(u)
        got = both_orders(ctx, "random0", o, d, rm.RM_TRACE_SHADOW, f"tiny s{mode}")
        bits_equal(got["t"], want["t"], f"tiny sphere shadow s{mode}")


# ---- 3. SHADE: the tables' own ids (id 7 carries the shadow rule) -----------------------
@pytest.mark.parametrize("bounces", [0, 2, 5])
@pytest.mark.parametrize("mode", [0, 1], ids=["soft", "hard"])
@pytest.mark.parametrize("name", T.TABLES)
def test_shade(rm, oracle, ctx, name, mode, bounces):
    """Hit fields bit for bit, colours within colors_close's 2e-6.

    The scaled and border groups' longest rays (|rd| = 2^11, 2^12 and 2^12 (1 + 2^-10))
    have sky terms 0.6 - 0.2 rd.y, their own or a bounce's, up to 800, which leave the
    gamma as 4 to 21.  There one float ulp is 5e-7 to 1.9e-6: the bar allows powf's
    neighbour and nothing else.  With the frame kernels' pow (exp2(y log2 x) on the
    hardware transcendentals) six tables missed it by 2.9e-6 to 7.6e-6;
    the query kernels take the gamma of a linear colour above 16 in double
    (rm_scene.hpp gamma_pow) and the largest error is 4.8e-7."""
    scene = T.table(rm, name)
    ctx.set_scene(scene)
    o, d, _ = T.rays(rm, oracle, name)
    for which in ("default", "moved"):
        u = uniforms(rm, which, bounces, mode)
        ctx.set_uniforms(u)
        what = f"{name} {which} shade b{bounces} s{mode}"
        got = both_orders(ctx, name, o, d, rm.RM_TRACE_SHADE, what)
        want = oracle_hits(oracle, u, o, d, rm.RM_TRACE_SHADE, scene, name)
        hit_fields_equal(got, want, what)
        assert zeros(got["normal"]), what
        colors_close(got["color"], want["color"], what)


# ---- 4. rm_scene_specialize: queries stay on the generic code ---------------------------
def test_specialised_context_traces_the_same_bytes(rm, oracle, gpu):
    u = uniforms(rm, "default", 2)
    for name in ("random0", "floor0"):  # one hiprtc compile each
        scene = T.table(rm, name)
        o, d, _ = T.rays(rm, oracle, name)
        with rm.Renderer(37, 23, outputs=rm.RM_OUT_RGBA32F) as t:
            t.set_scene(scene)
            t.set_uniforms(u)
            before = {f: t.trace(o, d, f) for f in (rm.RM_TRACE_REFLECTED, rm.RM_TRACE_SHADE)}
            t.specialize_scene(True)
            for f, b in before.items():
                assert t.trace(o, d, f).tobytes() == b.tobytes(), f"{name} specialised, flags {f}"
