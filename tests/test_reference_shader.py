"""The oracle against the reference's own shader, run as C++ (oracle/_ref/glsl_ref).

oracle/rm_oracle.c is a hand restatement of the reference's compute shader; every
parity test of the kernels leans on it.  Here the arbiter is the shader's text
itself, compiled as C++20 against the reference's GLM (oracle/glsl_ref_main.cpp,
oracle/glsl_prelude.hpp; the built-ins are GLM's except those DESIGN.md §2
defines).  Everything is compared bit for bit (NaN against NaN, payload aside):

  * whole frames: the 24 fixture cases of tests/golden/reference_goldens.* and
    the first 64 seeded random uniforms of test_gpu_fuzz_uniforms at 67x41;
  * single functions (sdf, RayMarch, reflectedRay, GetNormal, softshadow, render,
    getPointLight, castRay) at the points where a restatement goes wrong;
  * the dispatch geometry: the frame does not depend on `workgroups`;
  * the oracle regenerates the committed reference frames (no binary needed: this
    one also runs where the reference tree, and so glsl_ref, is absent).
"""
import json
import math
import os

import numpy as np
import pytest

import glsl_ref as G
import uniforms as fuzz

HERE = os.path.join(os.path.dirname(__file__), "golden")
META = json.load(open(os.path.join(HERE, "reference_goldens.json")))
CASES = sorted(META["cases"])

needs_ref = pytest.mark.skipif(
    not G.available(),
    reason="oracle/_ref/glsl_ref does not exist: it is built from the reference tree, which is "
           "absent here (__graft_entry__.build() / `make glsl_ref` build it where it is present)")


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(HERE, "reference_goldens.npz"))


def _fixture_uniforms(rm, gold, name):
    return rm.rm_uniforms.from_buffer_copy(gold[name + "_uniforms"].tobytes())


def _assert_same_frame(a, b, label):
    """Equal as uint32 on every channel; NaN in the same channels (payload aside)."""
    assert a.shape == b.shape and a.dtype == b.dtype == np.float32, label
    np.testing.assert_array_equal(np.isnan(a), np.isnan(b), err_msg=f"{label}: NaN channels differ")
    bad = ~G.same_bits_or_nan(a, b)
    assert not bad.any(), (f"{label}: {int(bad.any(axis=-1).sum())} of {bad.shape[0] * bad.shape[1]} "
                           f"pixels differ, first at (row, col, channel) {np.argwhere(bad)[0]}")


# ---- fixtures: no binary needed -------------------------------------------------------
def test_fixture_metadata(gold):
    assert META["glm_version"] == "0.9.8.5"
    # DESIGN.md §3 lists these: every built-in that is not GLM's own
    assert META["overrides"] == ["mix", "min", "max", "clamp", "int"]
    assert "no report on 24 of 24 cases" in META["sanitizer"]
    assert len(CASES) == 24
    for name in CASES:
        m = META["cases"][name]
        assert gold[name + "_uniforms"].size == 168
        assert gold[name + "_rgba32f"].shape == (m["H"], m["W"], 4)
        assert int(np.isnan(gold[name + "_rgba32f"]).any(axis=2).sum()) == m["nan_pixels"]
    npz = os.path.join(HERE, "reference_goldens.npz")
    assert os.path.getsize(npz) <= os.path.getsize(os.path.join(HERE, "oracle_goldens.npz"))


@pytest.mark.parametrize("name", CASES)
def test_oracle_regenerates_reference_fixture(rm, oracle, gold, name):
    m = META["cases"][name]
    u = _fixture_uniforms(rm, gold, name)
    got = oracle.render(u, m["W"], m["H"], want_counts=False)["rgba32f"]
    _assert_same_frame(got, gold[name + "_rgba32f"], name)


# ---- whole frames ------------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("name", CASES)
def test_frame_fixture_case(rm, oracle, gold, name):
    m = META["cases"][name]
    u = _fixture_uniforms(rm, gold, name)
    ref = G.frame(u, m["W"], m["H"])
    _assert_same_frame(ref, gold[name + "_rgba32f"], f"{name}: glsl_ref vs its committed frame")
    got = oracle.render(u, m["W"], m["H"], want_counts=False)["rgba32f"]
    _assert_same_frame(got, ref, f"{name}: oracle vs glsl_ref")


@needs_ref
@pytest.mark.parametrize("i", range(64))
def test_frame_fuzz_case(rm, oracle, i):
    c = dict(fuzz.CASES[i], sm=0)  # the hard shadow is librm's extension: the shader has none
    u = fuzz._uniforms(rm, c)
    ref = G.frame(u, fuzz.W, fuzz.H)
    got = oracle.render(u, fuzz.W, fuzz.H, want_counts=False)["rgba32f"]
    _assert_same_frame(got, ref, f"fuzz case {i} {c}")


@needs_ref
def test_frame_refuses_hard_shadow(rm):
    u = rm.sweep_uniforms(20, 120, 1, False, rm.RM_SHADOW_HARD)
    p = G.frame_raw(u, 8, 8, check=False)
    assert p.returncode != 0 and b"shadow_mode" in p.stderr and not p.stdout


# ---- dispatch geometry ----------------------------------------------------------------------
@needs_ref
@pytest.mark.parametrize("shape", [(64, 40), (67, 41)], ids=["64x40", "67x41"])
def test_dispatch_geometry(rm, shape):
    """pixel = gl_WorkGroupID * workgroups + gl_LocalInvocationID: any tile edge, the same
    frame (64x40 is a whole number of 8x8 groups; 67x41 leaves partial groups)."""
    W, H = shape
    u = rm.sweep_uniforms(60, 120, 2, True, rm.RM_SHADOW_SOFT)
    one = G.frame_raw(u, W, H, 1).stdout
    assert len(one) == W * H * 16
    assert G.frame_raw(u, W, H, 8).stdout == one
    assert G.frame_raw(u, W, H, 5).stdout == one
    assert G.frame_raw(u, W, H).stdout == one  # the default edge


# ---- function probes -------------------------------------------------------------------------
SEED = 20261019
PI = math.pi
# the scene's constants as the oracle's KATs state them (tests/test_oracle_kats.py)
SPHERE0, SPHERE1, BLEND, TORUS = (15.0, 0.0, -10.0), (-25.0, 0.0, -10.0), (-5.0, 0.0, -10.0), (-5.0, 0.0, 10.0)
CAPSULE_A, CAPSULE_B = (-5.1, -1.9, -30.1), (-3.0, 2.0, -28.0)  # the segment's ends, radius 1
FLOOR_Y = -5.5
# uniform sets: (sweep frame, bounces, iTime or None for the sweep's own)
USETS = {
    "sweep20": (20, 3, None),
    "t0": (20, 0, 0.0),            # sin = 0: the blend weight is exactly 0.5
    "t0.5": (20, 1, 0.5),
    "t_half_pi": (20, 2, PI / 2),  # weight ~1: the sphere
    "t3": (20, 3, 3.0),
    "t_3half_pi": (20, 4, 1.5 * PI),  # weight ~0: the box
    "t10": (75, 5, 10.0),
    "t59.3": (100, 2, 59.3),
    "cam_in_blend": (20, 3, None),  # the camera at CAM_IN_BLEND: the view vector of a hit there is 0/0
}
CAM_IN_BLEND = (-5.5, 0.3, -9.6)


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def _f32(p):
    return tuple(float(x) for x in np.asarray(p, np.float32))


def _near(x):
    """x as float32 with its two float32 neighbours."""
    x = np.float32(x)
    return [float(np.nextafter(x, np.float32(-np.inf))), float(x), float(np.nextafter(x, np.float32(np.inf)))]


def _torus_surface(rng, n, r=0.5):
    """Points at distance r from the torus' centre circle (radius 2.5 in the world xy plane)."""
    a, b = rng.uniform(0, 2 * PI, n), rng.uniform(0, 2 * PI, n)
    ring = 2.5 + r * np.cos(b)
    return np.stack([TORUS[0] + ring * np.cos(a), TORUS[1] + ring * np.sin(a),
                     TORUS[2] + r * np.sin(b)], axis=1)


def _capsule_surface(rng, n, r=1.0):
    a, b = np.array(CAPSULE_A), np.array(CAPSULE_B)
    axis = (b - a) / np.linalg.norm(b - a)
    d = np.cross(_unit(rng, n), axis)
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    return a + rng.uniform(0, 1, (n, 1)) * (b - a) + r * d


def _build_probes():
    """-> {group: [(uniform set, function, args, note)]}, seeded."""
    rng = np.random.default_rng(SEED)
    g = {}

    def add(group, uset, fn, args, note=""):
        g.setdefault(group, []).append((uset, fn, _f32(np.ravel(args)), note))

    centres = {"sphere0": SPHERE0, "sphere1": SPHERE1, "blend": BLEND, "torus_hole": TORUS,
               "torus_tube": (-7.5, 0.0, 10.0), "capsule_a": CAPSULE_A, "capsule_b": CAPSULE_B,
               "capsule_mid": (-4.05, 0.05, -29.05), "floor": (2.0, FLOOR_Y, 3.0)}
    for name, c in centres.items():
        add("sdf_centres", "sweep20", G.P_SDF, c, name)
        add("normal_centres", "sweep20", G.P_NORMAL, c, name)
    # a surface point and an inside point of every primitive (sdf and its normal)
    surf, inside = [], []
    for c in (SPHERE0, SPHERE1, BLEND):
        d = _unit(rng, 6)
        surf += list(np.array(c) + 3.0 * d)
        inside += list(np.array(c) + rng.uniform(0.1, 2.4, (6, 1)) * d)
    surf += list(np.array(BLEND) + np.array([(3, 1, -1), (-3, 2, 2), (1, 2.5, 0), (0, -2.5, 2), (2, 1, 2.5),
                                             (3, 2.5, 2.5), (-3, -2.5, -2.5)], float))  # box faces, corners
    surf += list(_torus_surface(rng, 8))
    inside += list(_torus_surface(rng, 6, r=0.2))
    surf += list(_capsule_surface(rng, 8))
    inside += list(_capsule_surface(rng, 6, r=0.4))
    fl = rng.uniform(-40, 40, (8, 3))
    fl[:, 1] = FLOOR_Y
    surf += list(fl)
    fl = rng.uniform(-40, 40, (6, 3))
    fl[:, 1] = rng.uniform(-9.0, -5.6, 6)  # below the floor plane
    inside += list(fl)
    for p in surf:
        add("sdf_surface", "sweep20", G.P_SDF, p)
        add("normal_surface", "sweep20", G.P_NORMAL, p)
    for p in inside:
        add("sdf_inside", "sweep20", G.P_SDF, p)
        add("normal_inside", "sweep20", G.P_NORMAL, p)
    # opU ties: two primitives at exactly the same distance, both the nearest; the later one
    # of the chain wins (d1 < d2 ? d1 : d2).  Below a sphere / the torus ring / the blend
    # object (iTime 0: weight exactly 0.5) at the height where the floor is as far; all sums exact.
    ties = {"sphere0|floor": (15.0, -4.25, -10.0), "sphere1|floor": (-25.0, -4.25, -10.0),
            "torus|floor": (-5.0, -4.25, 10.0), "blend|floor": (-5.0, -4.125, -10.0)}
    for name, (x, y, z) in ties.items():
        for yy in _near(y):
            add("sdf_ties", "t0", G.P_SDF, (x, yy, z), name)
    # checkers: cell borders, also where 1000 + x is negative (int() truncates toward zero,
    # % gives -1, and -1 != 1 although both are odd); on the floor and just above it
    xs = [v for k in (-3.0, -1.0, 0.0, 1.0, 2.0, 7.0, -999.0, -1000.0, -1001.0, -1002.0, -1003.0) for v in _near(k)]
    xs += [-1000.5, -1001.5, -1002.5, -999.5, -2000.5, -2001.5, 0.5, 1.5, -0.5, -1.5]
    zs = [0.5, 1.5, -0.5, -1001.5, -1002.5, -1002.0]
    for x in xs:
        for z in (zs if abs(x) > 500 or x in (0.5, -0.5) else zs[:3]):
            add("sdf_checkers", "sweep20", G.P_SDF, (x, FLOOR_Y, z))
            add("sdf_checkers", "sweep20", G.P_SDF, (z, FLOOR_Y + 0.05, x))
    # the blend at several iTime: its centre, surface and inside points, the box's corner
    pts = [BLEND, (-2.0, 0.0, -10.0), (-5.0, 2.5, -10.0), (-5.0, 3.0, -10.0), (-2.0, 2.5, -7.5),
           (-8.0, -2.5, -12.5), (-4.0, 1.0, -9.0), (-5.0, 0.0, -6.9)] + list(np.array(BLEND) + 3.2 * _unit(rng, 4))
    for us in USETS:
        for p in pts:
            add("sdf_blend_itime", us, G.P_SDF, p)
        add("normal_blend_itime", us, G.P_NORMAL, pts[2])
        add("normal_blend_itime", us, G.P_NORMAL, pts[4])
    # rays ending on the step caps: level with the floor, a little above it, away from the
    # objects: the step is the height, so 512 (256) steps come long before anything else
    for h in (0.05, 0.1, 0.3, 0.7):
        for d in ((1.0, 0.0, 0.0), (0.6, 0.0, 0.8)):
            for fn in (G.P_RAYMARCH, G.P_REFLECTED):
                add("march_step_cap", "sweep20", fn, (60.0, FLOOR_Y + h, 40.0) + d, "cap")
    # rays ending on the escape test (a step longer than 400 / 200): up into the sky
    for d in _unit(rng, 10):
        d[1] = abs(d[1]) + 0.3
        d /= np.linalg.norm(d)
        for fn in (G.P_RAYMARCH, G.P_REFLECTED):
            add("march_escape", "sweep20", fn, np.concatenate([rng.uniform(-20, 20, 3) + (0, 25, 0), d]), "escape")
    # rays at every primitive from outside, and rays that start inside one (hit at t = 0)
    targets = [SPHERE0, SPHERE1, BLEND, (-7.5, 0.0, 10.0), (-4.05, 0.05, -29.05), (0.0, FLOOR_Y, 0.0)]
    for c in targets:
        for _ in range(4):
            ro = np.array(c) + rng.uniform(8, 30) * _unit(rng, 1)[0]
            ro[1] = abs(ro[1]) + 1.0
            d = np.array(c) + rng.uniform(-0.8, 0.8, 3) - ro
            d /= np.linalg.norm(d)
            for fn, us in ((G.P_RAYMARCH, "sweep20"), (G.P_REFLECTED, "t3")):
                add("march_hits", us, fn, np.concatenate([ro, d]))
            add("render_rays", "t10", G.P_RENDER, np.concatenate([ro, d]))
    for p in inside[:24:2]:
        d = _unit(rng, 1)[0]
        add("march_from_inside", "sweep20", G.P_RAYMARCH, np.concatenate([p, d]))
        add("march_from_inside", "sweep20", G.P_REFLECTED, np.concatenate([p, d]))
        add("render_rays", "sweep20", G.P_RENDER, np.concatenate([p, d]))
    # softshadow: its first step divides by t = 0; origins on the floor (some under the
    # objects), inside a primitive (0.05 at once) and within 0.001 of a surface
    light = np.array((0.0, 20.0, 0.0))
    for c in (SPHERE0, SPHERE1, BLEND, TORUS, (-4.05, 0.05, -29.05)):
        for _ in range(4):
            p = np.array(c) + rng.uniform(-6, 6, 3)
            p[1] = FLOOR_Y
            add("softshadow", "sweep20", G.P_SOFTSHADOW, np.concatenate([p + (0, 0.02, 0), light - p, [2.0]]))
    for p in rng.uniform(-40, 40, (10, 3)):
        p[1] = FLOOR_Y
        add("softshadow", "t3", G.P_SOFTSHADOW, np.concatenate([p + (0, 0.02, 0), light - p, [2.0]]))
    for p in inside[:12:3]:
        add("softshadow", "sweep20", G.P_SOFTSHADOW, np.concatenate([p, light - p, [2.0]]))
    for y in _near(FLOOR_Y + 0.001) + [FLOOR_Y + 0.0005, FLOOR_Y]:
        add("softshadow", "sweep20", G.P_SOFTSHADOW, (30.0, y, 30.0, -30.0, 25.5, -30.0, 2.0))
    # whole rays through render(): from the sweep's cameras, every bounce count
    for us in USETS:
        for d in _unit(rng, 6):
            d[1] = -abs(d[1]) * 0.5
            d /= np.linalg.norm(d)
            add("render_rays", us, G.P_RENDER, np.concatenate([(0.0, 2.0, 25.0) + rng.uniform(-3, 3, 3), d]))
    # getPointLight and castRay
    for p, n in zip(surf[:18:3], _unit(rng, 6)):
        add("point_light", "t10", G.P_POINTLIGHT, np.concatenate([rng.uniform(0, 1, 3), n, p]))
    for uv in rng.uniform(-1, 1, (6, 2)):
        add("cast_ray", "t59.3", G.P_CASTRAY, uv)
    # NaN through max(): at the camera's own position the view vector is normalize(0) = NaN,
    # and max(NaN, 0) is NaN under §2's form (0 under `x > y ? x : y`)
    for n in _unit(rng, 4):
        add("nan_through_max", "cam_in_blend", G.P_POINTLIGHT, np.concatenate([(0.5, 0.6, 0.7), n, CAM_IN_BLEND]))
        add("nan_through_max", "cam_in_blend", G.P_RENDER, np.concatenate([CAM_IN_BLEND, n]))
    return g


PROBES = _build_probes()
NPROBES = sum(len(v) for v in PROBES.values())


def _uset(rm, name):
    frame, bounces, itime = USETS[name]
    u = rm.sweep_uniforms(frame, 120, bounces, True, rm.RM_SHADOW_SOFT)
    if itime is not None:
        u.iTime = itime
    if name == "cam_in_blend":
        for i in range(3):
            u.camera.pos[i] = CAM_IN_BLEND[i]
    return u


@pytest.fixture(scope="module")
def probed(rm):
    """Every probe through glsl_ref, one process per uniform set: {(group, index): uint32[8]}."""
    out = {}
    for us in USETS:
        keys = [(grp, i) for grp, recs in PROBES.items() for i, r in enumerate(recs) if r[0] == us]
        if keys:
            res = G.probe(_uset(rm, us), [(PROBES[grp][i][1], PROBES[grp][i][2]) for grp, i in keys])
            out.update(zip(keys, res))
    return out


def _words(*floats, ints=()):
    w = np.zeros(8, np.uint32)
    f = np.asarray(floats, np.float32).ravel()
    w[:f.size] = f.view(np.uint32)
    for at, v in ints:
        w[at] = np.int32(v).view(np.uint32)
    return w


def _hit_words(h):
    return _words(h.hitpoint, *h.color, 0.0, h.material, ints=[(4, h.id)])


def _oracle_words(O, u, fn, a, note):
    p, q = a[0:3], a[3:6]
    if fn == G.P_SDF:
        return _hit_words(O.sdf(u, p))
    if fn in (G.P_RAYMARCH, G.P_REFLECTED):
        h, steps = O.raymarch(u, p, q, reflected=fn == G.P_REFLECTED)
        cap = 256 if fn == G.P_REFLECTED else 512
        if note == "cap":  # the case is what it claims to be
            assert steps == cap and h.hitpoint == -1.0, (steps, h.hitpoint)
        if note == "escape":
            assert steps < cap and h.hitpoint == -1.0, (steps, h.hitpoint)
        return _hit_words(h)
    if fn == G.P_NORMAL:
        return _words(O.get_normal(u, p))
    if fn == G.P_SOFTSHADOW:
        return _words(O.softshadow(u, p, q, a[6])[0])
    if fn == G.P_POINTLIGHT:
        return _words(O.point_light(u, p, q, a[6:9]))
    if fn == G.P_CASTRAY:
        ro, rd = O.cast_ray(u, a[0], a[1])
        return _words(ro, rd)
    assert fn == G.P_RENDER
    return _words(O.render_ray(u, p, q))


def test_probe_plan():
    """A few hundred points, every group present, and the cases are what they claim."""
    assert 300 <= NPROBES <= 1500, NPROBES
    assert set(PROBES) >= {"sdf_centres", "sdf_surface", "sdf_inside", "sdf_ties", "sdf_checkers",
                           "sdf_blend_itime", "march_step_cap", "march_escape", "march_hits",
                           "march_from_inside", "softshadow", "render_rays", "normal_surface"}
    for grp, recs in PROBES.items():
        for _, _, a, _ in recs:
            assert np.all(np.abs(a) < 2.0e9), (grp, a)  # int() stays inside the int range


def test_probe_cases_are_what_they_claim(rm, oracle):
    u = _uset(rm, "t0")
    want = {"sphere0|floor": (0, 7), "sphere1|floor": (1, 7), "torus|floor": (5, 7), "blend|floor": (4, 7)}
    for (_, _, a, name), k in zip(PROBES["sdf_ties"], range(len(PROBES["sdf_ties"]))):
        h = oracle.sdf(u, a[:3])
        first, later = want[name]
        # below the tie height the floor is nearer, at it the later entry (the floor) wins the
        # tie, above it the earlier primitive is nearer
        assert h.id == (first if k % 3 == 2 else later), (name, k, h.id, h.hitpoint)
    u = _uset(rm, "sweep20")
    colours = {oracle.sdf(u, a[:3]).color[0] for _, _, a, _ in PROBES["sdf_checkers"]}
    assert len(colours) == 2  # both cell colours are reached
    u2 = _uset(rm, "cam_in_blend")
    for _, fn, a, _ in PROBES["nan_through_max"]:
        v = oracle.point_light(u2, a[0:3], a[3:6], a[6:9]) if fn == G.P_POINTLIGHT else oracle.render_ray(u2, a[0:3], a[3:6])
        assert np.isnan(v).all(), (fn, a, v)
    neg = [oracle.sdf(u, a[:3]) for _, _, a, _ in PROBES["sdf_checkers"] if a[0] < -1001.0 and a[2] > 0.0]
    assert neg and all(h.id == 7 for h in neg)


@needs_ref
@pytest.mark.parametrize("group", sorted(PROBES))
def test_probe_group(rm, oracle, probed, group):
    bad = []
    for i, (us, fn, a, note) in enumerate(PROBES[group]):
        u = _uset(rm, us)
        want = _oracle_words(oracle, u, fn, a, note)
        got = probed[(group, i)]
        same = G.same_bits_or_nan(want.view(np.float32), got.view(np.float32))
        if fn in (G.P_SDF, G.P_RAYMARCH, G.P_REFLECTED):
            same[4] = want[4] == got[4]  # id: an int, compared as one
        if not same.all():
            bad.append((i, us, fn, a, want.view(np.float32), got.view(np.float32), want[4], got[4]))
    assert not bad, f"{group}: {len(bad)} of {len(PROBES[group])} probes differ, first: {bad[0]}"
