"""The hit's clearance (rm_scene.hpp "the hit's clearance", DESIGN.md §4.4 item
22) against the reference scene's five bounded primitives (rm_default_scene,
float64 distances):

  * geometry:   g = min_k sdf_k(p) - plane(p) > 2 r  =>  every primitive is above the
                plane's value at every p' with |p' - p| <= r;
  * budgets:    along p(t) = ro + rd t, an expiry te = t_i + gap_i / (|rd| + rd.y)
                with gap_i = sdf_k(p_i) - plane(p_i) leaves
                sdf_k(p(t)) - plane(p(t)) >= (|rd| + rd.y)(te - t) for t < te; the
                ball budget te = t_i + gap_i / (2 |rd|), gap_i = sdf_k(p_i) - min(p_i),
                leaves sdf_k - min >= 2 |rd| (te - t) >= (|rd| + rd.y)(te - t), which
                is the bound on sdf_k - plane wherever the plane is the minimum (a
                floor hit, the only place the kernels use it);
  * radii:      the thresholds' radii, formed in float32 as the kernels form them
                (CLR_THR_N, clr_thr_shadow), are at least the true distances of the
                probe points and of shadow steps 0 and 1 from the hit point.

The kernels' float roundings are covered by their margins (stated in the code);
this pins the geometry and the constants.  CPU only.
"""
import numpy as np

from scene_words import sdf64

BLENDS = (0.0, 0.3, 1.0)  # the blend's weight: box, between, sphere


def _prims(rm):
    prims = [q for q in rm.default_scene() if q.type != rm.PRIM_PLANE]
    assert len(prims) == 5
    return prims


def _each(rm, p, blend):
    """[5][n]: the bounded primitives' distances, the blend at weight `blend`."""
    out = []
    for q in _prims(rm):
        d = sdf64(p, q, blend)
        out.append(d[0] if len(d) == 1 else d[0] * (1.0 - blend) + d[1] * blend)
    return np.array(out)


def _plane(p):
    return p[:, 1] + 5.5


def _ball(rng, n, r):
    """n random offsets of length <= r[i]."""
    v = rng.normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    return v * (r * rng.uniform(0.0, 1.0, n) ** (1.0 / 3.0))[:, None]


def test_clearance_keeps_objects_above_the_plane_nearby(rm):
    rng = np.random.default_rng(22)
    n = 200_000
    # above the floor, most of them low (floor hits), over and around the objects
    p = np.concatenate([rng.uniform([-45, -5.5, -45], [35, -3.0, 25], (n, 3)),
                        rng.uniform([-45, -5.5, -45], [35, 8.0, 25], (n, 3))])
    r = rng.uniform(0.0, 1.5, 2 * n)
    r[::4] = rng.uniform(0.0, 0.03, len(r[::4]))  # the normal's and step 0's scale
    q = p + _ball(rng, 2 * n, r)
    used = 0
    for b in BLENDS:
        g = _each(rm, p, b).min(0) - _plane(p)
        ok = g > 2.0 * r
        used += int(ok.sum())
        d = _each(rm, q[ok], b)
        assert (d > _plane(q[ok])[None, :]).all(), b
        # and the margin is what Lipschitz says: sdf_k(p') - plane(p') >= g - 2 r
        assert (d - _plane(q[ok])[None, :] >= (g - 2.0 * r)[ok][None, :] - 1e-9).all(), b
    assert used > 300_000  # the claim is not vacuous on this sample
    # and it is tight: without the factor 2 some primitive does reach the plane's value
    g = _each(rm, p, 1.0).min(0) - _plane(p)
    near = (g > 0.5 * r) & (g < r)
    assert near.sum() > 1000


def test_budgets_bound_the_clearance_along_rays(rm):
    rng = np.random.default_rng(23)
    n = 20_000
    ro = rng.uniform([-40, -5.0, -40], [30, 12, 20], (n, 3))
    rd = rng.normal(size=(n, 3)) * rng.uniform(0.5, 2.0, (n, 1))  # not unit: reflected rays
    rd[::2, 1] = -np.abs(rd[::2, 1])  # half of them downward, toward the floor
    rl = np.linalg.norm(rd, axis=1)
    v = rl + rd[:, 1]  # |rd| + rd.y >= 0
    checked_p = checked_b = floor = 0
    for b in BLENDS:
        for ti in (0.0, 0.7, 4.0, 15.0):
            pi = ro + rd * ti
            di = _each(rm, pi, b)
            gap_p = di - _plane(pi)[None, :]                         # plane budget
            gap_b = di - np.minimum(di.min(0), _plane(pi))[None, :]  # ball budget (U = the minimum)
            te_p = ti + gap_p / np.maximum(v, 1e-12)[None, :]
            te_b = ti + gap_b / (2.0 * rl)[None, :]
            for f in (0.0, 0.25, 0.6, 0.95):
                for te, gap, ball in ((te_p, gap_p, False), (te_b, gap_b, True)):
                    for k in range(5):
                        live = gap[k] > 0.0
                        t = ti + f * (te[k] - ti)
                        live &= t < 1.0e4  # level rays: the plane budget may be long
                        pt = ro[live] + rd[live] * t[live][:, None]
                        dk = _each(rm, pt, b)
                        left = (te[k] - t)[live]
                        tol = 1e-9 * (1.0 + np.abs(pt).max(1) + gap[k][live])
                        if not ball:
                            assert (dk[k] - _plane(pt) >= v[live] * left - tol).all(), (b, ti, f, k)
                            checked_p += int(live.sum())
                        else:
                            mn = np.minimum(dk.min(0), _plane(pt))
                            assert (dk[k] - mn >= 2.0 * rl[live] * left - tol).all(), (b, ti, f, k)
                            assert (2.0 * rl[live] >= v[live]).all()
                            # where the plane is the minimum (a floor hit) that is the
                            # clearance's bound on sdf_k - plane
                            fl = _plane(pt) <= dk.min(0)
                            assert (dk[k][fl] - _plane(pt)[fl] >= (v[live] * left)[fl] - tol[fl]).all()
                            checked_b += int(live.sum())
                            floor += int(fl.sum())
    assert checked_p > 100_000 and checked_b > 100_000 and floor > 10_000


def test_threshold_radii_cover_the_probe_and_shadow_points(rm):
    f32 = np.float32
    rng = np.random.default_rng(24)
    n = 100_000
    pos = np.stack([rng.uniform(-300, 300, n), -5.5 + rng.uniform(-1e-4, 1e-4, n),
                    rng.uniform(-300, 300, n)], -1).astype(f32)
    nrm = np.array([0.0, 1.0, 0.0]) + rng.uniform(-1e-3, 1e-3, (n, 3))
    nrm = (nrm / np.linalg.norm(nrm, axis=1, keepdims=True)).astype(f32)
    light = rng.uniform(-40, 40, (n, 3)).astype(f32)
    M = 1.0 + 2.0 ** -10  # the thresholds promise r rounded up by this much
    pos64, nrm64, light64 = pos.astype(np.float64), nrm.astype(np.float64), light.astype(np.float64)
    # The float points are the real ones moved by their own roundings, which the
    # clearance's slack S pays for, not r: S >= 2^-14 (|pos|_1 + 64), and the
    # roundings below stay under E = 2^-21 (|pos|_1 + 64), 128 times less.
    E = 2.0 ** -21 * (np.abs(pos64).sum(1) + 64.0)

    # the normal's probes (normal_samples_plane): pos + 0.001 e_j, float adds
    CLR_THR_N = float(f32(0.00201))
    assert CLR_THR_N >= 2.0 * M * M * float(f32(0.001))  # the real probe distance
    for j in range(3):
        e = np.zeros(3, f32)
        e[j] = f32(0.001)
        pj = pos + e
        assert pj.dtype == f32
        dist = np.linalg.norm(pj.astype(np.float64) - pos64, axis=1)
        assert (CLR_THR_N >= 2.0 * M * M * (dist - E)).all()

    # softshadow (render): ro' = pos + 0.02 normal, rd' = light - pos, |rd'| = len(rd')
    ro = pos + nrm * f32(0.02)
    rd = light - pos
    rdl = np.sqrt((rd[:, 0] * rd[:, 0] + rd[:, 1] * rd[:, 1]) + rd[:, 2] * rd[:, 2]).astype(f32)
    assert rd.dtype == f32 and ro.dtype == f32 and rdl.dtype == f32

    def thr(t):  # clr_thr_shadow: fma(t * rdl, 2.004, 0.0401), one rounding
        return ((t * rdl).astype(np.float64) * float(f32(2.004)) + float(f32(0.0401))).astype(f32).astype(np.float64)

    def dists(t):
        """|p(t) - pos| of the real point (float64 arithmetic on the float inputs)
        and of the float point the kernel forms."""
        real = np.linalg.norm(float(f32(0.02)) * nrm64 + (light64 - pos64) * t.astype(np.float64)[:, None], axis=1)
        pf = ro + rd * t[:, None]
        assert pf.dtype == f32
        return real, np.linalg.norm(pf.astype(np.float64) - pos64, axis=1)

    zero = np.zeros(n, f32)
    r0, r0f = dists(zero)
    assert (thr(zero) >= 2.0 * M * M * r0).all() and (thr(zero) >= 2.0 * M * M * (r0f - E)).all()
    # step 1 at t1 = h0 = the plane's value at step 0, and at other small t
    h0 = (ro[:, 1] + f32(5.5)).astype(f32)
    for t1 in (h0, f32(0.5) * h0, rng.uniform(0.0, 1.0, n).astype(f32)):
        r1, r1f = dists(t1)
        assert (thr(t1) >= 2.0 * M * M * r1).all() and (thr(t1) >= 2.0 * M * M * (r1f - E)).all()
    assert 0.019 < r0.min() and r0.max() < 0.0201
