"""The uniforms of the tests (a helper, not a test): the main frame, the query tests'
defaults, the AA switch, a camera aimed at a point, and the seeded random cases of the
uniform fuzz (tests/test_gpu_fuzz_uniforms.py) with the frames other files take from them.
Importable without a device: `rm` is the rmarch module the tests' fixture hands in."""
import os

import numpy as np


def main_u(rm, bounces=1, shadow=0, aa=False):
    """The main frame of the G-buffer, adaptive and pattern tests."""
    return rm.sweep_uniforms(60, 120, bounces, aa, shadow)


def default_u(rm, bounces=0, shadow_mode=0, itime=1.0):
    """The query tests' uniforms: the defaults with iTime = 1."""
    u = rm.default_uniforms()
    u.iTime = itime
    u.bounceVar = bounces
    u.shadow_mode = shadow_mode
    return u


def with_aa(u, aa):
    v = type(u).from_buffer_copy(u)
    v.AA = 1 if aa else 0
    return v


def aim(u, pos, look):
    """The camera at pos looking at the point `look`: the uniform's basis (glsl:68-74
    takes dir, xAxis and yAxis as they come), right-handed with world up (0, 1, 0)."""
    f = np.array(look, np.float64) - np.array(pos, np.float64)
    f /= np.linalg.norm(f)
    x = np.cross(f, (0.0, 1.0, 0.0))
    x /= np.linalg.norm(x)
    y = np.cross(x, f)
    for i in range(3):
        u.camera.pos[i], u.camera.dir[i] = pos[i], f[i]
        u.camera.xAxis[i], u.camera.yAxis[i] = x[i], y[i]


# ---- the uniform fuzz: seeded random cameras, lights, bounce counts, AA and shadow modes ----
SEED = 20261018
# RM_FUZZ_CASES widens the run (the first N cases do not depend on N)
NCASES = int(os.environ.get("RM_FUZZ_CASES", "256"))
W, H = 67, 41  # ragged: neither a multiple of the 8x8 tile

# primitive centres of the built-in scene (glsl:111-120; rm_scene.hpp offsets,
# CAP_M*): spheres, blend, torus, capsule midpoint
CENTRES = np.array([(15.0, 0.0, -10.0), (-25.0, 0.0, -10.0), (-5.0, 0.0, -10.0),
                    (-5.0, 0.0, 10.0), (-4.05, 0.05, -29.05)], np.float32)


def _cases():
    rng = np.random.default_rng(SEED)
    out = []
    for i in range(NCASES):
        if rng.random() < 0.35:
            pos = CENTRES[rng.integers(len(CENTRES))] + rng.uniform(-4.0, 4.0, 3)
        else:
            pos = rng.uniform((-40.0, -6.0, -40.0), (40.0, 15.0, 40.0))
        while True:
            look = np.array((-5.0, 0.0, -10.0)) + rng.uniform(-20.0, 20.0, 3)
            f = look - pos
            n = np.linalg.norm(f)
            if n > 1.0 and abs(f[1]) / n < 0.98:
                break
        r = rng.random()
        if r < 0.2:
            light = rng.uniform(-1.0, 1.0, 3) * 1.0e3
        elif r < 0.4:
            light = CENTRES[rng.integers(len(CENTRES))] + rng.uniform(-5.0, 5.0, 3)
        elif r < 0.8:
            light = rng.uniform((-40.0, -8.0, -40.0), (40.0, 30.0, 40.0))
        else:
            light = None  # the sweep's own light
        out.append(dict(pos=tuple(map(float, pos)), look=tuple(map(float, look)),
                        light=None if light is None else tuple(map(float, light)),
                        bounces=int(rng.integers(0, 6)), aa=bool(rng.random() < 0.5),
                        sm=int(rng.integers(0, 2)), itime=float(rng.uniform(0.0, 60.0)),
                        frame=int(rng.integers(0, 120))))
    return out


CASES = _cases()


def _uniforms(rm, c):
    u = rm.sweep_uniforms(c["frame"], 120, c["bounces"], c["aa"], c["sm"])
    u.camera = rm.Camera(W, H, pos=c["pos"], lookAt=c["look"]).to_uniform()
    if c["light"] is not None:
        for i in range(3):
            u.light.position[i] = c["light"][i]
    u.iTime = c["itime"]
    return u


def off_sweep_uniforms(rm, i):
    """(u, (W, H)) of fuzz case i < 16; i = 16 is case 0 with one non-finite camera."""
    if i < 16:
        return _uniforms(rm, CASES[i]), (W, H)
    u = _uniforms(rm, CASES[0])
    u.camera.pos[0] = float("nan")
    return u, (W, H)
