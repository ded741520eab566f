"""SDF field queries against tests/sdf_model.py on many seeded points (diagnostic, not
product).

  python tools/stress_sdf.py [--n 200000]

Four seeded sets of n points each, spread over the fast lanes' predicate and across its
border, through rm_sdf_points (VALUE | NORMAL) of the built-in scene and of the default
table at iTime 0, 1 and 4.5, every field compared with the model bit for bit (a NaN equal
to a NaN; the model is pinned to the oracle by tests/test_sdf_model.py):

  box      uniform in the scene's box
  shell    directions uniform, |p| log-uniform in [2^-20, 2^22] (both sides of |p|_1 = 2^20)
  surface  box points moved to within 1e-3 of the nearest surface along the model's normal
  axis     box points with one or two coordinates replaced by +-0, denormals and the
           object centres' coordinates
"""
import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

F32 = np.float32
FIELDS = ("t", "id", "material", "albedo", "normal", "color")


def point_sets(M, scene, n):
    g = np.random.default_rng(11)
    box = g.uniform([-32, -7, -36], [22, 12, 16], (n, 3)).astype(F32)
    d = g.normal(size=(n, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    shell = (d * np.exp2(g.uniform(-20, 22, (n, 1)))).astype(F32)
    dist = M.sdf_table(scene, 1.0, box)[0]
    nrm = M.get_normal(scene, 1.0, box)
    with np.errstate(all="ignore"):
        surface = (box - nrm * (dist + g.uniform(-1e-3, 1e-3, n).astype(F32))[:, None]).astype(F32)
    surface = np.where(np.isfinite(surface), surface, box)
    special = np.array([0.0, -0.0, 1e-40, -1e-40, 1e-30, 15.0, -25.0, -5.0, -10.0, 10.0, -2.0, -30.0, -5.5], F32)
    axis = box.copy()
    for k in range(2):
        col = g.integers(0, 3, n)
        use = g.uniform(size=n) < (1.0 if k == 0 else 0.5)
        axis[np.arange(n)[use], col[use]] = special[g.integers(0, len(special), n)][use]
    return {"box": box, "shell": shell, "surface": surface, "axis": axis}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=200000)
    a = ap.parse_args()
    import rmarch as rm
    import sdf_model as M

    if rm.device_count() < 1:
        sys.exit("stress_sdf: no GPU")
    scene = rm.default_scene()
    sets = point_sets(M, scene, a.n)
    bad = 0
    for itime in (0.0, 1.0, 4.5):
        u = rm.default_uniforms()
        u.iTime = itime
        for name, pts in sets.items():
            want = M.sdf_records(rm, scene, itime, pts, normal=True)
            fast = int((np.abs(pts).sum(axis=1, dtype=F32) <= F32(2.0 ** 20)).sum())
            for kind in ("built-in", "table"):
                with rm.Renderer(64, 64) as r:
                    if kind == "table":
                        r.set_scene(scene)
                    r.set_uniforms(u)
                    got = r.sdf(pts, rm.RM_SDF_NORMAL)
                diff = 0
                for f in FIELDS:
                    x, y = got[f], want[f]
                    same = x.view(np.uint32) == y.view(np.uint32)
                    if x.dtype.kind == "f":
                        same |= np.isnan(x) & np.isnan(y)
                    diff += int((~same).sum())
                bad += diff
                print(f"iTime {itime:<4} {name:<8} {kind:<9} {len(pts)} points ({fast} in the predicate, "
                      f"{int((want['t'] < 0).sum())} inside, {int(np.isnan(want['normal']).any(axis=1).sum())} NaN normals): "
                      f"{diff} mismatches")
    print(f"total mismatches: {bad}")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
