"""Generate tests/golden/reference_goldens.npz + .json: small frames computed by the
reference's own compute shader, compiled as C++ (oracle/_ref/glsl_ref: the shader
text over the reference's GLM, with DESIGN §2's built-ins; oracle/glsl_ref_main.cpp).

The files hold data only: per case the rm_uniforms bytes, W, H and the RGBA32F
frame.  They let the CPU suite check that the oracle still equals the shader
where the reference is absent (tests/test_reference_shader.py) and let the GPU
suite compare librm with the shader's output directly (tests/test_gpu_reference.py).

Every case also runs through oracle/_ref/glsl_ref_ubsan (UBSan + float-cast-
overflow: the shader's int() of an out-of-range float is undefined in C++).  A
case on which that binary reports anything, or whose frame differs from
glsl_ref's, is refused and nothing is written.

Needs the reference tree at build time (`make glsl_ref`).  Regenerate only when
the cases change:
    python tests/golden/make_reference_goldens.py
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import rmarch as rm  # noqa: E402
import glsl_ref as G  # noqa: E402

S, M, L = (33, 19), (48, 27), (67, 41)  # ragged: no frame is a whole number of 4x4 wave tiles

LIGHT_FAR = (300.0, 200.0, -400.0)
LIGHT_BETWEEN_A = (5.0, 1.0, -10.0)    # between sphere 0 and the blend object
LIGHT_BETWEEN_B = (-5.0, 0.5, 0.0)     # between the blend object and the torus
IN_BLEND = (-5.5, 0.3, -9.6)
IN_SPHERE0 = (15.5, 0.2, -10.3)
IN_SPHERE1 = (-25.0, 0.5, -10.0)
IN_TORUS_TUBE = (-7.5, 0.0, 10.0)

# name: (shape, sweep frame, bounces, AA, light position, camera position, (pos, lookAt))
CASES = {
    "sweep_f0_b0": (L, 0, 0, False, None, None, None),
    "sweep_f0_b1_aa": (S, 0, 1, True, None, None, None),
    "sweep_f0_b3_aa": (M, 0, 3, True, None, None, None),
    "sweep_f37_b1": (M, 37, 1, False, None, None, None),
    "sweep_f37_b4_aa": (S, 37, 4, True, None, None, None),
    "sweep_f37_b5_aa": (M, 37, 5, True, None, None, None),
    "sweep_f60_b0_aa": (S, 60, 0, True, None, None, None),
    "sweep_f60_b2_aa": (L, 60, 2, True, None, None, None),
    "sweep_f60_b5": (M, 60, 5, False, None, None, None),
    "sweep_f119_b2": (M, 119, 2, False, None, None, None),
    "sweep_f119_b3": (S, 119, 3, False, None, None, None),
    "sweep_f119_b5_aa": (L, 119, 5, True, None, None, None),
    "light_far_b3_aa": (M, 20, 3, True, LIGHT_FAR, None, None),
    "light_far_b1": (L, 75, 1, False, LIGHT_FAR, None, None),
    "light_between_b3_aa": (L, 20, 3, True, LIGHT_BETWEEN_A, None, None),
    "light_between_b2": (S, 100, 2, False, LIGHT_BETWEEN_B, None, None),
    "cam_in_blend_b3_aa": (M, 20, 3, True, None, IN_BLEND, None),
    "cam_in_blend_b1": (S, 45, 1, False, None, IN_BLEND, None),
    "cam_in_sphere_b2_aa": (S, 20, 2, True, None, IN_SPHERE0, None),
    "cam_in_sphere_b0": (M, 90, 0, False, None, IN_SPHERE1, None),
    "cam_in_torus_tube_b3_aa": (L, 20, 3, True, None, IN_TORUS_TUBE, None),
    "cam_in_torus_tube_b1": (S, 60, 1, False, None, IN_TORUS_TUBE, None),
    "graze_floor_b3_aa": (L, 20, 3, True, None, None, ((10.0, -5.45, 30.0), (-5.0, -5.3, -10.0))),
    "graze_floor_b0": (M, 20, 0, False, None, None, ((-30.0, -5.49, 5.0), (15.0, -5.2, -10.0))),
}
NAN_CASES = [n for n in CASES if n.startswith("cam_in_")]


def uniforms(name):
    (W, H), frame, bounces, aa, light, cam, look = CASES[name]
    u = rm.sweep_uniforms(frame, 120, bounces, aa, rm.RM_SHADOW_SOFT)
    if light is not None:
        for i in range(3):
            u.light.position[i] = light[i]
    if cam is not None:
        for i in range(3):
            u.camera.pos[i] = cam[i]
    if look is not None:
        u.camera = rm.Camera(W, H, pos=look[0], lookAt=look[1]).to_uniform()
    return u, W, H


def main():
    for b in (G.GLSL_REF, G.GLSL_REF_UBSAN):
        if not G.available(b):
            sys.exit(f"{b} is missing: build it where the reference tree is present (make glsl_ref)")
    arrays, cases = {}, {}
    env_note = "UBSan (-fsanitize=undefined,float-cast-overflow)"
    for name in CASES:
        u, W, H = uniforms(name)
        img = G.frame(u, W, H)
        san = G.frame_raw(u, W, H, binary=G.GLSL_REF_UBSAN, check=False)
        if san.returncode != 0 or san.stderr:
            sys.exit(f"case {name}: glsl_ref_ubsan exit {san.returncode}, reports:\n"
                     f"{san.stderr.decode(errors='replace')}\nrefused; nothing written")
        if san.stdout != img.tobytes():
            sys.exit(f"case {name}: glsl_ref_ubsan's frame differs from glsl_ref's; nothing written")
        nan = int(np.isnan(img).any(axis=2).sum())
        if (name in NAN_CASES) != (nan > 0):
            sys.exit(f"case {name}: {nan} NaN pixels, expected {'some' if name in NAN_CASES else 'none'}")
        arrays[name + "_uniforms"] = np.frombuffer(G.uniform_bytes(u), np.uint8)
        arrays[name + "_rgba32f"] = img
        cases[name] = {"W": W, "H": H, "nan_pixels": nan}
        print(f"{name}: {W}x{H}, {nan} NaN pixels, {env_note}: no report, same frame")
    meta = {"generator": "tests/golden/make_reference_goldens.py", "binary": "oracle/_ref/glsl_ref",
            "shader": "shaders/computeShader.glsl", **G.info(),
            "sanitizer": f"oracle/_ref/glsl_ref_ubsan, {env_note}: no report on {len(cases)} of "
                         f"{len(cases)} cases, every frame equal to glsl_ref's",
            "cases": cases}
    out = os.path.join(HERE, "reference_goldens.npz")
    np.savez_compressed(out, **arrays)
    size, cap = os.path.getsize(out), os.path.getsize(os.path.join(HERE, "oracle_goldens.npz"))
    if size > min(cap, 1 << 20):
        os.unlink(out)
        sys.exit(f"reference_goldens.npz would be {size} bytes (> {min(cap, 1 << 20)}): shrink the shapes")
    with open(os.path.join(HERE, "reference_goldens.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(meta["sanitizer"])
    print(f"wrote {len(cases)} cases, {sum(c['W'] * c['H'] for c in cases.values())} pixels, "
          f"{size} bytes (limit {min(cap, 1 << 20)})")


if __name__ == "__main__":
    main()
