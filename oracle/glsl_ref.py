"""Runs oracle/_ref/glsl_ref (the reference's shader compiled as C++, see
oracle/glsl_ref_main.cpp) — TEST INFRASTRUCTURE ONLY.

The binaries exist only where the reference tree was present at build time
(`make oracle/_ref/glsl_ref`); tests that need them skip otherwise, and the GPU
suite reads the frames they produced from tests/golden/reference_goldens.*.
"""
from __future__ import annotations

import ctypes as C
import json
import os
import subprocess
import tempfile
from typing import Optional, Sequence

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.path.join(_HERE, "_ref")
GLSL_REF = os.path.join(REF_DIR, "glsl_ref")              # GLM built-ins + DESIGN §2's exceptions
GLSL_REF_GLM = os.path.join(REF_DIR, "glsl_ref_glm")      # GLM built-ins only
GLSL_REF_UBSAN = os.path.join(REF_DIR, "glsl_ref_ubsan")  # glsl_ref under UBSan (fixture generator)

# probe function numbers (glsl_ref_main.cpp)
P_SDF, P_RAYMARCH, P_REFLECTED, P_NORMAL, P_SOFTSHADOW, P_POINTLIGHT, P_CASTRAY, P_RENDER = range(8)

PROBE_REC = np.dtype([("fn", "<i4"), ("a", "<f4", (9,))])
assert PROBE_REC.itemsize == 40


def available(binary: str = GLSL_REF) -> bool:
    return os.access(binary, os.X_OK)


def uniform_bytes(u) -> bytes:
    """The rm_uniforms struct (ctypes) as the 168 bytes the driver reads."""
    b = bytes(memoryview(u).cast("B")) if not isinstance(u, (bytes, bytearray)) else bytes(u)
    assert len(b) == 168, len(b)
    return b


def _with_uniforms(u, fn):
    fd, path = tempfile.mkstemp(prefix="rm_uniforms_", suffix=".bin")
    try:
        with os.fdopen(fd, "wb") as fh:
            fh.write(uniform_bytes(u))
        return fn(path)
    finally:
        os.unlink(path)


def frame_raw(u, W: int, H: int, workgroups: Optional[int] = None, binary: str = GLSL_REF,
              check: bool = True) -> subprocess.CompletedProcess:
    """`glsl_ref frame`: the finished process (stdout = raw RGBA32F, stderr = its reports)."""
    def run(path):
        cmd = [binary, "frame", str(W), str(H), path]
        if workgroups is not None:
            cmd.append(str(workgroups))
        return subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, check=check)
    return _with_uniforms(u, run)


def frame(u, W: int, H: int, workgroups: Optional[int] = None, binary: str = GLSL_REF) -> np.ndarray:
    """The shader's RGBA32F image for uniforms u, [H][W][4], row 0 = pixel row 0."""
    p = frame_raw(u, W, H, workgroups, binary)
    out = np.frombuffer(p.stdout, "<f4")
    assert out.size == W * H * 4, (out.size, W, H)
    return out.reshape(H, W, 4).copy()


def probe(u, records: Sequence, binary: str = GLSL_REF) -> np.ndarray:
    """Shader functions on single arguments.  records: (fn, args) pairs, args up
    to 9 floats.  Returns uint32 [n][8], the raw result words: a RayHit is
    (hitpoint, colour x3, id as int32, material), a vec3 its 3 floats, a float
    itself, castRay's Ray origin then direction."""
    rec = np.zeros(len(records), PROBE_REC)
    for i, (fn, args) in enumerate(records):
        a = np.asarray(args, np.float32).ravel()
        rec["fn"][i] = fn
        rec["a"][i, :a.size] = a
    p = _with_uniforms(u, lambda path: subprocess.run(
        [binary, "probe", path], input=rec.tobytes(), stdout=subprocess.PIPE,
        stderr=subprocess.PIPE, check=True))
    out = np.frombuffer(p.stdout, "<u4")
    assert out.size == len(records) * 8, (out.size, len(records))
    return out.reshape(len(records), 8).copy()


def info(binary: str = GLSL_REF) -> dict:
    p = subprocess.run([binary, "info"], stdout=subprocess.PIPE, check=True)
    return json.loads(p.stdout)


def same_bits_or_nan(a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """Elementwise: equal as uint32, or NaN on both sides (the payload is not compared)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))
