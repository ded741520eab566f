"""The diagnostic builds of the fixed-work items, compiled
for gfx950 as tests/test_builds.py compiles the others: the RM_DBL_CAST and
RM_DBL_STORE cost probes of rm_kernels.hip (tools/build_variant.sh,
tools/ab_kernel.py), and tools/exhaustive_fp.hip with its quantize and sqrt_vote
modes.  No GPU needed."""
import os
import subprocess

import pytest

from code_objects import hipflags

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd", "csrc")
HIPCC = "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")


@pytest.mark.parametrize("probe", ["RM_DBL_CAST", "RM_DBL_STORE"])
def test_cost_probe_compiles(probe, tmp_path):
    cmd = [HIPCC, *hipflags(), "--cuda-device-only", "-c", os.path.join(CSRC, "rm_kernels.hip"),
           "-o", str(tmp_path / "k.o"), f"-D{probe}=1"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]


def _kernel_asm(asm, name):
    """The instructions of kernel `name` in hipcc -S output."""
    body, on = [], False
    for line in asm.splitlines():
        if line.startswith("_Z") and ":" in line:  # "_Z10k_quantizePyPj:   ; @..."
            on = name in line.split(":")[0]
        elif on and line.startswith("\t") and not line.startswith("\t."):
            body.append(line.strip())
        if on and "s_endpgm" in line:
            on = False
    return body


def test_exhaustive_fp_compiles_and_enumerates_the_lean_forms(tmp_path):
    """The tool builds, and its two new kernels hold the forms they are there to prove,
    not the forms they are compared with: k_quantize the clamp (v_med3_f32, or the
    v_max_f32 ... clamp the compiler makes of it), k_sqrt_vote the vote's scalar branch
    with sqrt_core on both sides of it besides the reference's (three v_rsq_f32)."""
    src = os.path.join(ROOT, "tools", "exhaustive_fp.hip")
    text = open(src).read()
    for mode in ('"quantize"', '"sqrt_vote"', "rmd::quantize<true>", "rmd::sqrt_vote"):
        assert mode in text, mode
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "-c", src, "-o", str(tmp_path / "e.o")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    cmd = [HIPCC, "--offload-arch=gfx950", "-O3", "-ffp-contract=off", "--cuda-device-only", "-S", src,
           "-o", str(tmp_path / "e.s")]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    asm = open(tmp_path / "e.s").read()
    q = _kernel_asm(asm, "k_quantize")
    assert q and any(i.startswith("v_med3_f32") or (i.startswith("v_max_f32") and "clamp" in i) for i in q), q[:40]
    assert any(i.startswith("v_cndmask") for i in q), "the compare-and-select form is there to compare with"
    v = _kernel_asm(asm, "k_sqrt_vote")
    assert sum(i.startswith("v_rsq_f32") for i in v) >= 3, [i for i in v if "rsq" in i]
    assert any(i.startswith("s_cbranch") for i in v)
