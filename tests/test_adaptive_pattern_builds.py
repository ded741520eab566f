"""The pattern-refinement kernels of the in-tree build (make librm, __graft_entry__.build):
rm_adaptive_pattern.o holds k_adapt_refine_pattern and k_adapt_refine_pattern_one,
rm_table_adaptive_pattern.o their table twins, and no older object holds one of them
(DESIGN §4.15).  From the kernel descriptors alone (`<kernel>.kd`, 64 bytes): none uses
scratch memory (private_segment_fixed_size), the multi-sample kernels hold the wave's
running sums in 192 B of LDS (group_segment_fixed_size; the staged table is dynamic LDS
and not in the descriptor) and the one-sample kernels none, the built-in pair's registers
allow 8 waves per SIMD, and the table pair needs no more VGPRs than k_table_pattern."""
import os
import shutil
import struct
import subprocess

import pytest

from test_trace_builds import BUILD, OBJDUMP

NEW = {"rm_adaptive_pattern.o": ("22k_adapt_refine_patternE", "26k_adapt_refine_pattern_oneE"),
       "rm_table_adaptive_pattern.o": ("28k_table_adapt_refine_patternE", "32k_table_adapt_refine_pattern_oneE")}
OLD = ["rm_kernels.o", "rm_kernels_aa.o", "rm_table.o", "rm_trace.o", "rm_table_trace.o", "rm_gbuffer.o",
       "rm_table_gbuffer.o", "rm_sdf.o", "rm_table_sdf.o", "rm_adaptive.o", "rm_table_adaptive.o",
       "rm_adaptive_edges.o", "rm_mesh.o", "rm_pattern.o", "rm_table_pattern.o"]

pytestmark = pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")


def descriptors(obj, tmp_path):
    """{kernel: dict(lds, scratch, vgprs, sgprs)} of the gfx950 code object in build/obj.  vgprs and
    sgprs are the allocations compute_pgm_rsrc1 encodes: (granule + 1) * 8 of the unified vector
    file, (granule / 2 + 1) * 16 scalar registers."""
    src = os.path.join(BUILD, obj)
    if not os.path.exists(src):
        pytest.skip("librm not built")
    d = tmp_path / obj
    d.mkdir()
    shutil.copy(src, d / "x.o")
    subprocess.run([OBJDUMP, "--offloading", "x.o"], cwd=d, capture_output=True, check=True)
    cos = [p for p in os.listdir(d) if "gfx950" in p]
    assert len(cos) == 1, os.listdir(d)
    co = open(d / cos[0], "rb").read()
    shoff, = struct.unpack_from("<Q", co, 0x28)
    shentsize, shnum = struct.unpack_from("<HH", co, 0x3A)
    secs = [struct.unpack_from("<IIQQQQIIQQ", co, shoff + i * shentsize) for i in range(shnum)]
    out = {}
    for _, type_, _, _, off, size, link, _, _, _ in secs:
        if type_ != 2:  # SHT_SYMTAB
            continue
        stroff = secs[link][4]
        for k in range(size // 24):
            st_name, _, _, st_shndx, st_value, _ = struct.unpack_from("<IBBHQQ", co, off + 24 * k)
            sym = co[stroff + st_name:co.index(b"\0", stroff + st_name)].decode()
            if sym.endswith(".kd") and st_shndx < shnum:
                sec = secs[st_shndx]
                kd = sec[4] + (st_value - sec[3])
                lds, scratch = struct.unpack_from("<II", co, kd)
                rsrc1, = struct.unpack_from("<I", co, kd + 48)
                out[sym[:-3]] = dict(lds=lds, scratch=scratch, vgprs=((rsrc1 & 63) + 1) * 8,
                                     sgprs=(((rsrc1 >> 6) & 15) // 2 + 1) * 16)
    return out


def find(kd, name):
    hit = [v for k, v in kd.items() if name in k]
    assert len(hit) == 1, (name, list(kd))
    return hit[0]


@pytest.mark.parametrize("obj", sorted(NEW))
def test_new_objects_hold_the_four_kernels_without_scratch(obj, tmp_path):
    kd = descriptors(obj, tmp_path)
    print(obj, kd)
    assert len(kd) == 2, list(kd)  # the object's only kernels
    multi, one = (find(kd, k) for k in NEW[obj])
    assert multi["scratch"] == 0 and one["scratch"] == 0, kd
    assert multi["lds"] == 192 and one["lds"] == 0, kd


def test_builtin_pair_allows_eight_waves_per_simd(tmp_path):
    """512 vector registers per lane of a SIMD: 8 waves at up to 64.  800 scalar registers per
    SIMD in allocations of 16: 8 waves at up to 96 (the compiler's bound is 100)."""
    kd = descriptors("rm_adaptive_pattern.o", tmp_path)
    for k in NEW["rm_adaptive_pattern.o"]:
        d = find(kd, k)
        assert 512 // d["vgprs"] >= 8 and d["sgprs"] <= 96, (k, d)


def test_table_pair_needs_no_more_vgprs_than_the_pattern_frame_kernels(tmp_path):
    """k_table_pattern's allocation (88: 5 waves per SIMD) bounds both: the measured build has
    88 and 80, as k_table_pattern and k_table_pattern_one."""
    kd = descriptors("rm_table_adaptive_pattern.o", tmp_path)
    ref = descriptors("rm_table_pattern.o", tmp_path)
    cap = find(ref, "15k_table_patternE")["vgprs"]
    for k in NEW["rm_table_adaptive_pattern.o"]:
        assert find(kd, k)["vgprs"] <= cap, (k, kd, cap)


@pytest.mark.parametrize("obj", OLD)
def test_existing_objects_hold_no_refine_pattern_kernel(obj, tmp_path):
    kd = descriptors(obj, tmp_path)
    assert kd and not [k for k in kd if "refine_pattern" in k], list(kd)
