"""The accumulation kernels of the in-tree build (make librm, __graft_entry__.build):
rm_accum.o holds k_accum and k_accum_one, rm_table_accum.o their table twins, and no other
object holds a kernel of theirs.  From the kernel descriptors alone
(`<kernel>.kd`, tests/code_objects.py): none uses scratch memory, the multi-sample kernels
hold the wave's running sums in 192 B of LDS (the staged table is dynamic LDS and not in the
descriptor) and the one-sample kernels none, the built-in pair's registers allow 8 waves per
SIMD, and the table pair needs no more VGPRs than k_table_pattern."""
import os

import pytest

from code_objects import OBJDUMP, built_descriptors, kernel_objects

NEW = {"rm_accum.o": ("7k_accumE", "11k_accum_oneE"),
       "rm_table_accum.o": ("13k_table_accumE", "17k_table_accum_oneE")}
OTHERS = kernel_objects(but=list(NEW))

pytestmark = pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")


def find(kd, name):
    hit = [v for k, v in kd.items() if name in k]
    assert len(hit) == 1, (name, list(kd))
    return hit[0]


def test_the_new_objects_are_in_the_recipe():
    assert all(obj in kernel_objects() for obj in NEW) and len(OTHERS) == len(kernel_objects()) - 2


@pytest.mark.parametrize("obj", sorted(NEW))
def test_new_objects_hold_the_four_kernels_without_scratch(obj, tmp_path):
    kd = built_descriptors(obj, tmp_path)
    print(obj, kd)
    assert len(kd) == 2, list(kd)  # the object's only kernels
    multi, one = (find(kd, k) for k in NEW[obj])
    assert multi["scratch"] == 0 and one["scratch"] == 0, kd
    assert multi["lds"] == 192 and one["lds"] == 0, kd


def test_builtin_pair_allows_eight_waves_per_simd(tmp_path):
    """512 vector registers per lane of a SIMD: 8 waves at up to 64.  800 scalar registers per
    SIMD in allocations of 16: 8 waves at up to 96 (tests/test_adaptive_pattern_builds.py)."""
    kd = built_descriptors("rm_accum.o", tmp_path)
    for k in NEW["rm_accum.o"]:
        d = find(kd, k)
        assert 512 // d["vgprs"] >= 8 and d["sgprs"] <= 96, (k, d)


def test_table_pair_needs_no_more_vgprs_than_the_pattern_frame_kernel(tmp_path):
    kd = built_descriptors("rm_table_accum.o", tmp_path)
    ref = built_descriptors("rm_table_pattern.o", tmp_path)
    cap = find(ref, "15k_table_patternE")["vgprs"]
    for k in NEW["rm_table_accum.o"]:
        assert find(kd, k)["vgprs"] <= cap, (k, kd, cap)


@pytest.mark.parametrize("obj", OTHERS)
def test_other_objects_hold_no_accum_kernel(obj, tmp_path):
    kd = built_descriptors(obj, tmp_path)
    assert kd and not [k for k in kd if "accum" in k], list(kd)
