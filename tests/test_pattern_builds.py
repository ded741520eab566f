"""The sample-pattern kernels of the in-tree build (make librm, __graft_entry__.build):
rm_pattern.o holds k_pattern and k_pattern_one, rm_table_pattern.o holds k_table_pattern
and k_table_pattern_one, none uses scratch memory (the kernel descriptors' private
segment), and no older object holds a kernel of theirs."""
import os

import pytest

from code_objects import OBJDUMP, kernel_objects, private_sizes

NEW = [("rm_pattern.o", ("9k_patternE", "13k_pattern_oneE")),
       ("rm_table_pattern.o", ("15k_table_patternE", "19k_table_pattern_oneE"))]
# every other object that holds kernels, except pattern refinement's, whose kernels are
# k_*_refine_pattern* (test_adaptive_pattern_builds.py)
OLD = kernel_objects(but=[obj for obj, _ in NEW] + ["rm_adaptive_pattern.o", "rm_table_adaptive_pattern.o"])


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj,kernels", NEW)
def test_pattern_kernels_use_no_scratch(obj, kernels, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert len(priv) == len(kernels), priv  # the object's only kernels
    for k in kernels:
        assert [name for name in priv if k in name], (k, priv)
    assert all(v == 0 for v in priv.values()), priv


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj", OLD)
def test_existing_objects_hold_no_pattern_kernel(obj, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert priv and not [k for k in priv if "pattern" in k], priv
