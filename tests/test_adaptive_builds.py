"""The adaptive-supersampling kernels of the in-tree build (make librm,
__graft_entry__.build): rm_adaptive.o holds k_adapt_classify, k_adapt_mask, k_adapt_scan,
k_adapt_scatter and k_adapt_refine, rm_table_adaptive.o holds k_table_adapt_refine, none
uses scratch memory (the kernel descriptors' private segment), and no other object holds
a kernel of theirs."""
import os

import pytest

from code_objects import OBJDUMP, kernel_objects, private_sizes

NEW = [("rm_adaptive.o", ("16k_adapt_classifyE", "12k_adapt_maskE", "12k_adapt_scanE", "15k_adapt_scatterE",
                          "14k_adapt_refineE")),
       ("rm_table_adaptive.o", ("20k_table_adapt_refineE",))]
# every other object that holds kernels, except the later members of the family, whose
# kernels are k_adapt_* too: the geometry-edge classifier (test_adaptive_edges_builds.py) and
# pattern refinement (test_adaptive_pattern_builds.py)
OLD = kernel_objects(but=[obj for obj, _ in NEW] + ["rm_adaptive_edges.o", "rm_adaptive_pattern.o",
                                                    "rm_table_adaptive_pattern.o"])


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj,kernels", NEW)
def test_adaptive_kernels_use_no_scratch(obj, kernels, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert len(priv) == len(kernels), priv  # the object's only kernels
    for k in kernels:
        assert [name for name in priv if k in name], (k, priv)
    assert all("adapt" in name for name in priv), priv
    assert all(v == 0 for v in priv.values()), priv


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj", OLD)
def test_existing_objects_hold_no_adaptive_kernel(obj, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert priv and not [k for k in priv if "adapt" in k], priv
