"""The geometry-edge classifier of the in-tree build (make librm, __graft_entry__.build):
rm_adaptive_edges.o holds k_adapt_classify_edges in its two lane mappings and nothing
else, neither uses scratch memory (the kernel descriptors' private segment), and no other
object holds it."""
import os

import pytest

from code_objects import OBJDUMP, kernel_objects, private_sizes

KERNEL = "22k_adapt_classify_edges"
OTHERS = kernel_objects(but=["rm_adaptive_edges.o"])


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
def test_edge_classifier_uses_no_scratch(tmp_path):
    priv = private_sizes("rm_adaptive_edges.o", tmp_path)
    assert len(priv) == 2, priv  # the two-pair form (ILb1E) and the plain one (ILb0E)
    assert all(KERNEL in name for name in priv), priv
    assert [n for n in priv if "ILb1E" in n] and [n for n in priv if "ILb0E" in n], priv
    assert all(v == 0 for v in priv.values()), priv


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj", OTHERS)
def test_other_objects_do_not_hold_it(obj, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert priv and not [k for k in priv if "classify_edges" in k], priv
