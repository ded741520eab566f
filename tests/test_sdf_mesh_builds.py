"""The mesh-extraction kernels of the in-tree build (make librm,
__graft_entry__.build): rm_mesh.o holds the six of them and no other, and none
uses scratch memory (its kernel descriptor's private segment)."""
import os

import pytest

from code_objects import OBJDUMP, private_sizes

KERNELS = ("15k_mesh_classifyE", "11k_mesh_scanE", "18k_mesh_scan_chunksE", "15k_mesh_verticesE", "12k_mesh_quadsE", "16k_mesh_attr_copyE")


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
def test_mesh_kernels_use_no_scratch(tmp_path):
    priv = private_sizes("rm_mesh.o", tmp_path)
    assert len(priv) == len(KERNELS), priv  # the object's only kernels
    for k in KERNELS:
        assert [name for name in priv if k in name], (k, priv)
    assert all(v == 0 for v in priv.values()), priv
