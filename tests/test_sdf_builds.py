"""The SDF field-query kernels of the in-tree build (make librm, __graft_entry__.build):
k_sdf_points / k_sdf_grid and k_table_sdf_points / k_table_sdf_grid use no scratch
memory (their kernel descriptors' private segment) and live in objects of their
own, so the render, ray-query and G-buffer kernels' objects hold no sdf kernel
(DESIGN §4.11)."""
import os

import pytest

from code_objects import OBJDUMP, kernel_objects, private_sizes

NEW = [("rm_sdf.o", ("12k_sdf_pointsE", "10k_sdf_gridE")),
       ("rm_table_sdf.o", ("18k_table_sdf_pointsE", "16k_table_sdf_gridE"))]
OLD = kernel_objects(but=[obj for obj, _ in NEW])


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj,kernels", NEW)
def test_sdf_kernels_use_no_scratch(obj, kernels, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert len(priv) == len(kernels), priv  # the object's only kernels
    for k in kernels:
        assert [name for name in priv if k in name], (k, priv)
    assert all(v == 0 for v in priv.values()), priv


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj", OLD)
def test_existing_objects_hold_no_sdf_kernel(obj, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert priv and not [k for k in priv if "sdf" in k], priv
