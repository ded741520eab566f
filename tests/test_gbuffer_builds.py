"""The G-buffer kernels of the in-tree build (make librm, __graft_entry__.build):
k_gbuf_pixel / k_gbuf_sample and k_table_gbuf_pixel / k_table_gbuf_sample use no
scratch memory (their kernel descriptors' private segment) and live in objects of
their own, so the render and ray-query kernels' objects hold no G-buffer kernel
(DESIGN §4.10)."""
import os

import pytest

from code_objects import OBJDUMP, kernel_objects, private_sizes

NEW = [("rm_gbuffer.o", ("12k_gbuf_pixelE", "13k_gbuf_sampleE")),
       ("rm_table_gbuffer.o", ("18k_table_gbuf_pixelE", "19k_table_gbuf_sampleE"))]
OLD = kernel_objects(but=[obj for obj, _ in NEW])


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj,kernels", NEW)
def test_gbuffer_kernels_use_no_scratch(obj, kernels, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert len(priv) == len(kernels), priv  # the object's only kernels
    for k in kernels:
        assert [name for name in priv if k in name], (k, priv)
    assert all("gbuf" in name for name in priv), priv
    assert all(v == 0 for v in priv.values()), priv


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj", OLD)
def test_existing_objects_hold_no_gbuffer_kernel(obj, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert priv and not [k for k in priv if "gbuf" in k], priv
