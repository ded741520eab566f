"""The ray-query kernels of the in-tree build (make librm, __graft_entry__.build):
k_trace and k_table_trace use no scratch memory (their kernel descriptors'
private segment), and live in objects of their own, so the render kernels'
objects hold no trace kernel."""
import os

import pytest

from code_objects import OBJDUMP, private_sizes


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj,kernel", [("rm_trace.o", "7k_traceE"), ("rm_table_trace.o", "13k_table_traceE")])
def test_trace_kernels_use_no_scratch(obj, kernel, tmp_path):
    priv = private_sizes(obj, tmp_path)
    assert list(priv) and all(kernel in k for k in priv), priv  # the object's only kernel
    assert all(v == 0 for v in priv.values()), priv


@pytest.mark.skipif(not os.path.exists(OBJDUMP), reason="llvm-objdump not installed")
@pytest.mark.parametrize("obj", ["rm_kernels.o", "rm_kernels_aa.o", "rm_table.o"])
def test_render_objects_hold_no_trace_kernel(obj, tmp_path):
    assert not [k for k in private_sizes(obj, tmp_path) if "trace" in k]
