"""pytest configuration: the `gpu` marker and import paths.

`-m "not gpu"` tests run in the CPU container (oracle, host logic, ABI
loading); `-m gpu` tests run on an MI355X and call librm through its C-ABI.
"""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "opengl-raymarching-in-compute-shader_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "oracle")):
    if p not in sys.path:
        sys.path.insert(0, p)


_TMP_BASE = None


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs a HIP device (MI355X); calls librm")
    # hiprtc unpacks a program's headers under the temporary directory by their include
    # names, and "../../include/rm_api.h" (rm_jit.hip) lands one level above hiprtc's own
    # folder there: in a shared /tmp that is /tmp/include, which another user's earlier
    # run may own.  The session gets a private, nested TMPDIR, removed at its end.
    global _TMP_BASE
    import tempfile
    _TMP_BASE = tempfile.mkdtemp(prefix="rm_tests_")
    os.environ["TMPDIR"] = os.path.join(_TMP_BASE, "tmp")
    os.makedirs(os.environ["TMPDIR"])
    tempfile.tempdir = None  # re-read TMPDIR (tmp_path, mkdtemp in the tests)


def pytest_unconfigure(config):
    import shutil
    if _TMP_BASE:
        shutil.rmtree(_TMP_BASE, ignore_errors=True)


@pytest.fixture(scope="session")
def rm():
    import rmarch
    rmarch.lib()  # fails loudly if librm.so is missing
    return rmarch


@pytest.fixture(scope="session")
def oracle():
    import oracle as O
    O.lib()
    return O


@pytest.fixture(scope="session")
def gpu(rm):
    """Skip-free guard: a gpu-marked test must run on a GPU box."""
    n = rm.device_count()
    assert n > 0, "gpu test selected but no HIP device is visible"
    return n
