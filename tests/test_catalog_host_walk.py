"""CPU: the bodies of csrc/nbe_catalog.h, which the FoF, pair-count and profile kernels are loops around, walked serially on
the host by tools/catalog_host_walk.hip and held to tests/fof_ref.py, tests/pairs_ref.py and tests/profiles_ref.py on every
case of tools/catalog_host_walk.py: the same integers, to the bit.  The program is built here without sanitizers; the recipe
with them is at its head."""
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")


@pytest.fixture(scope="module")
def walker(tmp_path_factory):
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import catalog_host_walk as W
    prog = str(tmp_path_factory.mktemp("catalog_host_walk") / "catalog_host_walk")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", prog,
                        os.path.join(ROOT, "tools", "catalog_host_walk.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return W, prog


@pytest.mark.parametrize("mode, cases", [("fof", 7), ("pairs", 23), ("profiles", 15)])
def test_bodies_equal_the_reference(walker, mode, cases):
    W, prog = walker
    assert W.walk_mode(prog, mode) == cases
