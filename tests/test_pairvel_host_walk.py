"""CPU: the velocity bodies of csrc/nbe_catalog.h (the velocity word and its gather, pair_velocity_terms with its exact
rounding, pair_velocity_particle and profile_velocity_stream), which the kernels of csrc/nbe_pairvel.hip are loops around,
walked serially on the host by mode `velocity` of tools/catalog_host_walk.hip -- the pair moments in an order of its own, the
per-centre tables in strides of 256 and of 64 -- and held to tests/pairvel_ref.py on every case of its list: the same
integers, to the bit.  The program is built here without sanitizers; the recipe with them is at its head."""
import os
import shutil
import subprocess
import sys

import pytest

import pairvel_ref as V

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


def test_velocity_bodies_equal_the_reference(walker):
    W, prog = walker
    lines = []
    assert W.walk_mode(prog, "velocity", lines.append) == len(V.CASE_NAMES) == 25
    assert all("equal to the reference" in line for line in lines)
