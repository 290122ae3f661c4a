"""CPU: the bodies of csrc/nbe_web.h, which the eigenvalue and classification kernels are loops around, walked serially on
the host by tools/web_host_walk.hip and held to tests/web_ref.py on every tensor family of tools/web_host_walk.py: random,
diagonal, isotropic, rank one, two equal, nearly diagonal, wide range and non-finite input.  The program is built here
without sanitizers; the recipe with them is at its head."""
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
    import web_host_walk as W
    prog = str(tmp_path_factory.mktemp("web_host_walk") / "web_host_walk")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", prog,
                        os.path.join(ROOT, "tools", "web_host_walk.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return W, prog


def test_bodies_hold_the_reference(walker):
    """The bound 2^-23 |A|_F, lambda_1 >= lambda_2 >= lambda_3 on the bits returned, == on the families without
    off-diagonal words, three NaNs for a non-finite word, and the types of the returned words under four thresholds."""
    W, prog = walker
    worst = W.walk(prog)
    print({k: round(v, 3) for k, v in worst.items()})
    assert set(worst) >= {"random", "diagonal", "isotropic", "rank one", "two equal", "nearly diagonal", "wide range", "nan"}
    # one float32 rounding is half the bound: the float64 method may add 0.14 of a rounding to it (csrc/nbe_web.h)
    assert max(worst.values()) <= 0.5 * (1.0 + 0.14) + 1e-9
    for name in W.W.EXACT_FAMILIES:
        assert worst[name] == 0.0
