#!/usr/bin/env python
"""Drive tools/web_host_walk.hip: write the tensor families of tests/web_ref.py, run the host program (built under
-fsanitize=address,undefined, see its head) on each and hold what the bodies of csrc/nbe_web.h produced to the reference:
the eigenvalue bound, the order, == where the off-diagonal words are 0, NaN where a word is not finite, and the types from
the returned words.  A CPU machine only: nothing here touches a device.

    python tools/web_host_walk.py ./web_host_walk

tests/test_web_host_walk.py runs the same cases on a build without the sanitizers.
"""

import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import web_ref as W  # noqa: E402

COUNT = 20000
THRESHOLDS = np.array([0.0, -0.5, 0.2, 1.0e-6], np.float32)


def run(prog, h, thresholds):
    """(eig (3, count) float32, types (T, count) uint8) of the program on the tensors h (6, count) float32."""
    count = h.shape[1]
    with tempfile.TemporaryDirectory() as tmp:
        case, result = os.path.join(tmp, "case"), os.path.join(tmp, "result")
        with open(case, "wb") as f:
            f.write(np.array([count, len(thresholds)], np.int64).tobytes())
            f.write(np.ascontiguousarray(thresholds, np.float32).tobytes())
            f.write(np.ascontiguousarray(h, np.float32).tobytes())
        r = subprocess.run([prog, case, result], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        raw = open(result, "rb").read()
    eig = np.frombuffer(raw[:12 * count], np.float32).reshape(3, count)
    types = np.frombuffer(raw[12 * count:], np.uint8).reshape(len(thresholds), count)
    return eig, types


def walk(prog, verbose=False):
    """Every family; returns {name: worst error over the bound}."""
    worst = {}
    for name, h in W.tensor_families(COUNT, seed=31).items():
        eig, types = run(prog, h, THRESHOLDS)
        worst[name] = W.check_eigenvalues(name, h, eig)
        for t, th in enumerate(THRESHOLDS):
            assert np.array_equal(types[t], W.web_types(eig, th)), (name, t)
        if verbose:
            print("%-28s worst error / bound %.3f" % (name, worst[name]))
    return worst


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    walk(sys.argv[1], verbose=True)
    print("ok")
