#!/usr/bin/env python
"""Drive tools/fof_host_walk.hip: write the small cases of the FoF tests, run the host program (built under
-fsanitize=address,undefined, see its head) on each and compare what the kernel bodies produced with tests/fof_ref.py.

    python tools/fof_host_walk.py ./fof_host_walk
"""

import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fof_ref as F  # noqa: E402


def cases():
    for name in ("clustered16", "clustered16_half", "clustered24"):
        psi, L, v, kw, _ = F.case(name)
        yield name, psi, L, v, dict(kw)
    psi, L, ell, _, _ = F.threshold_field()
    yield "threshold", psi, L, None, dict(linking_length=ell, nmin=2, absolute=True)
    lattice = np.zeros((3, 16, 16, 16), np.float32)
    yield "lattice b=0.2", lattice, 100.0, None, dict(linking_length=0.2, nmin=2)
    yield "lattice b=1.0", lattice, 100.0, None, dict(linking_length=1.0, nmin=2)
    psi, L, ell = F.chain_field()
    yield "chain", psi, L, None, dict(linking_length=ell, nmin=2, absolute=True)


def walk(prog, tmp, psi, L, v, kw):
    ref = F.fof(psi, L, velocity=v, **kw)
    n = psi.shape[1]
    e = F.velocity_exponents(v) if v is not None else np.zeros(3, np.int64)
    case, res = os.path.join(tmp, "case.bin"), os.path.join(tmp, "result.bin")
    with open(case, "wb") as f:
        np.array([n, psi.dtype == np.float16, F.ncell_of(ref["R2"]), ref["R2"], kw["nmin"], v is not None], np.int64).tofile(f)
        np.array([L], np.float64).tofile(f)
        e.astype(np.int32).tofile(f)
        np.ascontiguousarray(psi).tofile(f)
        if v is not None:
            np.ascontiguousarray(v, np.float32).tofile(f)
    subprocess.run([prog, case, res], check=True)
    with open(res, "rb") as f:
        count, rows, bad = np.fromfile(f, np.int64, 3)
        X = np.fromfile(f, np.int32, 3 * count).reshape(3, count)
        root = np.fromfile(f, np.int32, count)
        label = np.fromfile(f, np.int32, rows)
        sums = np.fromfile(f, np.int64, 6 * rows).reshape(rows, 6)
    assert bad == 0
    assert np.array_equal(X, ref["X"]), "coordinates"
    assert np.array_equal(root, ref["root"]), "roots"
    assert np.array_equal(label, ref["label"]), "labels"
    length = ref["Length"].astype(np.float64)[:, None]
    cm = np.mod(ref["X"][:, ref["label"]].T + sums[:, :3].astype(np.float64) / length, float(F.U)) / float(F.U) * L
    assert np.array_equal(cm, ref["CMPosition"]), "CMPosition"
    if v is not None:
        cv = np.ldexp(sums[:, 3:].astype(np.float64), (e - 24)[None, :].astype(np.int32)) / length
        assert np.array_equal(cv, ref["CMVelocity"]), "CMVelocity"
    return rows, ref["ngroups"]


def main():
    prog = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        for name, psi, L, v, kw in cases():
            rows, groups = walk(prog, tmp, psi, L, v, kw)
            print("%-18s %5d halos of %6d groups: equal to the reference" % (name, rows, groups))


if __name__ == "__main__":
    main()
