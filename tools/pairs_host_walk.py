#!/usr/bin/env python
"""Drive tools/pairs_host_walk.hip: write the small cases of the pair-count tests, run the host program (built under
-fsanitize=address,undefined, see its head) on each and compare the counts of the kernel bodies with tests/pairs_ref.py.
A CPU machine only: nothing here touches a device.

    python tools/pairs_host_walk.py ./pairs_host_walk
"""

import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import fof_ref as F  # noqa: E402
import pairs_ref as R  # noqa: E402


def cases():
    """(name, a, b or None, L, edges, nmu, los)"""
    lat = R.lattice_positions()
    yield "lattice positions", lat, None, R.LATTICE_L, R.LATTICE_EDGES, None, 2
    yield "lattice displacement", np.zeros((3, 16, 16, 16), np.float32), None, R.LATTICE_L, R.LATTICE_EDGES, None, 2
    pos = R.uniform_points()
    for dt in (np.float64, np.float32):
        p = pos.astype(dt)
        yield "uniform auto %s" % np.dtype(dt).name, p, None, R.UNIFORM_L, R.UNIFORM_EDGES, None, 2
        yield "uniform cross %s" % np.dtype(dt).name, p[:600], p[600:], R.UNIFORM_L, R.UNIFORM_EDGES, None, 2
    yield "uniform cross with itself", pos, pos, R.UNIFORM_L, R.UNIFORM_EDGES, None, 2
    for nmu in (1, 5, 32):
        for los in (0, 1, 2):
            yield "uniform nmu %d los %d" % (nmu, los), pos[:700], None, R.UNIFORM_L, R.UNIFORM_EDGES, nmu, los
    yield "uniform cross nmu 5", pos[:300], pos[300:900], R.UNIFORM_L, R.UNIFORM_EDGES, 5, 1
    rng = np.random.default_rng(8)
    yield "edges hit exactly", R.edge_points(), None, R.EDGE_L, R.EDGE_EDGES, 4, 0
    yield "one cell", rng.uniform(10.0, 10.2, size=(1000, 3)), None, 100.0, (0.0, 0.05, 0.1, 0.2), None, 2
    yield "ncell 4096", rng.uniform(0.0, 100.0, size=(10, 3)), None, 100.0, (0.0, 0.01, 0.02), None, 2
    yield "one row", np.array([[1.0, 2.0, 3.0]]), None, 100.0, (0.0, 1.0), 3, 2
    yield "128 bins", pos[:500], None, R.UNIFORM_L, np.linspace(0.0, 30.0, 129), None, 2
    yield "clustered displacement", F.clustered_field(16), pos[:400], R.UNIFORM_L, (0.0, 1.25, 4.0, 9.0), 2, 2


def write_catalogue(f, x):
    if x is None:
        return -1, 0
    if x.ndim == 4:
        np.ascontiguousarray(x, np.float32).tofile(f)
        return 2, x.shape[1]
    np.ascontiguousarray(x).tofile(f)
    return (1 if x.dtype == np.float64 else 0), x.shape[0]


def walk(prog, tmp, a, b, L, edges, nmu, los):
    T = R.thresholds(edges, L)
    ref = R.pair_counts(R.catalogue(a, L), T, None if b is None else R.catalogue(b, L), nmu=nmu, los=los)
    case, res = os.path.join(tmp, "case.bin"), os.path.join(tmp, "result.bin")
    with open(case, "wb") as f:
        f.write(b"\0" * (8 * 8))
        np.array([L], np.float64).tofile(f)
        np.array(T, np.int64).tofile(f)
        ka, ra = write_catalogue(f, a)
        kb, rb = write_catalogue(f, b)
        f.seek(0)
        np.array([ka, ra, kb, rb, R.ncell_of(T), len(T) - 1, nmu or 1, los], np.int64).tofile(f)
    subprocess.run([prog, case, res], check=True)
    with open(res, "rb") as f:
        bad = np.fromfile(f, np.int64, 1)[0]
        counts = np.fromfile(f, np.int64).reshape(len(T) - 1, nmu or 1)
    assert bad == 0
    assert np.array_equal(counts if nmu else counts[:, 0], ref), "counts"
    return int(ref.sum()), R.ncell_of(T)


def main():
    prog = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        for name, a, b, L, edges, nmu, los in cases():
            pairs, ncell = walk(prog, tmp, a, b, L, edges, nmu, los)
            print("%-28s %9d pairs, ncell %4d: equal to the reference" % (name, pairs, ncell))


if __name__ == "__main__":
    main()
