#!/usr/bin/env python
"""Drive tools/profiles_host_walk.hip: write the small cases of the profile tests, run the host program (built under
-fsanitize=address,undefined, see its head) on each and compare the count tables of the kernel bodies, in both forms'
strides, with tests/profiles_ref.py.  A CPU machine only: nothing here touches a device.

    python tools/profiles_host_walk.py ./profiles_host_walk
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
import profiles_ref as PR  # noqa: E402


def cases():
    """(name, centres, matter, L, edges)"""
    pos = R.uniform_points()
    for dt in (np.float64, np.float32):
        p = pos.astype(dt)
        yield "uniform %s" % np.dtype(dt).name, p[:300], p, R.UNIFORM_L, R.UNIFORM_EDGES
    yield "uniform r_0 = 2", pos[:300], pos, R.UNIFORM_L, R.UNIFORM_EDGES[1:]
    psi = F.clustered_field(16)
    corners = np.array([[x, y, z] for x in (0.0, 100.0) for y in (0.0, 100.0) for z in (0.0, 100.0)])
    faces = np.array([[50.0, 50.0, 0.0], [50.0, 0.0, 50.0], [0.0, 50.0, 50.0], [50.0, 50.0, 100.0]])
    centres = np.concatenate([F.CENTRES * 100.0, corners, faces])
    yield "clustered displacement", centres, psi, 100.0, PR.profile_edges(0.5, 20.0, 12)
    rng = np.random.default_rng(8)
    yield "ncell 3", rng.uniform(0.0, 100.0, size=(40, 3)), rng.uniform(0.0, 100.0, size=(200, 3)), 100.0, (0.0, 10.0, 33.0)
    ten = rng.uniform(0.0, 100.0, size=(10, 3))
    yield "ncell 4096", ten, ten, 100.0, (0.0, 0.01, 0.02)
    for count in (255, 256, 257, 1000):
        c, m, L, e = PR.one_cell_case(count)
        yield "one cell of %d" % count, c, m, L, e
    yield "edges hit exactly", R.edge_points(), R.edge_points(), R.EDGE_L, R.EDGE_EDGES
    yield "1 bin", pos[:50], pos, R.UNIFORM_L, (0.0, 25.0)
    yield "128 bins", pos[:50], pos, R.UNIFORM_L, np.linspace(0.0, 30.0, 129)
    yield "H = 1, count_b = 1", pos[:1], pos[:1], R.UNIFORM_L, R.UNIFORM_EDGES
    yield "isothermal halo", np.array([PR.ISO_CENTRE]), PR.isothermal_halo(), PR.ISO_L, PR.ISO_EDGES


def write_catalogue(f, x):
    if x.ndim == 4:
        np.ascontiguousarray(x, np.float32).tofile(f)
        return 2, x.shape[1]
    np.ascontiguousarray(x).tofile(f)
    return (1 if x.dtype == np.float64 else 0), x.shape[0]


def walk(prog, tmp, a, b, L, edges):
    T = R.thresholds(edges, L)
    ref = PR.radial_counts(R.catalogue(a, L), R.catalogue(b, L), T)
    case, res = os.path.join(tmp, "case.bin"), os.path.join(tmp, "result.bin")
    with open(case, "wb") as f:
        f.write(b"\0" * (6 * 8))
        np.array([L], np.float64).tofile(f)
        np.array(T, np.int64).tofile(f)
        ka, ra = write_catalogue(f, a)
        kb, rb = write_catalogue(f, b)
        f.seek(0)
        np.array([ka, ra, kb, rb, R.ncell_of(T), len(T) - 1], np.int64).tofile(f)
    subprocess.run([prog, case, res], check=True)
    with open(res, "rb") as f:
        bad = np.fromfile(f, np.int64, 1)[0]
        tables = np.fromfile(f, np.int64).reshape((2,) + ref.shape)
    assert bad == 0
    assert np.array_equal(tables[0], ref), "workgroup form"
    assert np.array_equal(tables[1], ref), "wave form"
    return int(ref.sum()), R.ncell_of(T)


def main():
    prog = os.path.abspath(sys.argv[1])
    with tempfile.TemporaryDirectory() as tmp:
        for name, a, b, L, edges in cases():
            pairs, ncell = walk(prog, tmp, np.asarray(a), np.asarray(b), L, edges)
            print("%-28s %9d counted, ncell %4d: both forms equal to the reference" % (name, pairs, ncell))


if __name__ == "__main__":
    main()
