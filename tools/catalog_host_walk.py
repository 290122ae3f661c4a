#!/usr/bin/env python
"""Drive tools/catalog_host_walk.hip: write the small cases of the FoF, pair-count, profile and velocity-moment tests, run the
host program (built under -fsanitize=address,undefined, see its head) on each and compare what the bodies of
csrc/nbe_catalog.h produced with tests/fof_ref.py, tests/pairs_ref.py, tests/profiles_ref.py and tests/pairvel_ref.py.  A CPU
machine only: nothing here touches a device.

    python tools/catalog_host_walk.py ./catalog_host_walk [fof|pairs|profiles|velocity ...]

tests/test_catalog_host_walk.py and tests/test_pairvel_host_walk.py run the same cases on a build without the sanitizers.
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
import pairvel_ref as V  # noqa: E402


def fof_cases():
    """(name, psi, L, velocity or None, keywords of F.fof)"""
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


def pairs_cases():
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


def profiles_cases():
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
    """The array of a catalogue into the case file; its (kind, rows) for the header (see the head of the program)."""
    if x is None:
        return -1, 0
    x = np.asarray(x)
    if x.ndim == 4:
        half = x.dtype == np.float16
        np.ascontiguousarray(x, np.float16 if half else np.float32).tofile(f)
        return (3 if half else 2), x.shape[1]
    np.ascontiguousarray(x).tofile(f)
    return (1 if x.dtype == np.float64 else 0), x.shape[0]


def run(prog, mode, tmp, header, write_body):
    """Write a case (the int64 header is known only once write_body has written the catalogues), run the program on it and
    return the open result file."""
    case, res = os.path.join(tmp, "case.bin"), os.path.join(tmp, "result.bin")
    with open(case, "wb") as f:
        f.write(b"\0" * (8 * header))
        head = write_body(f)
        assert len(head) == header
        f.seek(0)
        np.array(head, np.int64).tofile(f)
    subprocess.run([prog, mode, case, res], check=True)
    return open(res, "rb")


def walk_fof(prog, tmp, psi, L, v, kw):
    ref = F.fof(psi, L, velocity=v, **kw)
    e = F.velocity_exponents(v) if v is not None else np.zeros(3, np.int64)

    def body(f):
        np.array([L], np.float64).tofile(f)
        e.astype(np.int32).tofile(f)
        kind, n = write_catalogue(f, psi)
        if v is not None:
            np.ascontiguousarray(v, np.float32).tofile(f)
        return [kind, n, F.ncell_of(ref["R2"]), ref["R2"], kw["nmin"], v is not None]

    with run(prog, "fof", tmp, 6, body) as f:
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
    return "%5d halos of %6d groups: equal to the reference" % (rows, ref["ngroups"])


def walk_pairs(prog, tmp, a, b, L, edges, nmu, los):
    T = R.thresholds(edges, L)
    ref = R.pair_counts(R.catalogue(a, L), T, None if b is None else R.catalogue(b, L), nmu=nmu, los=los)

    def body(f):
        np.array([L], np.float64).tofile(f)
        np.array(T, np.int64).tofile(f)
        return [*write_catalogue(f, a), *write_catalogue(f, b), R.ncell_of(T), len(T) - 1, nmu or 1, los]

    with run(prog, "pairs", tmp, 8, body) as f:
        bad = np.fromfile(f, np.int64, 1)[0]
        counts = np.fromfile(f, np.int64).reshape(len(T) - 1, nmu or 1)
    assert bad == 0
    assert np.array_equal(counts if nmu else counts[:, 0], ref), "counts"
    return "%9d pairs, ncell %4d: equal to the reference" % (int(ref.sum()), R.ncell_of(T))


def walk_profiles(prog, tmp, a, b, L, edges):
    T = R.thresholds(edges, L)
    ref = PR.radial_counts(R.catalogue(a, L), R.catalogue(b, L), T)

    def body(f):
        np.array([L], np.float64).tofile(f)
        np.array(T, np.int64).tofile(f)
        return [*write_catalogue(f, a), *write_catalogue(f, b), R.ncell_of(T), len(T) - 1]

    with run(prog, "profiles", tmp, 6, body) as f:
        bad = np.fromfile(f, np.int64, 1)[0]
        tables = np.fromfile(f, np.int64).reshape((2,) + ref.shape)
    assert bad == 0
    assert np.array_equal(tables[0], ref), "workgroup form"
    assert np.array_equal(tables[1], ref), "wave form"
    return "%9d counted, ncell %4d: both forms equal to the reference" % (int(ref.sum()), R.ncell_of(T))


def velocity_cases():
    """(name, a, va or None, b or None, vb, L, edges): tests/pairvel_ref.py's list"""
    return V.cases()


def write_velocity(f, v, x):
    """The velocity v of the catalogue x in the layout and dtype of x's kind."""
    x = np.asarray(x)
    w = np.ascontiguousarray(v, x.dtype if x.ndim == 4 or x.dtype == np.float64 else np.float32)
    assert np.array_equal(w.astype(np.float64), np.asarray(v).astype(np.float64)), "the case file's dtype would round the velocity"
    w.tofile(f)


def walk_velocity(prog, tmp, a, va, b, vb, L, edges):
    T = R.thresholds(edges, L)
    nb = len(T) - 1
    e = V.exponent(va, vb)
    pairs = None if va is None else V.moments_of(a, va, L, edges, b, vb)[0]
    tables = None if b is None or np.asarray(a).ndim == 4 else V.profiles_of(a, va, b, vb, L, edges)[0]

    def body(f):
        np.array([L], np.float64).tofile(f)
        np.array(T, np.int64).tofile(f)
        ka = write_catalogue(f, a)
        if va is not None:
            write_velocity(f, va, a)
        kb = write_catalogue(f, b)
        if b is not None:
            write_velocity(f, vb, b)
        return [*ka, *kb, R.ncell_of(T), nb, e, va is not None]

    with run(prog, "velocity", tmp, 8, body) as f:
        bad = np.fromfile(f, np.int64, 1)[0]
        got = np.fromfile(f, np.int64, 6 * nb).reshape(nb, 6)
        rest = np.fromfile(f, np.int64)
    assert bad == 0
    if pairs is not None:
        assert np.array_equal(got, pairs), "pair moments"
    if tables is not None:
        both = rest.reshape((2,) + tables.shape)
        assert np.array_equal(both[0], tables), "workgroup form"
        assert np.array_equal(both[1], tables), "wave form"
    else:
        assert rest.size == 0 or np.asarray(a).ndim == 4
    n = int((pairs if pairs is not None else tables.sum(axis=0))[:, 0].sum())
    return "%9d pairs, ncell %4d, e %3d: equal to the reference" % (n, R.ncell_of(T), e)


MODES = {"fof": (fof_cases, walk_fof), "pairs": (pairs_cases, walk_pairs), "profiles": (profiles_cases, walk_profiles),
         "velocity": (velocity_cases, walk_velocity)}


def walk_mode(prog, mode, report=None):
    """Every case of a mode through the program; an AssertionError where one differs from the reference.  Returns their
    number."""
    cases, walk = MODES[mode]
    done = 0
    with tempfile.TemporaryDirectory() as tmp:
        for name, *case in cases():
            line = walk(prog, tmp, *case)
            if report:
                report("%-9s %-28s %s" % (mode, name, line))
            done += 1
    return done


def main():
    prog = os.path.abspath(sys.argv[1])
    for mode in sys.argv[2:] or list(MODES):
        walk_mode(prog, mode, print)


if __name__ == "__main__":
    main()
