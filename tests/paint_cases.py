"""Case tables of tests/test_gpu_paint_limits.py, and the decisions of the three painters they are aimed at, restated in
NumPy float64 / Python integers.

The painters (csrc/nbe_density.hip: paint_kernel, paint_field_kernel, paint_particles_kernel)
  * a workgroup owns 512 particles: a Lagrangian tile of 8^3 lattice points (ragged at the lattice's far faces), or 512
    consecutive entries of `order` (the last chunk ragged);
  * a position is painted if |u| < 2^30 mesh cells on every axis, else counted in stats[1] and left out;
  * the footprint of the workgroup's painted particles is lo = min floor(u + 1 - P/2), hi = max floor(u + 1 - P/2) + P - 1
    per axis (footprint);
  * beyond_image: the footprint takes the direct path, and is counted in stats[0], if an extent or the product of the three
    exceeds the image: 16384 cells for paint_kernel, 8192 for the other two (direct_tiles, direct_chunks);
  * particle_keys_kernel: the tile of edge^3 cells that holds floor(u) mod res, row-major over ceil(res / edge) tiles per
    axis or with interleaved bits, INT64_MAX for a position that is not painted (keys).
The integers that reach the mesh do not depend on any of this; the float64 references are mas_ref / field_ref /
particles_ref.  tests/test_paint_cases.py holds every case to the property it was built for, on the CPU."""

import collections
import functools

import numpy as np

import mas_ref as R
import particles_ref as PR

U_MAX = 2.0 ** 30                  # kUMax
LDS_CELLS, FIELD_CELLS = 16384, 8192
TILE, CHUNK = 8, 512
KEY_NONE = np.iinfo(np.int64).max
WORDERS = (1, 2, 3, 4)

# disp: (3, N0, N1, N2) float32; rejected: particles that are not painted
Lattice = collections.namedtuple("Lattice", "name disp boxsize res rejected why")
# pos: (count, 3); shift: None or (axis, values float32, scale)
Catalogue = collections.namedtuple("Catalogue", "name pos boxsize res shift rejected why")


# ---- the painters' decisions, restated -------------------------------------------------------------------------------------
def accepted(u):
    """(count,) bool for (3, count) mesh coordinates: painted, i.e. finite and within 2^30 cells on every axis"""
    with np.errstate(invalid="ignore"):
        return (np.abs(np.asarray(u, np.float64)) < U_MAX).all(axis=0)


def footprint(u, P):
    """(lo, hi), int64 (3,): first and last node per axis touched by the particles at (3, count) coordinates u"""
    j = np.floor(np.asarray(u, np.float64).reshape(3, -1) + 1.0 - 0.5 * P).astype(np.int64)
    return j.min(axis=1), j.max(axis=1) + P - 1


def extents(u, P):
    lo, hi = footprint(u, P)
    return tuple(int(h) - int(l) + 1 for l, h in zip(lo, hi))


def beyond(ext, limit):
    """the footprint does not fit an image of `limit` cells (Python integers: the product is exact)"""
    e0, e1, e2 = (int(e) for e in ext)
    return max(e0, e1, e2) > limit or e0 * e1 * e2 > limit


def direct_tiles(u, n, P, limit):
    """stats[0] of a lattice painter: the 8^3 tiles of the (N0, N1, N2) lattice, ragged ones included, whose painted
    particles' footprint is beyond `limit` cells.  u: (3, N0 N1 N2) in lattice order (mas_ref.positions)."""
    n = tuple(int(v) for v in n)
    u = np.asarray(u, np.float64).reshape((3,) + n)
    ok = accepted(u.reshape(3, -1)).reshape(n)
    count = 0
    for t0 in range(0, n[0], TILE):
        for t1 in range(0, n[1], TILE):
            for t2 in range(0, n[2], TILE):
                sl = (slice(t0, t0 + TILE), slice(t1, t1 + TILE), slice(t2, t2 + TILE))
                live = ok[sl]
                if live.any() and beyond(extents(u[(slice(None),) + sl][:, live], P), limit):
                    count += 1
    return count


def direct_chunks(u, P, limit=FIELD_CELLS, order=None):
    """stats[0] of the catalogue painter: the chunks of 512 consecutive entries of `order` (None: the rows as they come)
    whose painted particles' footprint is beyond `limit` cells.  u: (3, count) (particles_ref.mesh_coordinates)."""
    u = np.asarray(u, np.float64)
    rows = np.arange(u.shape[1]) if order is None else np.asarray(order)
    count = 0
    for s in range(0, len(rows), CHUNK):
        uc = u[:, rows[s:s + CHUNK]]
        live = accepted(uc)
        if live.any() and beyond(extents(uc[:, live], P), limit):
            count += 1
    return count


def spread3(x):
    """bit b of x (below 2^20) at position 3 b"""
    x = np.asarray(x, np.int64)
    out = np.zeros_like(x)
    for b in range(20):
        out |= ((x >> b) & 1) << (3 * b)
    return out


def keys(u, res, edge, morton):
    """(count,) int64 of particle_keys_kernel for (3, count) mesh coordinates u"""
    u = np.asarray(u, np.float64)
    ok = accepted(u)
    t = [np.mod(np.floor(u[c][ok]).astype(np.int64), int(res[c])) // edge for c in range(3)]
    T = [(int(r) + edge - 1) // edge for r in res]
    out = np.full(u.shape[1], KEY_NONE, np.int64)
    out[ok] = (spread3(t[0]) << 2 | spread3(t[1]) << 1 | spread3(t[2])) if morton else (t[0] * T[1] + t[1]) * T[2] + t[2]
    return out


def rows_of(case):
    """(count, 3) float64 positions of a lattice case in lattice order: the catalogue painter's input for the same
    particles.  Where boxsize = res they are the mesh coordinates themselves."""
    return PR.lattice_positions(case.disp, case.boxsize)


# ---- threshold: a footprint of exactly the image, and the next ones ------------------------------------------------------------
# name -> (lattice, extents, worders).  The lattice is one tile; boxsize = res = lattice, so that a = s = 1 and u = i + psi
# is exact.  Undisplaced, a tile of n points spans n + P - 1 nodes per axis; the last particle alone is moved up by the rest.
THRESHOLD = {
    "lds-fit": ((8, 8, 8), (32, 32, 16), WORDERS),           # 16384 = the 32-bit image: LDS in paint_kernel
    "lds-beyond": ((8, 8, 8), (32, 32, 17), WORDERS),        # one more plane of nodes
    "lds-next": ((2, 2, 2), (5, 29, 113), WORDERS),          # 16385 cells: one cell more than the image
    "field-fit": ((8, 8, 8), (16, 16, 32), WORDERS),         # 8192 = the 64-bit image of the field and catalogue painters
    "field-beyond": ((8, 8, 8), (16, 16, 33), WORDERS),
    "field-next": ((2, 2, 1), (3, 2731, 1), (1,)),           # 8193 = 3 x 2731 cells: an extent of 1 needs NGP and one plane
}


def threshold(kind, P):
    n, ext, worders = THRESHOLD[kind]
    assert P in worders
    disp = np.zeros((3,) + n, np.float32)
    for c in range(3):
        d = ext[c] - (n[c] + P - 1)
        assert d >= 0
        disp[c][-1, -1, -1] = d
    L = tuple(float(v) for v in n)
    return Lattice("threshold-%s-P%d" % (kind, P), disp, L, n, 0,
                   "one tile whose footprint is %d x %d x %d = %d nodes" % (ext + (ext[0] * ext[1] * ext[2],)))


# ---- overflow: extents whose product does not fit 64 bits ---------------------------------------------------------------------
def overflow():
    disp = np.zeros((3, 8, 8, 8), np.float32)
    disp[:, 1, 2, 3] = 2.0 ** 20 + 64.25
    disp[:, 6, 5, 4] = -(2.0 ** 20 + 64.5)
    return Lattice("overflow", disp, (16.0,) * 3, (16,) * 3, 0,
                   "extents of about 2^21 nodes per axis: their product is 2^63 or more and wraps negative in int64")


# ---- range: the position limit from both sides ---------------------------------------------------------------------------------
RANGE = [(axis, sign) for axis in range(3) for sign in (1, -1)]


def in_range(axis, sign, reject):
    """Lattice 2^3, boxsize = res = 4: a = 2, s = 1, u = 2 i + psi.  Particle (0, 0, 0) sits at sign (2^30 - 64) cells on
    `axis`, exact in float32 and painted.  With `reject` the particle with index 0 on `axis` and 1 on the other two sits at
    sign 2^30 exactly, and is not."""
    disp = np.zeros((3, 2, 2, 2), np.float32)
    disp[axis, 0, 0, 0] = sign * (2.0 ** 30 - 64.0)
    if reject:
        idx = [1, 1, 1]
        idx[axis] = 0
        disp[(axis,) + tuple(idx)] = sign * 2.0 ** 30
    return Lattice("range-%s-axis%d%s" % ("reject" if reject else "accept", axis, "+" if sign > 0 else "-"), disp,
                   (4.0,) * 3, (4,) * 3, int(reject), "|u| = 2^30 - 64 is painted%s" % (", |u| = 2^30 is not" if reject else ""))


# ---- tiny meshes: several nodes of one particle alias onto one cell ---------------------------------------------------------------
TINY_MESHES = [(1, 1, 1), (2, 3, 1), (3, 2, 5)]


@functools.lru_cache(maxsize=None)
def _tiny_disp():
    rng = np.random.default_rng(505)
    n, L = (5, 9, 3), (7.0, 9.0, 11.0)
    return np.stack([rng.standard_normal(n) * 2.0 * (L[c] / n[c]) for c in range(3)]).astype(np.float32)


def tiny_mesh(res):
    return Lattice("tiny-mesh-%dx%dx%d" % tuple(res), _tiny_disp(), (7.0, 9.0, 11.0), tuple(res), 0,
                   "res < worder: the LDS image keeps a particle's nodes apart, the flush wraps them together")


# ---- ragged lattices on the plain painter --------------------------------------------------------------------------------------
RAGGED = {(1, 1, 1): (1, 2), (3, 5, 9): (1, 2), (9, 8, 7): (1, 2), (20, 20, 20): (0.5, 1, 2)}     # lattice -> res / N


@functools.lru_cache(maxsize=None)
def _ragged_disp(n):
    rng = np.random.default_rng(600 + sum(n))
    return (rng.standard_normal((3,) + n) * 1.5 * 12.5).astype(np.float32)


def ragged(n, scale):
    res = tuple(int(v * scale) for v in n)
    assert all(r == v * scale for r, v in zip(res, n))
    return Lattice("ragged-%dx%dx%d-res%dx%dx%d" % (n + res), _ragged_disp(n), tuple(12.5 * v for v in n), res, 0,
                   "tiles of 8 do not divide the lattice; displacements of 1.5 lattice cells rms")


# ---- ties: positions on nodes and half-way between them ------------------------------------------------------------------------
TIE_RES = 9
TIES = (-1.5, -1.0, -0.5, -0.0, 0.0, 0.5, 1.0, TIE_RES - 0.5, float(TIE_RES))


def ties():
    """A 9^3 lattice, boxsize = res = 9 (a = s = 1): particle (i, j, k) sits at (TIES[i], TIES[j], TIES[k]) exactly.
    (u = i + psi: the lattice painters see +0.0 where the catalogue painter sees -0.0.)"""
    t = np.asarray(TIES)
    idx = np.indices((9, 9, 9))
    disp = np.stack([t[idx[c]] - idx[c] for c in range(3)]).astype(np.float32)
    return Lattice("ties", disp, (float(TIE_RES),) * 3, (TIE_RES,) * 3, 0,
                   "every combination of a node, a half-way point, -0.0, 0 and the far face per axis: NGP's half-way-goes-up, "
                   "TSC's d = -1/2, negative u next to 0")


def tie_rows():
    """the (729, 3) positions themselves, -0.0 included, for the catalogue painter"""
    t = np.asarray(TIES)
    idx = np.indices((9, 9, 9)).reshape(3, -1)
    return Catalogue("ties-rows", np.stack([t[idx[c]] for c in range(3)], axis=1), (float(TIE_RES),) * 3, (TIE_RES,) * 3,
                     None, 0, "the tie positions as rows")


# ---- keys ------------------------------------------------------------------------------------------------------------------------
KEY_RES, KEY_BOX = (24, 20, 36), (12.0, 10.0, 18.0)        # s = 2 on every axis: x s is exact
KEY_EDGES = (4, 8, 16)                                     # 16 divides none of 24, 20, 36
KEY_NAN_ROW, KEY_FAR_ROW, KEY_EDGE_ROW = 17, 1234, 1235


@functools.lru_cache(maxsize=None)
def key_catalogue(dtype, shifted):
    """2000 rows: 1200 inside the box, 500 up to five boxes away on either side, 300 at negative u within one cell of 0
    (down to -1e-20), of which one is NaN, one sits at 2^30 cells (rejected) and one at 2^30 - 64 (painted).  The shift
    along axis 1 is a multiple of 2^-6 times a scale of 0.5, so that v vs is exact: x s + v vs is rounded once, however
    the compiler contracts it."""
    rng = np.random.default_rng(77)
    L = np.asarray(KEY_BOX)
    x = np.concatenate([rng.uniform(0.0, 1.0, (1200, 3)) * L, rng.uniform(-5.0, 6.0, (500, 3)) * L,
                        -rng.uniform(0.0, 0.5, (300, 3)) * 10.0 ** rng.integers(-20, 1, (300, 3))])
    x = x[rng.permutation(len(x))]
    x[KEY_NAN_ROW, 1] = np.nan
    x[KEY_FAR_ROW, 0] = 2.0 ** 29
    x[KEY_EDGE_ROW, 2] = -(2.0 ** 29 - 32.0)
    x = x.astype(dtype)
    shift = None
    if shifted:
        v = (rng.integers(-512, 513, len(x)) / 64.0).astype(np.float32)
        v[KEY_FAR_ROW] = v[KEY_EDGE_ROW] = 0.0
        shift = (1, v, 0.5)
    return Catalogue("keys-%s%s" % (np.dtype(dtype).name, "-shifted" if shifted else ""), x, KEY_BOX, KEY_RES, shift, 2,
                     "rows in the box, boxes away, at negative u next to 0, a NaN and the position limit")


# ---- references, computed once ---------------------------------------------------------------------------------------------------
def lattice_u(case):
    return R.positions(case.disp, case.boxsize, case.res)


def catalogue_u(case):
    return PR.mesh_coordinates(case.pos, case.boxsize, case.res, case.shift)


def painted_rows(case):
    """(pos, shift) of a catalogue case without the rows that are not painted: what particles_ref.paint is given"""
    ok = accepted(catalogue_u(case))
    shift = None if case.shift is None else (case.shift[0], case.shift[1][ok], case.shift[2])
    return np.asarray(case.pos, np.float64)[ok], shift
