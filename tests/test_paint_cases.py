"""The case tables of tests/paint_cases.py held to their purpose with the NumPy references alone: every limit of the three
painters that a case was built for is named here, so that a table cannot be thinned out unnoticed.  CPU only."""

import numpy as np
import pytest

import mas_ref as R
import paint_cases as PC
import particles_ref as PR


def _lattice_cases():
    out = [PC.threshold(kind, P) for kind, (_, _, worders) in PC.THRESHOLD.items() for P in worders]
    out += [PC.overflow(), PC.ties()]
    out += [PC.in_range(axis, sign, False) for axis, sign in PC.RANGE]
    out += [PC.tiny_mesh(res) for res in PC.TINY_MESHES]
    out += [PC.ragged(n, s) for n, scales in PC.RAGGED.items() for s in scales]
    return out


def test_names_are_unique_and_every_case_says_why():
    cases = _lattice_cases() + [PC.in_range(axis, sign, True) for axis, sign in PC.RANGE] + [PC.tie_rows()]
    cases += [PC.key_catalogue(dt, sh) for dt in (np.float32, np.float64) for sh in (False, True)]
    names = [c.name for c in cases]
    assert len(set(names)) == len(names)
    assert all(len(c.why) > 5 for c in cases)
    for c in cases:
        if isinstance(c, PC.Lattice):
            assert c.disp.dtype == np.float32 and max(c.disp.shape[1:]) <= 20 and max(c.res) <= 48
        else:
            assert len(c.pos) <= 2048 and max(c.res) <= 48


@pytest.mark.parametrize("P", PC.WORDERS)
def test_threshold_cases_have_exactly_the_stated_extents(P):
    for kind, (n, ext, worders) in PC.THRESHOLD.items():
        if P not in worders:
            continue
        c = PC.threshold(kind, P)
        u = PC.lattice_u(c)
        assert np.array_equal(u, PC.rows_of(c).T)                       # a = s = 1: both painters' positions, exactly
        assert PC.extents(u, P) == ext
        cells = ext[0] * ext[1] * ext[2]
        for limit in (PC.LDS_CELLS, PC.FIELD_CELLS):
            assert PC.direct_tiles(u, n, P, limit) == int(cells > limit)
            assert PC.direct_chunks(u, P, limit) == int(cells > limit)
    cells = {k: int(np.prod(v[1])) for k, v in PC.THRESHOLD.items()}
    assert cells["lds-fit"] == PC.LDS_CELLS and cells["lds-next"] == PC.LDS_CELLS + 1 and cells["lds-beyond"] > PC.LDS_CELLS
    assert cells["field-fit"] == PC.FIELD_CELLS and cells["field-next"] == PC.FIELD_CELLS + 1
    assert cells["field-beyond"] > PC.FIELD_CELLS
    # what the exact-count tests would not see without these cases: a limit that is one cell off, either way
    u, n = PC.lattice_u(PC.threshold("lds-fit", P)), (8, 8, 8)
    assert [PC.direct_tiles(u, n, P, PC.LDS_CELLS + d) for d in (-1, 0, 1)] == [1, 0, 0]
    u, n = PC.lattice_u(PC.threshold("lds-next", P)), (2, 2, 2)
    assert [PC.direct_tiles(u, n, P, PC.LDS_CELLS + d) for d in (-1, 0, 1)] == [1, 1, 0]
    u = PC.lattice_u(PC.threshold("field-fit", P))
    assert [PC.direct_chunks(u, P, PC.FIELD_CELLS + d) for d in (-1, 0, 1)] == [1, 0, 0]


@pytest.mark.parametrize("P", PC.WORDERS)
def test_overflow_case_wraps_the_64_bit_product(P):
    c = PC.overflow()
    u = PC.lattice_u(c)
    assert np.array_equal(u, PC.rows_of(c).T) and np.array_equal(u.astype(np.float32).astype(np.float64), u)
    assert PC.accepted(u).all()
    ext = PC.extents(u, P)
    assert all(2 ** 21 + 118 <= e <= 2 ** 21 + 132 for e in ext)       # 2 (2^20 + 64.x) less 10, 6, 2 lattice cells, plus P
    assert ext[0] * ext[1] * ext[2] >= 2 ** 63                          # exact
    with np.errstate(over="ignore"):
        wrapped = int(np.prod(np.asarray(ext, np.int64)))               # what e0 * e1 * e2 is in long long
    assert wrapped <= PC.LDS_CELLS and wrapped < -9.2e18
    assert PC.beyond(ext, PC.LDS_CELLS) and PC.direct_tiles(u, (8, 8, 8), P, PC.LDS_CELLS) == 1
    assert PC.direct_chunks(u, P) == 1


@pytest.mark.parametrize("P", PC.WORDERS)
def test_reference_conserves_the_mass_of_every_lattice_case(P):
    for c in _lattice_cases():
        if c.name.startswith("threshold") and not c.name.endswith("P%d" % P):
            continue
        mass, _ = R.paint(c.disp, c.boxsize, c.res, P)
        assert abs(mass.sum() - c.disp[0].size) <= 1e-9, c.name
        assert PC.accepted(PC.lattice_u(c)).all()


def test_range_cases_are_exact_in_their_input_dtype():
    for axis, sign in PC.RANGE:
        for reject in (False, True):
            c = PC.in_range(axis, sign, reject)
            u = PC.lattice_u(c)
            x = PC.rows_of(c)
            assert np.array_equal(x.T, u)                                # boxsize = res
            assert np.array_equal(x.astype(np.float32).astype(np.float64), x)
            assert u[axis, 0] == sign * (2.0 ** 30 - 64.0)
            ok = PC.accepted(u)
            assert np.count_nonzero(~ok) == c.rejected == int(reject)
            if reject:
                assert np.abs(u[:, ~ok]).max() == 2.0 ** 30
            # the painted particles are 2^30 cells apart: the direct path in every painter
            for P in PC.WORDERS:
                assert PC.direct_tiles(u, (2, 2, 2), P, PC.LDS_CELLS) == 1 and PC.direct_chunks(u, P) == 1
                _, mass, _, _ = PR.paint(x[ok], c.boxsize, c.res, P)
                assert abs(mass.sum() - (8 - c.rejected)) <= 1e-9


def test_tiny_meshes_are_smaller_than_the_windows():
    assert PC.TINY_MESHES == [(1, 1, 1), (2, 3, 1), (3, 2, 5)]
    c = PC.tiny_mesh((2, 3, 1))
    assert c.disp.shape == (3, 5, 9, 3) and c.boxsize == (7.0, 9.0, 11.0)
    for c in range(3):
        rms = PC._tiny_disp()[c].std() / ((7.0, 9.0, 11.0)[c] / (5, 9, 3)[c])
        assert 1.5 < rms < 2.5


def test_ragged_table():
    assert set(PC.RAGGED) == {(1, 1, 1), (3, 5, 9), (9, 8, 7), (20, 20, 20)}
    assert PC.RAGGED[(20, 20, 20)] == (0.5, 1, 2)
    assert any(v % PC.TILE for n in PC.RAGGED for v in n)
    assert PC.ragged((20, 20, 20), 0.5).res == (10, 10, 10) and PC.ragged((9, 8, 7), 2).res == (18, 16, 14)


@pytest.mark.parametrize("P", PC.WORDERS)
def test_ties_sit_where_they_say_and_the_reference_is_exact(P):
    c, rows = PC.ties(), PC.tie_rows()
    u = PC.lattice_u(c)
    assert np.array_equal(u, rows.pos.T) and u.shape == (3, 729)
    assert {float(v) for v in u[0]} == {float(t) for t in PC.TIES}
    assert np.signbit(rows.pos).any() and (rows.pos[np.signbit(rows.pos)] == 0).any()          # a -0.0 among the rows
    assert np.array_equal(PC.catalogue_u(rows), rows.pos.T)
    # the rules the case is about, one particle at a time
    j, w = R.nodes(np.array([0.5, -0.5, -1.5, PC.TIE_RES - 0.5]), 1)
    assert j.tolist() == [1, 0, -1, PC.TIE_RES]                          # NGP: half-way goes up
    j, w = R.nodes(np.array([0.5]), 3)
    assert j.tolist() == [0] and w[0].tolist() == [0.5, 0.5, 0.0]        # TSC at d = -1/2: the third node gets nothing
    j, w = R.nodes(np.array([-0.0, 0.0, -0.5]), 2)
    assert j.tolist() == [0, 0, -1] and w.tolist() == [[1.0, 0.0], [1.0, 0.0], [0.5, 0.5]]
    # NGP, CIC and TSC weights at these positions are dyadic, so the float64 reference is exact; PCS has multiples of
    # 1/48 and 1/6, exact to a rounding of float64
    mass, _ = R.paint(c.disp, c.boxsize, c.res, P)
    scale = 2.0 ** 9 if P < 4 else 2.0 ** 9 * 48 ** 3
    assert np.abs(mass * scale - np.rint(mass * scale)).max() <= (0 if P < 4 else 1e-13 * mass.max() * scale)
    assert abs(mass.sum() - 729) <= (0 if P < 4 else 1e-9)
    _, mass_rows, _, _ = PR.paint(rows.pos, rows.boxsize, rows.res, P)
    assert np.array_equal(mass_rows, mass)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("shifted", [False, True])
def test_keys_mark_exactly_the_rows_that_are_not_painted(dtype, shifted):
    c = PC.key_catalogue(dtype, shifted)
    assert c.pos.dtype == dtype and c.pos.shape == (2000, 3) and c.res == (24, 20, 36)
    assert all(r % 16 for r in c.res) and PC.KEY_EDGES == (4, 8, 16)
    u = PC.catalogue_u(c)
    ok = PC.accepted(u)
    assert np.flatnonzero(~ok).tolist() == [PC.KEY_NAN_ROW, PC.KEY_FAR_ROW] and c.rejected == 2
    assert u[0, PC.KEY_FAR_ROW] == 2.0 ** 30 and u[2, PC.KEY_EDGE_ROW] == -(2.0 ** 30 - 64.0)
    inside = ((u >= 0) & (u < np.asarray(c.res)[:, None])).all(axis=0)
    near = ((u > -1) & (u < 0)).any(axis=0)
    assert inside.sum() >= 800 and (~inside & ok).sum() >= 500 and near.sum() >= 250
    assert (u[:, ok].min(axis=1) < -3 * np.asarray(c.res)).all() and (u[:, ok].max(axis=1) > 4 * np.asarray(c.res)).all()
    if shifted:
        axis, v, scale = c.shift
        assert axis == 1 and v.dtype == np.float32 and np.count_nonzero(v) > 1900
        assert np.array_equal(v * 64.0, np.rint(v * 64.0)) and scale * c.res[1] / c.boxsize[1] == 1.0
    pos, shift = PC.painted_rows(c)
    for P in (1, 4):
        _, mass, _, _ = PR.paint(pos, c.boxsize, c.res, P, shift=shift)
        assert abs(mass.sum() - (2000 - c.rejected)) <= 1e-9
    for edge in PC.KEY_EDGES:
        T = [(r + edge - 1) // edge for r in c.res]
        for morton in (False, True):
            k = PC.keys(u, c.res, edge, morton)
            assert k.dtype == np.int64 and np.array_equal(k == PC.KEY_NONE, ~ok)
            assert k[ok].min() == 0
            if not morton:
                assert k[ok].max() == T[0] * T[1] * T[2] - 1 and len(np.unique(k[ok])) >= 0.9 * T[0] * T[1] * T[2]
                # a row at negative u within a cell of 0 belongs to the last tile of its axis
                row = np.flatnonzero(ok & (u[2] > -1) & (u[2] < 0))[0]
                assert k[row] % T[2] == T[2] - 1
        # both keys order the same tiles: equal row-major keys, equal Morton keys
        a, b = PC.keys(u, c.res, edge, False)[ok], PC.keys(u, c.res, edge, True)[ok]
        assert len(np.unique(a)) == len(np.unique(b)) == len(set(zip(a.tolist(), b.tolist())))


def test_spread3_interleaves():
    assert PC.spread3(np.array([0, 1, 2, 3, 5, 2 ** 19])).tolist() == [0, 1, 8, 9, 65, 2 ** 57]
