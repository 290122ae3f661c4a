"""The three mass-assignment painters on the MI355X (csrc/nbe_density.hip: paint_kernel, paint_field_kernel,
paint_particles_kernel) at the limits their branches are written around, on the cases of tests/paint_cases.py: footprints of
exactly the LDS image and just beyond it, extents whose product does not fit 64 bits, the position limit from both sides,
meshes smaller than the window, ragged lattices, exact ties, and the sort keys.  Every result is held to the float64
references with the bounds of test_gpu_density.check_paint, test_gpu_particles.check_delta and field_ref, unchanged;
stats[0] is held to the exact number of tiles or chunks that paint_cases predicts."""

import ctypes as C
import functools

import numpy as np
import pytest

import field_ref as F
import mas_ref as R
import paint_cases as PC
import particles_ref as PR
from test_gpu_density import check_paint, smooth_field
from test_gpu_particles import bits, check_delta

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -22


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


def _t(a):
    return None if a is None else _torch().from_numpy(np.ascontiguousarray(a)).cuda()


def _floats(v):
    return tuple(float(x) for x in v)


# ---- the painters, with their stats ----------------------------------------------------------------------------------------------
def plain(case, P, disp=None):
    """paint_kernel: (delta, [direct tiles, rejected])"""
    from jax_nbody_emulator_with_dj_amd import density as D
    delta, stats = D._paint(_t(case.disp if disp is None else disp), _floats(case.boxsize), tuple(case.res), P, False)
    return delta.cpu().numpy(), stats.cpu().tolist()[:2]


def field(case, P, q=None, normalize="mean"):
    """paint_field_kernel: (field or None, delta, [direct tiles, rejected, cells at the mass limit])"""
    from jax_nbody_emulator_with_dj_amd import density as D
    f, delta, stats = D._paint_fields(_t(case.disp), _t(q), None, 0, 0.0, tuple(case.disp.shape[1:]), _floats(case.boxsize),
                                      tuple(case.res), P, normalize, 0.0, True)
    return None if f is None else f.cpu().numpy(), delta.cpu().numpy(), stats.cpu().tolist()[:3]


def rows(pos, boxsize, res, P):
    """paint_particles_kernel on the rows as they come: (delta, [direct chunks, rejected])"""
    from jax_nbody_emulator_with_dj_amd import density as D
    _, delta, stats = D._paint_particles(_t(pos), None, None, 0, 0.0, _floats(boxsize), tuple(res), P, sort=False,
                                         want_delta=True)
    return delta.cpu().numpy(), stats.cpu().tolist()[:2]


def raw_rows(pos, boxsize, res, P, order=None, shift=None):
    """nbe_paint_particles with an explicit order (None: the identity): (int64 mass mesh, [direct chunks, rejected])"""
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd import _lib, density as D
    p, o = _t(pos), _t(None if order is None else np.asarray(order, np.int64))
    axis, v, scale = (0, None, 0.0) if shift is None else shift
    v = _t(v)
    mesh = torch.zeros(tuple(res), dtype=torch.int64, device=p.device)
    stats = torch.zeros(4, dtype=torch.int32, device=p.device)
    _lib.check(_lib.lib().nbe_paint_particles(D._ptr(p), 2 if p.dtype == torch.float64 else 0, D._ptr_or_null(o), None, 0, 0,
                                              (C.c_int * 4)(), D._ptr_or_null(v), 0, int(axis), float(scale), len(pos),
                                              (C.c_double * 3)(*_floats(boxsize)), D._i64(res), P, D._ptr(mesh), None,
                                              D._ptr(stats), D._stream(p.device)))
    return mesh.cpu().numpy(), stats.cpu().tolist()[:2]


def device_keys(case, edge, morton):
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd import _lib, density as D
    p = _t(case.pos)
    axis, v, scale = (0, None, 0.0) if case.shift is None else case.shift
    v = _t(v)
    k = torch.empty(len(case.pos), dtype=torch.int64, device=p.device)
    _lib.check(_lib.lib().nbe_particle_keys(D._ptr(p), 2 if p.dtype == torch.float64 else 0, D._ptr_or_null(v), 0, int(axis),
                                            float(scale), len(case.pos), (C.c_double * 3)(*_floats(case.boxsize)),
                                            D._i64(case.res), edge, int(morton), D._ptr(k), D._stream(p.device)))
    return k.cpu().numpy()


def same_rows(case):
    """(pos, boxsize) that give the catalogue painter the lattice case's particles.  Where boxsize = res, i a + psi s and
    x s are the same float64.  Elsewhere (tiny-mesh) the rows are the mesh coordinates i a + psi s of mas_ref.positions in a
    box of res cells: the lattice kernels contract that expression into one fused multiply-add, so their u can differ from it
    in the last bit of a float64, which moves a weight by 1e-16 and a fixed-point weight only if 2^22 S lies that close to a
    half-integer."""
    if _floats(case.boxsize) == _floats(case.res):
        return PC.rows_of(case), case.boxsize
    return PC.lattice_u(case).T.copy(), _floats(case.res)


def quantity(case, seed=9):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((2,) + case.disp.shape[1:]) * np.array([1.0, 300.0])[:, None, None, None]).astype(np.float32)


def three_kernels(case, P, dtypes=(np.float64,)):
    """One answer from three kernels: the plain painter against the reference, the other two bit for bit against it, and the
    exact path counts of all three.  Returns the delta."""
    u = PC.lattice_u(case)
    n = case.disp.shape[1:]
    a, sa = plain(case, P)
    check_paint(case.disp, case.boxsize, case.res, P, gpu=a)
    _, b, sb = field(case, P)
    print("%s P%d: direct tiles %d (plain), %d (field)" % (case.name, P, sa[0], sb[0]))
    assert sa == [PC.direct_tiles(u, n, P, PC.LDS_CELLS), 0]
    assert sb == [PC.direct_tiles(u, n, P, PC.FIELD_CELLS), 0, 0]
    assert np.array_equal(bits(b), bits(a))
    pos, L = same_rows(case)
    for dt in dtypes:
        c, sc = rows(pos.astype(dt), L, case.res, P)
        assert sc == [PC.direct_chunks(PR.mesh_coordinates(pos, L, case.res), P), 0]
        assert np.array_equal(bits(c), bits(a)), (case.name, P, dt)
    return a


def with_quantity(case, P):
    """two channels through the field painter against field_ref, both normalisations"""
    q = quantity(case)
    ref = F.paint(case.disp, q, case.boxsize, case.res, P)
    mean, delta, st = field(case, P, q, "mean")
    assert st[1:] == [0, 0]
    F.check_mean(mean, q, ref, case.disp[0].size)
    dens, _, _ = field(case, P, q, "density")
    F.check_density(dens, q, ref)
    return delta


# ---- 1. thresholds, overflow, tiny meshes, the accepted limit: one answer from three kernels ------------------------------------
@pytest.mark.parametrize("kind,P", [(kind, P) for kind in sorted(PC.THRESHOLD) for P in PC.THRESHOLD[kind][2]])
def test_footprint_at_the_image_limit(kind, P):
    """32 x 32 x 16 nodes fill paint_kernel's image exactly and stay in LDS, 32 x 32 x 17 and 5 x 29 x 113 = 16385 do not;
    16 x 16 x 32 against 16 x 16 x 33 and 3 x 2731 x 1 = 8193 for the 8192-cell image of the other two."""
    case = PC.threshold(kind, P)
    ext = PC.THRESHOLD[kind][1]
    cells = ext[0] * ext[1] * ext[2]
    a = three_kernels(case, P, (np.float32, np.float64))
    assert plain(case, P)[1][0] == int(cells > PC.LDS_CELLS)
    assert field(case, P)[2][0] == int(cells > PC.FIELD_CELLS)
    assert np.array_equal(bits(with_quantity(case, P)), bits(a))


@pytest.mark.parametrize("P", PC.WORDERS)
def test_extents_whose_product_overflows_take_the_direct_path(P):
    """Two particles of one tile 2^21 cells apart on every axis: e0 e1 e2 >= 2^63 is negative in int64.  Every kernel takes
    the direct path, rejects nothing and conserves the 512 masses."""
    case = PC.overflow()
    a = three_kernels(case, P, (np.float32, np.float64))
    assert plain(case, P)[1] == [1, 0] and field(case, P)[2] == [1, 0, 0]
    pos, L = same_rows(case)
    mesh, st = raw_rows(pos, L, case.res, P)
    assert st == [1, 0] and int(mesh.sum()) == 512 << 22
    assert (a.astype(np.float64) + 1.0).sum() / 8.0 == pytest.approx(512, rel=1e-6)
    assert np.array_equal(bits(with_quantity(case, P)), bits(a))


@pytest.mark.parametrize("P", PC.WORDERS)
@pytest.mark.parametrize("res", PC.TINY_MESHES)
def test_meshes_smaller_than_the_window(res, P):
    """res < worder: several nodes of one particle are one cell.  The LDS image keeps them apart and the flush wraps them
    together; on the (1, 1, 1) mesh every weight of every particle lands in the one cell."""
    case = PC.tiny_mesh(res)
    a = three_kernels(case, P)
    if res == (1, 1, 1):
        assert a.shape == (1, 1, 1) and abs(float(a[0, 0, 0])) <= 2.0 ** -52       # the one rounding of n_cells / (N 2^22)
    assert np.array_equal(bits(with_quantity(case, P)), bits(a))


@pytest.mark.parametrize("P", PC.WORDERS)
def test_positions_just_inside_the_limit_are_painted(P):
    """|u| = 2^30 - 64 cells on each axis in turn, both signs: painted by all three kernels (float32 and float64 rows), on the
    direct path, since the footprint is 2^30 nodes long."""
    for axis, sign in PC.RANGE:
        case = PC.in_range(axis, sign, False)
        three_kernels(case, P, (np.float32, np.float64))
        assert plain(case, P)[1] == [1, 0] and field(case, P)[2] == [1, 0, 0]


# ---- 2. rejection ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PC.WORDERS)
def test_positions_at_the_limit_are_rejected_and_counted(P):
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    from jax_nbody_emulator_with_dj_amd.density import paint_density, paint_field, paint_particles
    for axis, sign in PC.RANGE:
        case = PC.in_range(axis, sign, True)
        kw = dict(boxsize=case.boxsize, res=case.res, worder=P)
        assert plain(case, P)[1][1] == 1 and field(case, P)[2][1] == 1
        with pytest.raises(NBEError, match=r"paint_density: 1 particle\(s\)"):
            paint_density(case.disp, deconvolve=False, **kw)
        with pytest.raises(NBEError, match=r"paint_field: 1 particle\(s\)"):
            paint_field(case.disp, quantity(case), **kw)
        for dt in (np.float32, np.float64):
            for sort in (False, True):
                with pytest.raises(NBEError, match=r"paint_particles: 1 particle\(s\)"):
                    paint_particles(PC.rows_of(case).astype(dt), deconvolve=False, sort=sort, **kw)
        # the call after a rejection paints the accepted limit
        good = PC.in_range(axis, sign, False)
        check_paint(good.disp, good.boxsize, good.res, P)
    bad = np.zeros((3, 2, 2, 2), np.float32)
    bad[1, 0, 1, 0], bad[2, 1, 1, 1], bad[0, 1, 0, 0] = np.nan, np.inf, -np.inf
    with pytest.raises(NBEError, match=r"paint_density: 3 particle\(s\)"):
        paint_density(bad, 4.0, 4, P, deconvolve=False)
    good = PC.in_range(0, 1, False)
    check_paint(good.disp, good.boxsize, good.res, P)


# ---- 3. ragged lattices on the plain painter ------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PC.WORDERS)
@pytest.mark.parametrize("n", sorted(PC.RAGGED))
def test_plain_painter_on_ragged_lattices(n, P):
    for scale in PC.RAGGED[n]:
        case = PC.ragged(n, scale)
        a, st = plain(case, P)
        check_paint(case.disp, case.boxsize, case.res, P, gpu=a)
        assert st == [PC.direct_tiles(PC.lattice_u(case), n, P, PC.LDS_CELLS), 0]
        _, b, sb = field(case, P)
        assert np.array_equal(bits(b), bits(a)) and sb[:2] == [PC.direct_tiles(PC.lattice_u(case), n, P, PC.FIELD_CELLS), 0]


# ---- 4. ties ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PC.WORDERS)
def test_exact_ties(P):
    """Particles on nodes, half-way between them, at -0.0, at negative u next to 0 and on the far face, in every
    combination.  The reference is exact, so check_paint's bound is a statement in units of 2^-22; for NGP, CIC and TSC
    every weight is a multiple of 2^-9, the running sums are exact and the integer mesh is the reference itself."""
    case, cat = PC.ties(), PC.tie_rows()
    a = three_kernels(case, P, (np.float32, np.float64))
    _, ref, cnt, _ = PR.paint(cat.pos, cat.boxsize, cat.res, P)
    for dt in (np.float32, np.float64):
        d, st = rows(cat.pos.astype(dt), cat.boxsize, cat.res, P)                    # -0.0 among the rows
        assert st[1] == 0
        check_delta(d, ref, cnt, len(cat.pos))
        assert np.array_equal(bits(d), bits(a))
    mesh, _ = raw_rows(cat.pos, cat.boxsize, cat.res, P)
    assert int(mesh.sum()) == len(cat.pos) << 22
    if P < 4:
        assert np.array_equal(mesh.astype(np.float64) * UNIT, ref)
    else:
        assert (np.abs(mesh.astype(np.float64) * UNIT - ref) <= UNIT * cnt).all()    # the scheme's own bound: one unit a weight


# ---- 5. exact path counts on a realistic field --------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _smooth():
    return smooth_field((16, 16, 16), 1000.0, 3.0, seed=77, slab=True)


@pytest.mark.parametrize("P", PC.WORDERS)
@pytest.mark.parametrize("res", [8, 16, 20, 24, 32])
def test_path_counts_are_exact_on_a_smooth_field(res, P):
    """8 tiles, 8 chunks: stats[0] is the number paint_cases predicts for each of the three kernels, for the rows as they
    come and in an explicit order, and the meshes are the same bits whichever path a tile took.  (At res 8, 16 and 32 the
    tiles of paint_kernel all take one path; at 20 and 24 they split 0 / 2 / 4 / 4 and 4 / 4 / 5 / 7 of 8 for P = 1 .. 4.
    Those of paint_field_kernel split at 16 and 20.)"""
    disp, L, n = _smooth(), (1000.0,) * 3, (16, 16, 16)
    case = PC.Lattice("smooth", disp, L, (res,) * 3, 0, "")
    u = PC.lattice_u(case)
    a, sa = plain(case, P)
    _, b, sb = field(case, P)
    want = [PC.direct_tiles(u, n, P, PC.LDS_CELLS), PC.direct_tiles(u, n, P, PC.FIELD_CELLS)]
    pos = PC.rows_of(case)
    uc = PR.mesh_coordinates(pos, L, case.res)
    perm = np.random.default_rng(res + P).permutation(len(pos))
    m0, s0 = raw_rows(pos, L, case.res, P)
    m1, s1 = raw_rows(pos, L, case.res, P, order=perm)
    _, s2 = rows(pos, L, case.res, P)
    print("res %d P%d: direct %d of 8 tiles (plain), %d (field); %d of 8 chunks in lattice order, %d shuffled"
          % (res, P, sa[0], sb[0], s0[0], s1[0]))
    assert [sa[0], sb[0]] == want and sa[1] == sb[1] == 0
    assert s0 == s2 == [PC.direct_chunks(uc, P), 0]
    assert s1 == [PC.direct_chunks(uc, P, order=perm), 0]
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(m0, m1) and int(m0.sum()) == len(pos) << 22
    check_paint(disp, L, case.res, P, gpu=a)


# ---- 6. keys ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shifted", [False, True])
@pytest.mark.parametrize("dtype", [np.float32, np.float64])
def test_particle_keys_word_for_word(dtype, shifted):
    """nbe_particle_keys against paint_cases.keys for tiles of 4, 8 and 16 cells (16 divides no axis of the mesh), row-major
    and Morton; painting in the order of any of those keys gives the bits of painting the rows as they come."""
    from jax_nbody_emulator_with_dj_amd.density import paint_particles
    case = PC.key_catalogue(dtype, shifted)
    u = PC.catalogue_u(case)
    count = len(case.pos)
    m0 = {P: raw_rows(case.pos, case.boxsize, case.res, P, shift=case.shift) for P in PC.WORDERS}
    for P, (mesh, st) in m0.items():
        assert st == [PC.direct_chunks(u, P), case.rejected] and int(mesh.sum()) == (count - case.rejected) << 22
    for edge in PC.KEY_EDGES:
        for morton in (False, True):
            k = device_keys(case, edge, morton)
            want = PC.keys(u, case.res, edge, morton)
            assert k.dtype == np.int64 and np.array_equal(k, want), (edge, morton, np.flatnonzero(k != want)[:5])
            order = np.argsort(k, kind="stable")
            for P in (PC.WORDERS if (edge, morton) == (8, False) else (2,)):
                mesh, st = raw_rows(case.pos, case.boxsize, case.res, P, order=order, shift=case.shift)
                assert st == [PC.direct_chunks(u, P, order=order), case.rejected]
                assert np.array_equal(mesh, m0[P][0])
    # the public call on the rows that are painted, against the reference
    pos, shift = PC.painted_rows(case)
    kw = {} if shift is None else dict(velocity=shift[1], los=shift[0], velocity_to_length=shift[2])
    for P in PC.WORDERS:
        _, ref, cnt, _ = PR.paint(pos, case.boxsize, case.res, P, shift=shift)
        d = [paint_particles(pos.astype(dtype), case.boxsize, case.res, P, deconvolve=False, sort=s, **kw) for s in (False, True)]
        check_delta(d[0], ref, cnt, len(pos))
        assert np.array_equal(bits(d[0]), bits(d[1]))
        assert (np.abs(m0[P][0].astype(np.float64) * UNIT - ref) <= 4 * UNIT * cnt + 1e-12).all()     # the rejected rows add nothing


# ---- 7. float16 -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("P", PC.WORDERS)
def test_float16_displacement_is_its_float32_widening(P):
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    cases = [PC.tiny_mesh(res) for res in PC.TINY_MESHES]
    cases += [PC.threshold(kind, P) for kind in sorted(PC.THRESHOLD) if P in PC.THRESHOLD[kind][2]]
    for case in cases:
        half = case.disp.astype(np.float16)
        wide = half.astype(np.float32)
        dh, sh = plain(case, P, half)
        dw, sw = plain(case, P, wide)
        assert np.array_equal(bits(dh), bits(dw)) and sh == sw
        assert sh == [PC.direct_tiles(R.positions(wide, case.boxsize, case.res), wide.shape[1:], P, PC.LDS_CELLS), 0]
        check_paint(wide, case.boxsize, case.res, P, gpu=dh)
        assert np.array_equal(bits(paint_density(half, case.boxsize, case.res, P, deconvolve=False)), bits(dh))
