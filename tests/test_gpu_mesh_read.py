"""The mesh readout on the MI355X (density.read_mesh, halos.halo_environment and nbe_mesh_read behind them) against
tests/web_ref.py's readout from mas_ref's window weights.

Bound: |out - ref| <= (P^3 + 1) 2^-22 max|f_c|.  Each of the P^3 integer weights is within one unit of 2^-22 of the exact
product of the windows, and the float32 result is rounded once (at most 2^-24 max|f|, counted as one more unit).  What is
exact is held with ==: a constant field, the adjoint identity against nbe_paint_particles' integer mesh, the lattice form
against the catalogue form, and every permutation of the rows."""

import ctypes as C

import numpy as np
import pytest

import web_ref as W
from lpt_ref import red_field

pytestmark = pytest.mark.gpu

MESHES = [(1, 1, 1), (2, 3, 2), (6, 5, 7), (16, 16, 16)]
COUNTS = [1, 255, 256, 257, 513]
BOX = (100.0, 75.0, 125.0)


def _torch():
    import torch
    return torch


def _density():
    from jax_nbody_emulator_with_dj_amd import density
    return density


def _abi():
    from jax_nbody_emulator_with_dj_amd import _lib
    return _lib


def ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else None


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def mesh_units(x, res, box=BOX):
    return np.asarray(x, np.float64) * (np.asarray(res, np.float64) / np.asarray(box, np.float64))


def rows(count, seed, dtype):
    """Positions several boxes away on either side, negative ones included."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(-3.0, 4.0, (count, 3)) * np.asarray(BOX)).astype(dtype)


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("res", MESHES)
def test_read_mesh_vs_reference(res, worder):
    D = _density()
    rng = np.random.default_rng(sum(res) + worder)
    fields = rng.standard_normal((4,) + res).astype(np.float32)
    k = 0
    for count in COUNTS:
        for dtype in (np.float32, np.float64):
            nchan = 1 + k % 4
            k += 1
            x = rows(count, 100 * count + worder, dtype)
            f = fields[:nchan]
            out = D.read_mesh(f if nchan > 1 or k % 3 else f[0], BOX, positions=x, worder=worder)
            if out.ndim == 1:
                out = out[None]
            assert out.shape == (nchan, count) and out.dtype == np.float32
            ref = W.read_mesh(f, mesh_units(x, res), worder)
            bound = (worder ** 3 + 1) * 2.0 ** -22 * np.abs(f).reshape(nchan, -1).max(1)
            err = np.abs(out.astype(np.float64) - ref).max(1)
            assert (err <= bound).all(), (res, worder, count, dtype, (err / bound).max())


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
def test_constant_field_and_ngp_half_way_points(worder):
    torch = _torch()
    D = _density()
    for res in MESHES:
        const = np.full((2,) + res, np.float32(3.7), np.float32)
        const[1] = np.float32(-1.0e-3)
        out = D.read_mesh(const, BOX, positions=rows(300, 5, np.float64), worder=worder)
        assert np.all(out[0] == np.float32(3.7)) and np.all(out[1] == np.float32(-1.0e-3))
    if worder == 1:
        # u = j + 1/2 exactly: the node above, as the painter's floor(u + 1/2)
        f = np.arange(16, dtype=np.float32).reshape(16, 1, 1) * np.ones((16, 16, 16), np.float32)
        x = np.zeros((16, 3), np.float32)
        x[:, 0] = (np.arange(16) - 4 + 0.5) / 2.0
        out = D.read_mesh(torch.from_numpy(f).cuda(), 8.0, positions=torch.from_numpy(x).cuda(), worder=1)
        assert out.is_cuda and out.cpu().numpy().tolist() == [float((j - 4 + 1) % 16) for j in range(16)]


def paint_mass(x, res, worder):
    """nbe_paint_particles' int64 mass mesh of the rows x (float64), as Python-int friendly NumPy."""
    torch = _torch()
    l = _abi().lib()
    p = torch.from_numpy(x).cuda()
    mesh = torch.zeros(res, dtype=torch.int64, device="cuda")
    stats = torch.zeros(4, dtype=torch.int32, device="cuda")
    _abi().check(l.nbe_paint_particles(ptr(p), 2, None, None, 0, 0, (C.c_int * 4)(), None, 0, 0, 0.0, x.shape[0],
                                       (C.c_double * 3)(*BOX), (C.c_int64 * 3)(*res), worder, ptr(mesh), None, ptr(stats),
                                       None))
    assert stats.cpu().tolist()[1] == 0
    return mesh.cpu().numpy()


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
def test_exact_adjoint_of_the_painter(worder):
    """sum(M g) == sum(read(g) 2^22) in integers, for g in {-2 .. 2}: |sum of q g| <= 2^23 per row is a float32 integer."""
    D = _density()
    for res, count in (((6, 5, 7), 513), ((2, 3, 2), 257), ((16, 16, 16), 256)):
        x = rows(count, 900 + worder, np.float64)
        g = np.random.default_rng(worder).integers(-2, 3, res).astype(np.float32)
        M = paint_mass(x, res, worder)
        out = D.read_mesh(g, BOX, positions=x, worder=worder)
        scaled = out.astype(np.float64) * 2.0 ** 22
        assert np.all(scaled == np.rint(scaled))
        lhs = sum(int(m) * int(v) for m, v in zip(M.ravel().tolist(), g.ravel().tolist()))
        rhs = sum(int(v) for v in scaled.tolist())
        assert lhs == rhs and int(M.sum()) == count << 22


@pytest.mark.parametrize("N", [8, 12])
@pytest.mark.parametrize("dtype", [np.float32, np.float16])
def test_lattice_form_equals_the_catalogue_form(N, dtype):
    """L = 8 N and res = 2 N make res / L = 1/4 and res / N = 2 exact, and psi in multiples of 2^-6 makes every position
    exact in both forms: the same bits.  N = 12 leaves a ragged last workgroup."""
    D = _density()
    Lb, res = 8.0 * N, 2 * N
    rng = np.random.default_rng(N)
    psi = (rng.integers(-192, 193, (3, N, N, N)) / 64.0).astype(dtype)
    f = rng.standard_normal((3, res, res, res)).astype(np.float32)
    i = np.indices((N, N, N)).reshape(3, -1).T.astype(np.float64)
    x = i * (Lb / N) + psi.astype(np.float64).reshape(3, -1).T
    for worder in (1, 2, 3, 4):
        cat = D.read_mesh(f, Lb, positions=x, worder=worder)
        lat = D.read_mesh(f, Lb, displacement=psi, worder=worder)
        assert lat.shape == (3, N, N, N) and same_bits(lat.reshape(3, -1), cat)
        bare = D.read_mesh(f[0], Lb, lattice=N, worder=worder)
        assert bare.shape == (N, N, N) and same_bits(bare.reshape(-1), D.read_mesh(f[0], Lb, positions=i * (Lb / N), worder=worder))
    assert np.array_equal(D.read_mesh(f[0], Lb, lattice=(N, N, N), worder=1), f[0, ::2, ::2, ::2])


def test_rejected_rows_get_fill_and_are_counted():
    D = _density()
    res = (6, 5, 7)
    f = np.random.default_rng(1).standard_normal((2,) + res).astype(np.float32)
    x = rows(257, 4, np.float64)
    bad = [3, 100, 255, 256]
    x[3, 0] = np.nan
    x[100, 1] = np.inf
    x[255, 2] = -np.inf
    x[256, 0] = 1.0e12 * BOX[0]                            # beyond 2^30 mesh cells
    good = np.setdiff1d(np.arange(257), bad)
    ref = D.read_mesh(f, BOX, positions=x[good], worder=3)
    for dtype in (np.float64, np.float32):
        out, st = D.read_mesh(f, BOX, positions=x.astype(dtype), worder=3, fill=-7.5, return_stats=True)
        assert st == {"not_read": 4} and np.all(out[:, bad] == -7.5)
        if dtype == np.float64:
            assert same_bits(out[:, good], ref)
    out = D.read_mesh(f, BOX, positions=x, worder=2)
    assert np.isnan(out[:, bad]).all() and not np.isnan(out[:, good]).any()
    psi = np.zeros((3, 4, 4, 4), np.float32)
    psi[1, 2, 3, 1] = np.nan
    out, st = D.read_mesh(f, BOX, displacement=psi, fill=2.0, return_stats=True)
    assert st == {"not_read": 1} and np.all(out[:, 2, 3, 1] == 2.0)


def test_order_entries_out_of_range_write_nothing():
    torch = _torch()
    l = _abi().lib()
    res = (6, 5, 7)
    f = torch.from_numpy(np.random.default_rng(2).standard_normal((1,) + res).astype(np.float32)).cuda()
    x = torch.from_numpy(rows(4, 8, np.float64)).cuda()
    got = {}
    for name, order in (("identity", None), ("bad", [3, 7, 0, -1]), ("perm", [3, 1, 0, 2])):
        o = None if order is None else torch.tensor(order, dtype=torch.int64, device="cuda")
        out = torch.full((1, 4), 99.0, dtype=torch.float32, device="cuda")
        stats = torch.zeros(4, dtype=torch.int32, device="cuda")
        _abi().check(l.nbe_mesh_read(ptr(f), 1, (C.c_int64 * 3)(*res), None, 0, None, ptr(x), 2, ptr(o), 4,
                                     (C.c_double * 3)(*BOX), 2, 0.0, ptr(out), ptr(stats), None))
        got[name] = (out.cpu().numpy()[0], stats.cpu().tolist()[1])
    assert got["identity"][1] == 0 and got["perm"][1] == 0 and same_bits(got["perm"][0], got["identity"][0])
    assert got["bad"][1] == 2
    assert same_bits(got["bad"][0][[0, 3]], got["identity"][0][[0, 3]]) and got["bad"][0][[1, 2]].tolist() == [99.0, 99.0]


def test_every_order_and_sort_give_the_same_bits():
    """2^18 rows on 16^3 cells, where paint_particles' "auto" sorts (the readout's does not: it measured slower); a shuffled
    catalogue gives the permuted bits."""
    torch = _torch()
    D = _density()
    count, res = 1 << 18, (16, 16, 16)
    f = torch.from_numpy(np.random.default_rng(3).standard_normal((2,) + res).astype(np.float32)).cuda()
    x = torch.from_numpy(rows(count, 6, np.float32)).cuda()
    base = D.read_mesh(f, BOX, positions=x, worder=2, sort=False)
    for sort in (True, "auto"):
        assert torch.equal(D.read_mesh(f, BOX, positions=x, worder=2, sort=sort).view(torch.int32), base.view(torch.int32))
    perm = torch.randperm(count, device="cuda", generator=torch.Generator(device="cuda").manual_seed(1))
    shuffled = D.read_mesh(f, BOX, positions=x[perm].contiguous(), worder=2, sort=True)
    assert torch.equal(shuffled.view(torch.int32), base[:, perm].contiguous().view(torch.int32))
    small = x[:513].contiguous()
    assert torch.equal(D.read_mesh(f, BOX, positions=small, worder=4, sort=True).view(torch.int32),
                       D.read_mesh(f, BOX, positions=small, worder=4, sort=False).view(torch.int32))


def test_halo_environment_reads_the_voxel_of_the_centre():
    from jax_nbody_emulator_with_dj_amd import halos, lpt, web
    n, Lb, sm, th = 16, 200.0, 20.0, 0.05
    delta = red_field(n, 12, np.float32)
    rng = np.random.default_rng(5)
    cat = {"CMPosition": rng.uniform(-0.5 * Lb, 1.5 * Lb, (300, 3)), "Length": rng.integers(20, 500, 300).astype(np.int64)}
    env = halos.halo_environment(cat, delta, Lb, sm, threshold=th, worder=1, min_length=100)
    keep = cat["Length"] >= 100
    H = int(keep.sum())
    assert env["count"] == H and np.array_equal(env["Length"], cat["Length"][keep])
    assert env["eigenvalues"].shape == (H, 3) and env["delta_s"].shape == (H,) and env["web_type"].dtype == np.uint8
    full = web.cosmic_web(delta, Lb, sm, threshold=th)
    cell = np.mod(np.floor(cat["CMPosition"][keep] * (n / Lb) + 0.5).astype(np.int64), n)
    at = lambda m: m[..., cell[:, 0], cell[:, 1], cell[:, 2]]
    assert np.array_equal(env["web_type"], at(full["types"]))
    assert same_bits(env["eigenvalues"], np.ascontiguousarray(at(full["eigenvalues"]).T))
    assert same_bits(env["delta_s"], at(lpt.gaussian_smooth(delta, Lb, sm)))
    assert len(set(env["web_type"].tolist())) >= 3
    cic = halos.halo_environment(cat, delta, Lb, sm, threshold=th, worder=2)
    ref = W.read_mesh(full["eigenvalues"], cat["CMPosition"] * (n / Lb), 2)
    bound = 9 * 2.0 ** -22 * np.abs(full["eigenvalues"]).max()
    assert np.abs(cic["eigenvalues"].T.astype(np.float64) - ref).max() <= bound
