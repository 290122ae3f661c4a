"""Per-particle fields on the MI355X (density.paint_field, the line-of-sight shift of paint_density) against the NumPy
float64 reference (field_ref.py): both normalisations for NGP/CIC/TSC/PCS at res = N/2, N, 2N on cubic, non-cubic and
ragged lattices, exact integer quantities, collapsed regions up to the overflow limit, the direct path, bits that do not
depend on the path, the call or the other channels, residency and dtype, the density of the same pass, the shift along a
line of sight, the undisplaced lattice and process_box's own output."""

import functools

import numpy as np
import pytest

import field_ref as F
import mas_ref as R
from test_gpu_density import check_paint, smooth_field

pytestmark = pytest.mark.gpu

SCALES = np.array([1.0, 300.0, 1e-3])
LATTICES = {"cubic": ((24, 24, 24), 1000.0), "noncubic": ((16, 24, 40), (300.0, 400.0, 500.0)),
            "ragged": ((20, 20, 20), 1000.0)}


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


def quantity(shape, seed, scales=SCALES):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((len(scales),) + tuple(shape)) * scales[:, None, None, None]).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _inputs(lattice, worder):
    shape, L = LATTICES[lattice]
    return smooth_field(shape, L, 3.0, seed=10 + worder), quantity(shape, 50 + worder)


def _device_call(disp, q, L, res, worder, normalize="density", fill=0.0, vel=None, los=2, f=0.0, want_delta=False):
    """density._paint_fields on cuda tensors of NumPy inputs: (field, delta, stats list)."""
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd import density as D
    n = tuple(q.shape[-3:])
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    L3, r3 = D._triple(L, "boxsize", "a length"), D._triple(res, "res", "an int")
    field, delta, stats = D._paint_fields(t(disp), t(q if q.ndim == 4 else q[None]), t(vel), los, f, n, L3, r3, worder,
                                          normalize, fill, want_delta)
    return field.cpu().numpy(), None if delta is None else delta.cpu().numpy(), stats.cpu().tolist()


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [0.5, 1, 2])
@pytest.mark.parametrize("lattice", sorted(LATTICES))
def test_both_normalisations_vs_reference(lattice, scale, worder):
    """Momentum mode within 4 2^-22 A count + m 2^(e - 24) + 2e-7 |ref| in every cell; density mode cross-multiplied, so
    that no cell is left out; cells no particle touches hold `fill` exactly.  Three channels of scale 1, 300 and 1e-3."""
    from jax_nbody_emulator_with_dj_amd.density import paint_field
    shape, L = LATTICES[lattice]
    disp, q = _inputs(lattice, worder)
    res = tuple(int(n * scale) for n in shape)
    ref = F.paint(disp, q, L, res, worder)
    mean = paint_field(disp, q, L, res, worder, normalize="mean")
    assert isinstance(mean, np.ndarray) and mean.shape == (3,) + res
    worst = F.check_mean(mean, q, ref, int(np.prod(shape)))
    print("worst error / bound, momentum mode: %.3f" % worst)
    dens = paint_field(disp, q, L, res, worder, normalize="density", fill=0.0)
    F.check_density(dens, q, ref)
    filled = paint_field(disp, q, L, res, worder, fill=-7.5)
    empty = ref[2] == 0
    assert (filled[:, empty] == np.float32(-7.5)).all()
    assert np.array_equal(filled[:, ref[1] > 1e-3], dens[:, ref[1] > 1e-3])


def test_integer_quantities_are_exact():
    """NGP, res = N, integers below 2^24: every sum is an integer that float64 holds, and the field is that number rounded
    once to float32, bit for bit (ragged 20^3 lattice: tiles of 8 do not divide it)."""
    from jax_nbody_emulator_with_dj_amd.density import paint_field
    n = (20, 20, 20)
    disp = smooth_field(n, 1000.0, 3.0, seed=3)
    rng = np.random.default_rng(4)
    q = np.stack([rng.integers(-2 ** 24 + 1, 2 ** 24, n), rng.integers(-1000, 1000, n),
                  rng.integers(0, 2, n) * (2 ** 24 - 1)]).astype(np.float32)
    num, mass, count, _ = F.paint(disp, q, 1000.0, 20, 1)
    assert count.max() >= 4 and float(np.abs(num).max()) > 2.0 ** 25
    got = paint_field(disp, q, 1000.0, 20, 1, normalize="mean")
    want = (num * (mass.size / float(np.prod(n)))).astype(np.float32)
    assert np.array_equal(got.view(np.int32), want.view(np.int32))
    dens = paint_field(disp, q, 1000.0, 20, 1, normalize="density", fill=0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        want = np.where(mass == 0, 0.0, num / mass).astype(np.float32)
    assert np.array_equal(dens.view(np.int32), want.view(np.int32))


def _collapsed(n, L, target):
    q = [np.arange(k, dtype=np.float64) * (L / k) for k in n]
    grid = np.meshgrid(*q, indexing="ij")
    return np.stack([target[c] - grid[c] for c in range(3)]).astype(np.float32)


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("where", ["inside", "corner"])
def test_collapsed_region(worder, where):
    """32^3 particles in one point (inside a cell; at a box corner, so that the window wraps on all three axes) carrying
    +A, alternating +-A and a ramp, A = 2^9 - 2^-15 (V = 2^24 - 1): a mesh cell sums up to 2^61 and an LDS cell 2^55, which
    a 32-bit image cannot hold.  Every tile goes through LDS and nothing is rejected."""
    n, L, res = (32, 32, 32), 100.0, 32
    target = (37.3, 51.0, 12.9) if where == "inside" else (L - 1e-3 * L / res, 0.2 * L / res, L - 0.45 * L / res)
    disp = _collapsed(n, L, target)
    A = np.float32(2.0 ** 9 - 2.0 ** -15)
    i = np.indices(n).sum(axis=0)
    ramp = (np.arange(32 ** 3, dtype=np.float64).reshape(n) / 32 ** 3 * 2.0 - 1.0) * float(A)
    q = np.stack([np.full(n, A), np.where(i % 2 == 0, A, -A), ramp]).astype(np.float32)
    ref = F.paint(disp, q, L, res, worder)
    mean, delta, stats = _device_call(disp, q, L, res, worder, "mean", want_delta=True)
    assert stats[:3] == [0, 0, 0]
    if worder == 1:
        assert float(np.abs(ref[0][0]).max()) * 2.0 ** (22 + 24 - 9) > 2.0 ** 60.9
    F.check_mean(mean, q, ref, 32 ** 3)
    dens, _, stats = _device_call(disp, q, L, res, worder, "density")
    assert stats[:3] == [0, 0, 0]
    F.check_density(dens, q, ref)
    check_paint(disp, L, res, worder, gpu=delta)


def test_overflow_guard():
    """2^17 particle masses in one cell (a (64, 64, 32) lattice collapsed, NGP) reach M = 2^39 units, where |S| <= M 2^24
    no longer fits 63 bits: NBEError.  The integers wrap; nothing is read or written out of bounds.  (64, 64, 31) stays
    below the limit and matches the reference."""
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    from jax_nbody_emulator_with_dj_amd.density import paint_field
    L, res, target = 100.0, 32, (37.3, 51.0, 12.9)
    A = np.float32(2.0 ** 9 - 2.0 ** -15)
    with pytest.raises(NBEError, match=r"2\^17 particle masses"):
        paint_field(_collapsed((64, 64, 32), L, target), np.full((64, 64, 32), A, np.float32), L, res, 1)
    n = (64, 64, 31)
    disp = _collapsed(n, L, target)
    q = np.stack([np.full(n, A), -np.full(n, A)]).astype(np.float32)
    ref = F.paint(disp, q, L, res, 1)
    assert ref[1].max() == 64 * 64 * 31
    F.check_mean(paint_field(disp, q, L, res, 1, normalize="mean"), q, ref, 64 * 64 * 31)
    F.check_density(paint_field(disp, q, L, res, 1), q, ref)


def test_direct_path():
    """PCS at res = 2N with the slab shift: tiles whose footprint exceeds the LDS image add straight into the meshes."""
    disp, q = _inputs("cubic", 4)
    ref = F.paint(disp, q, 1000.0, 48, 4)
    mean, _, stats = _device_call(disp, q, 1000.0, 48, 4, "mean")
    assert stats[0] > 0 and stats[1:3] == [0, 0]
    F.check_mean(mean, q, ref, 24 ** 3)
    dens, _, stats = _device_call(disp, q, 1000.0, 48, 4, "density")
    assert stats[0] > 0
    F.check_density(dens, q, ref)


def test_bits_do_not_depend_on_the_path():
    """16^3 particles at res = 16 in a box of 16 (mesh spacing 1, so positions i + psi are exact in float64), PCS.  First a
    small displacement on a grid of 2^-10: all 8 tiles fit the LDS image.  Then one particle of every tile is moved by a
    whole number of boxes (3 + tile), which float32 and float64 hold exactly: the weights are the same bits, every tile's
    footprint is beyond the image, and all 8 take the direct path."""
    n, L = (16, 16, 16), 16.0
    rng = np.random.default_rng(8)
    disp = (np.rint(smooth_field(n, L, 0.3, seed=9, slab=False) * 1024.0) / 1024.0).astype(np.float32)
    assert float(np.abs(disp).max()) < 4.0
    q = quantity(n, 11)
    vel = (np.rint(rng.standard_normal(n) * 256.0) / 256.0).astype(np.float32)
    moved = disp.copy()
    for t, (t0, t1, t2) in enumerate(np.ndindex(2, 2, 2)):
        p = (8 * t0 + int(rng.integers(8)), 8 * t1 + int(rng.integers(8)), 8 * t2 + int(rng.integers(8)))
        moved[(t % 3,) + p] += np.float32((3 + t) * L)
        assert float(moved[(t % 3,) + p]) - float(disp[(t % 3,) + p]) == (3 + t) * L
    for normalize in ("mean", "density"):
        a = _device_call(disp, q, L, 16, 4, normalize, vel=vel, los=1, f=0.125, want_delta=True)
        b = _device_call(moved, q, L, 16, 4, normalize, vel=vel, los=1, f=0.125, want_delta=True)
        assert a[2][:3] == [0, 0, 0] and b[2][:3] == [8, 0, 0]
        assert np.array_equal(a[0].view(np.int32), b[0].view(np.int32))
        assert np.array_equal(a[1].view(np.int32), b[1].view(np.int32))


@pytest.mark.parametrize("worder", [2, 4])
def test_repeatable_and_channels_are_independent(worder):
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_field
    n = (64, 64, 64)
    x = torch.from_numpy(smooth_field(n, 1000.0, 2.0, seed=5)).cuda()
    q = torch.from_numpy(quantity(n, 6)).cuda()
    for normalize in ("mean", "density"):
        a = paint_field(x, q, 1000.0, 64, worder, normalize=normalize)
        b = paint_field(x, q, 1000.0, 64, worder, normalize=normalize)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32))
        one = paint_field(x, q[1], 1000.0, 64, worder, normalize=normalize)
        assert one.shape == (64, 64, 64) and torch.equal(one.view(torch.int32), a[1].view(torch.int32))
        four = paint_field(x, torch.stack([q[2], q[1], q[0], q[1]]), 1000.0, 64, worder, normalize=normalize)
        assert torch.equal(four[1].view(torch.int32), a[1].view(torch.int32))
        assert torch.equal(four[0].view(torch.int32), a[2].view(torch.int32))


def test_residency_and_float16():
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_density, paint_field
    n = (32, 32, 32)
    disp, q = smooth_field(n, 100.0, 2.0, seed=7), quantity(n, 8)
    dev = torch.device("cuda", torch.cuda.device_count() - 1)
    x, qt = torch.from_numpy(disp).to(dev), torch.from_numpy(q).to(dev)
    f = paint_field(x, qt, 100.0, 32, 3)
    assert isinstance(f, torch.Tensor) and f.device == dev and f.dtype == torch.float32 and f.shape == (3, 32, 32, 32)
    qh, vh = qt.half(), qt[:1].expand(3, -1, -1, -1).half()
    fh, dh = paint_field(x, qh, 100.0, 32, 3, return_delta=True, velocity=vh, los=0, velocity_to_length=0.25)
    fw, dw = paint_field(x, qh.float(), 100.0, 32, 3, return_delta=True, velocity=vh.float(), los=0,
                         velocity_to_length=0.25)
    assert fh.device == dev and dh.device == dev
    assert torch.equal(fh.view(torch.int32), fw.view(torch.int32)) and torch.equal(dh, dw)
    sh = paint_density(x, 100.0, 32, 3, deconvolve=False, velocity=vh[0], los=0, velocity_to_length=0.25)
    assert sh.device == dev and torch.equal(sh, dw)
    fn = paint_field(disp, q.astype(np.float16), 100.0, 32, 3, velocity=vh[0].cpu().numpy(), los=0,
                     velocity_to_length=0.25)
    assert isinstance(fn, np.ndarray) and fn.dtype == np.float32 and np.array_equal(fn, fw.cpu().numpy())
    # deconvolution divides every channel by the window
    fd = paint_field(x, qt[:2], 100.0, 32, 3, deconvolve=True)
    raw = paint_field(x, qt[:2], 100.0, 32, 3)
    for c in range(2):
        want = R.deconvolve(raw[c].cpu().numpy(), 3)
        assert np.linalg.norm(fd[c].cpu().numpy() - want) <= 1e-5 * np.linalg.norm(want)


def test_non_finite_quantity_raises():
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    from jax_nbody_emulator_with_dj_amd.density import paint_field
    disp = np.zeros((3, 8, 8, 8), np.float32)
    q = np.ones((2, 8, 8, 8), np.float32)
    q[1, 2, 3, 4] = np.inf
    q[0, 0, 0, 0] = np.nan
    with pytest.raises(NBEError, match="2 value"):
        paint_field(disp, q, 100.0, 8)
    bad = disp.copy()
    bad[1, 1, 1, 1] = np.nan
    with pytest.raises(NBEError, match="1 particle"):
        paint_field(bad, np.ones((8, 8, 8), np.float32), 100.0, 8)
    v = np.zeros((8, 8, 8), np.float32)
    v[5, 5, 5] = np.inf
    with pytest.raises(NBEError, match="1 particle"):
        paint_field(disp, np.ones((8, 8, 8), np.float32), 100.0, 8, velocity=v, velocity_to_length=1.0)
    zero = paint_field(disp, np.zeros((8, 8, 8), np.float32), 100.0, 8, fill=2.5)       # A = 0: a zero channel
    assert (zero == 0).all()


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
def test_return_delta_is_paint_density(worder):
    from jax_nbody_emulator_with_dj_amd.density import paint_density, paint_field
    disp, q = _inputs("ragged", worder)
    v = quantity((20, 20, 20), 70, np.array([200.0]))[0]
    for res in (20, (16, 24, 40)):
        _, delta = paint_field(disp, q, 1000.0, res, worder, return_delta=True)
        assert np.array_equal(delta.view(np.int32), paint_density(disp, 1000.0, res, worder, deconvolve=False).view(np.int32))
        _, delta = paint_field(disp, q, 1000.0, res, worder, return_delta=True, velocity=v, los=1, velocity_to_length=0.01)
        want = paint_density(disp, 1000.0, res, worder, deconvolve=False, velocity=v, los=1, velocity_to_length=0.01)
        assert np.array_equal(delta.view(np.int32), want.view(np.int32))


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("los", [0, 1, 2])
def test_line_of_sight_shift(worder, los):
    """paint_density with a velocity against mas_ref.paint of the float64 displacement disp + f v on axis los, through the
    bound of test_gpu_density.check_paint; the full (3, ...) velocity and its component give the same bits."""
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    n, L, f = (24, 24, 24), 1000.0, 0.0123
    disp = smooth_field(n, L, 3.0, seed=10 + worder)
    v = quantity(n, 80 + los, np.array([300.0, 300.0, 300.0]))
    got = paint_density(disp, L, 24, worder, deconvolve=False, velocity=v, los=los, velocity_to_length=f)
    moved = disp.astype(np.float64)
    moved[los] += f * v[los].astype(np.float64)
    check_paint(moved, L, 24, worder, gpu=got)
    one = paint_density(disp, L, 24, worder, deconvolve=False, velocity=v[los], los=los, velocity_to_length=f)
    assert np.array_equal(got.view(np.int32), one.view(np.int32))


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
def test_shift_by_one_box_length_changes_nothing(worder):
    """L = 96, res = N = 24: the mesh spacing is 4, so i + psi / 4 and the shift of exactly 24 cells are exact in float64
    and the weights are the same bits as those of the unshifted call (which takes paint_density's own kernel)."""
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    n, L = (24, 24, 24), 96.0
    disp = smooth_field(n, L, 3.0, seed=33)
    plain = paint_density(disp, L, 24, worder, deconvolve=False)
    for los in (0, 1, 2):
        got = paint_density(disp, L, 24, worder, deconvolve=False, velocity=np.full(n, 48.0, np.float32), los=los,
                            velocity_to_length=-2.0)
        assert np.array_equal(got.view(np.int32), plain.view(np.int32))


def test_undisplaced_lattice():
    """displacement=None is the reference's project_field_from_particles: a 32^3 field onto 16^3 with CIC; NGP at res = N
    returns the input, every value rounded at 2^(e - 25)."""
    from jax_nbody_emulator_with_dj_amd.density import paint_field
    n = (32, 32, 32)
    q = quantity(n, 90, np.array([1.7]))[0]
    ref = F.paint(None, q, 1000.0, 16, 2)
    got = paint_field(None, q, 1000.0, 16, 2)
    assert got.shape == (16, 16, 16)
    F.check_density(got, q, ref)
    np.testing.assert_allclose(ref[1], 8.0, rtol=0, atol=1e-12)
    F.check_mean(paint_field(None, q, 1000.0, 16, 2, normalize="mean"), q, ref, 32 ** 3)
    same = paint_field(None, q, 1000.0, 32, 1)
    A, e = F.exponents(q)
    assert (np.abs(same.astype(np.float64) - q) <= 2.0 ** (e[0] - 25)).all()
    top = np.abs(q) >= 2.0 ** (e[0] - 1)
    assert top.any() and np.array_equal(same[top], q[top])
    import torch
    t = paint_field(None, torch.from_numpy(q).cuda(), 1000.0, 16, 2)
    assert t.is_cuda and np.array_equal(t.cpu().numpy(), got)


def test_process_box_velocity_paints_without_host_copy():
    torch = _torch()
    import jax_nbody_emulator_with_dj_amd as J
    from jax_nbody_emulator_with_dj_amd.density import paint_density, paint_field, rsd_factor
    from oracle import params as P
    p = P.synthetic_params(seed=61, mid_chan=8)
    cfg = J.SubboxConfig(size=(16, 16, 16), ndiv=(1, 1, 1))
    emu = J.create_emulator(load_params=False, processor_config=cfg, mid_chan=8, compute_vel=True)
    emu.processor.params = p
    box = torch.from_numpy(np.random.default_rng(62).standard_normal((3, 16, 16, 16)).astype(np.float32) * 5).cuda()
    disp, vel = emu.process_box(box, z=0.5, Om=0.3, show_progress=False)
    assert isinstance(vel, torch.Tensor) and vel.is_cuda and vel.shape == (3, 16, 16, 16)
    f, delta = paint_field(disp, vel, 200.0, 16, 2, return_delta=True)
    assert f.is_cuda and f.shape == (3, 16, 16, 16) and delta.is_cuda
    d, v = disp.cpu().numpy(), vel.cpu().numpy()
    F.check_density(f.cpu().numpy(), v, F.paint(d, v, 200.0, 16, 2))
    check_paint(d, 200.0, 16, 2, gpu=delta.cpu().numpy())
    s = paint_density(disp, 200.0, 16, 2, deconvolve=False, velocity=vel, los=2, velocity_to_length=rsd_factor(0.5, 0.3))
    moved = d.astype(np.float64)
    moved[2] += rsd_factor(0.5, 0.3) * v[2].astype(np.float64)
    check_paint(moved, 200.0, 16, 2, gpu=s.cpu().numpy())
