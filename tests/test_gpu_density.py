"""Density fields on the MI355X (jax_nbody_emulator_with_dj_amd.density) against the NumPy float64 reference (mas_ref.py):
painting for NGP/CIC/TSC/PCS at res = N/2, N, 2N, collapsed regions, reproducibility, residency and dtype, the window
deconvolution and power spectra."""

import numpy as np
import pytest

import mas_ref as R
from test_density_host import plane_wave, two_particle_cic_case

pytestmark = pytest.mark.gpu

UNIT = 2.0 ** -22


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


def smooth_field(shape, boxsize, rms_cells, seed, slab=True):
    """(3, N0, N1, N2) float32: a smoothed random displacement with an rms of `rms_cells` lattice cells per axis, a little
    white noise, and (slab) a slab of planes moved by +-0.3 L across the periodic boundary."""
    rng = np.random.default_rng(seed)
    L = np.broadcast_to(np.asarray(boxsize, np.float64), (3,))
    out = np.empty((3,) + tuple(shape), np.float32)
    for c in range(3):
        f = np.fft.rfftn(rng.standard_normal(shape))
        k2 = sum(np.meshgrid(*[np.fft.fftfreq(n) ** 2 for n in shape[:2]], np.fft.rfftfreq(shape[2]) ** 2,
                             indexing="ij"))
        g = np.fft.irfftn(f * np.exp(-k2 * (2 * np.pi * 3.0) ** 2 / 2), s=shape, axes=(0, 1, 2))
        cell = L[c] / shape[c]
        g = g / g.std() * rms_cells * cell + 0.2 * cell * rng.standard_normal(shape)
        out[c] = g
    if slab:
        n0 = shape[0]
        out[0, n0 // 4: n0 // 4 + 3] += 0.3 * L[0]
        out[1, n0 // 2: n0 // 2 + 2] -= 0.3 * L[1]
    return out


def check_paint(disp, boxsize, res, worder, gpu=None):
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    if gpu is None:
        gpu = paint_density(disp, boxsize, res, worder, deconvolve=False)
    n = int(np.prod(disp.shape[1:]))
    ref, count = R.paint(disp, boxsize, res, worder)
    assert gpu.dtype == np.float32 and gpu.shape == ref.shape
    m = (gpu.astype(np.float64) + 1.0) * (n / gpu.size)
    err = np.abs(m - ref)
    bound = 4 * UNIT * count + 2e-7 * ref
    assert (err <= bound + 1e-12).all(), (err.max(), np.argmax(err - bound))
    assert m.sum() == pytest.approx(n, rel=1e-6)
    return gpu


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [0.5, 1, 2])
def test_paint_cubic_vs_reference(worder, scale):
    disp = smooth_field((64, 64, 64), 1000.0, 3.0, seed=10 + worder)
    check_paint(disp, 1000.0, int(64 * scale), worder)


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [0.5, 1, 2])
def test_paint_noncubic_vs_reference(worder, scale):
    shape, L = (48, 64, 80), (300.0, 400.0, 500.0)
    disp = smooth_field(shape, L, 2.5, seed=20 + worder)
    check_paint(disp, L, tuple(int(n * scale) for n in shape), worder)


def test_two_particle_cic_by_hand_on_gpu():
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    disp, m = two_particle_cic_case()
    gpu = paint_density(disp, 4.0, 4, 2, deconvolve=False)
    np.testing.assert_allclose((gpu.astype(np.float64) + 1.0) * (2.0 / 64.0), m, rtol=0, atol=2 * UNIT)


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("res", [8, 32, 96])
def test_collapsed_region_is_exact(worder, res):
    """Every particle of a 32^3 lattice in one point: inside a cell, and at a box corner so that the window wraps on all
    three axes.  Every tile lands in the same few cells (a 32-bit LDS cell holds a whole tile's 2^31 units)."""
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd import density as D
    n, L = 32, 100.0
    q = np.indices((n, n, n)).astype(np.float64) * (L / n)
    for target in ((37.3, 51.0, 12.9), (L - 1e-3 * L / res, 0.2 * L / res, L - 0.45 * L / res)):
        disp = np.stack([target[c] - q[c] for c in range(3)]).astype(np.float32)
        gpu = check_paint(disp, L, res, worder)
        x = torch.from_numpy(disp).cuda()
        delta, stats = D._paint(x, (L,) * 3, (res,) * 3, worder, False)
        assert stats.cpu().tolist()[:2] == [0, 0]                 # every tile painted through LDS, nothing rejected
        assert np.array_equal(delta.cpu().numpy(), gpu)


@pytest.mark.parametrize("worder", [2, 4])
def test_paint_is_bitwise_reproducible(worder):
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    x = torch.from_numpy(smooth_field((128, 128, 128), 1000.0, 0.8, seed=5)).cuda()
    a = paint_density(x, 1000.0, 128, worder, deconvolve=True)
    b = paint_density(x, 1000.0, 128, worder, deconvolve=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_residency_and_float16():
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    disp = smooth_field((32, 32, 32), 100.0, 2.0, seed=7)
    dev = torch.device("cuda", torch.cuda.device_count() - 1)
    x = torch.from_numpy(disp).to(dev)
    d = paint_density(x, 100.0, 32, 3)
    assert isinstance(d, torch.Tensor) and d.device == dev and d.dtype == torch.float32 and d.shape == (32, 32, 32)
    h = x.half()
    dh = paint_density(h, 100.0, 32, 3, deconvolve=False)
    dw = paint_density(h.float(), 100.0, 32, 3, deconvolve=False)
    assert dh.device == dev and torch.equal(dh, dw)
    dn = paint_density(disp.astype(np.float16), 100.0, 32, 3, deconvolve=False)
    assert isinstance(dn, np.ndarray) and np.array_equal(dn, dw.cpu().numpy())
    check_paint(disp.astype(np.float16).astype(np.float32), 100.0, 32, 3, gpu=dn)


def test_process_box_output_paints_without_host_copy():
    torch = _torch()
    import jax_nbody_emulator_with_dj_amd as J
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    from oracle import params as P
    p = P.synthetic_params(seed=61, mid_chan=8)
    cfg = J.SubboxConfig(size=(16, 16, 16), ndiv=(1, 1, 1))
    emu = J.create_emulator(load_params=False, processor_config=cfg, mid_chan=8, compute_vel=False)
    emu.processor.params = p
    box = torch.from_numpy(np.random.default_rng(62).standard_normal((3, 16, 16, 16)).astype(np.float32) * 5).cuda()
    disp = emu.process_box(box, z=0.5, Om=0.3, show_progress=False)
    assert isinstance(disp, torch.Tensor) and disp.is_cuda
    d = paint_density(disp, 200.0, 16, 2, deconvolve=False)
    assert d.is_cuda
    check_paint(disp.cpu().numpy(), 200.0, 16, 2, gpu=d.cpu().numpy())


def _rel_l2(a, b):
    return float(np.linalg.norm(np.asarray(a, np.float64) - b) / np.linalg.norm(b))


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
def test_deconvolution_vs_reference(worder):
    from jax_nbody_emulator_with_dj_amd.density import paint_density, deconvolve_mas
    shape, L = (48, 64, 80), (300.0, 400.0, 500.0)
    disp = smooth_field(shape, L, 2.0, seed=30 + worder)
    raw = paint_density(disp, L, (40, 64, 96), worder, deconvolve=False)
    ref = R.deconvolve(raw, worder)
    assert _rel_l2(paint_density(disp, L, (40, 64, 96), worder, deconvolve=True), ref) <= 1e-5
    assert _rel_l2(deconvolve_mas(raw, worder), ref) <= 1e-5


def test_power_spectrum_vs_reference():
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_density, power_spectrum
    L = 500.0
    fa, fc = smooth_field((64, 64, 64), L, 2.0, seed=41), smooth_field((64, 64, 64), L, 2.0, seed=42)
    a = paint_density(fa, L, 64, 2)
    b = paint_density((fa + 0.3 * fc).astype(np.float32), L, 64, 2)     # correlated, like emulated vs LPT fields
    c = paint_density(fc, L, 64, 2)                                      # independent of a
    pa = R.power(a, L)[1]
    for other in (None, b, c):
        k, pk, nm = power_spectrum(a, L, other=other)
        kr, pr, nr = R.power(a, L, other)
        assert k.dtype == pk.dtype == nm.dtype == np.float64 and k.shape == (32,)
        assert np.array_equal(nm, nr)
        np.testing.assert_allclose(k, kr, rtol=1e-10, atol=0)        # exact to the 2^-36 fixed point of the sums
        if other is c:
            # the mean of Re(a b*) of independent fields cancels to ~0: its float32-FFT error is relative to sqrt(Pa Pc)
            assert (np.abs(pk - pr) <= 1e-5 * np.sqrt(pa * R.power(c, L)[1])).all()
        else:
            np.testing.assert_allclose(pk, pr, rtol=1e-5, atol=0)
        # tensors in, same numbers, byte-identical on a second call
        kt, pt, nt = power_spectrum(torch.from_numpy(a).cuda(), L,
                                    other=None if other is None else torch.from_numpy(other).cuda())
        assert np.array_equal(kt, k) and np.array_equal(pt, pk) and np.array_equal(nt, nm)


def test_power_spectrum_of_a_plane_wave():
    from jax_nbody_emulator_with_dj_amd.density import power_spectrum
    n, L, A = 32, 100.0, 0.3
    k, pk, nm = power_spectrum(plane_wave(n, L, A).astype(np.float32), L)
    for s in (1, 3, 7, 16):
        assert nm[s - 1] == R.full_grid_modes(n, s)
    np.testing.assert_allclose(pk[2], A * A * L ** 3 / 2.0 / nm[2], rtol=1e-5)
    assert np.abs(np.delete(pk, 2)).max() < 1e-9 * pk[2]
