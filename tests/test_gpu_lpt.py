"""The emulator's input on the MI355X (jax_nbody_emulator_with_dj_amd.lpt) against the float64 restatement tests/lpt_ref.py.

Unless a test says otherwise the bound is a relative L2 error of 1e-5, the one test_deconvolution_vs_reference holds the
same rfftn - kernel - irfftn path to (float32 transforms reach 1e-7 to 2e-7 at these sizes)."""

import numpy as np
import pytest

import lpt_ref as R
from lpt_ref import power_law_table, red_field

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = 1000.0


def _torch():
    import torch
    return torch


def _lpt():
    from jax_nbody_emulator_with_dj_amd import lpt
    return lpt


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def within_ulps(got, ref, ulps=1):
    """Whether every float32 of `got` is within `ulps` float32 steps (at the reference's magnitude) of the float64 ref."""
    ref32 = np.asarray(ref, np.float64).astype(np.float32)
    err = np.abs(np.asarray(got, np.float64) - np.asarray(ref, np.float64))
    worst = float((err / np.spacing(np.maximum(np.abs(ref32), np.float32(1e-30))).astype(np.float64)).max())
    print("worst error: %.3f ulp" % worst)
    return worst <= ulps


# ---- Zel'dovich ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 15, 40])
def test_zeldovich_vs_reference(n):
    """Even, odd, and (40) more than one workgroup with a ragged tail: 1600 rows of 21 modes."""
    x = red_field(n, 200 + n, np.float32)
    psi = _lpt().zeldovich_displacement(x, boxsize=250.0, scale=0.8)
    assert isinstance(psi, np.ndarray) and psi.dtype == np.float32 and psi.shape == (3, n, n, n)
    err = rel_l2(psi, R.zeldovich_displacement(x, 250.0, 0.8))
    print("n %d: rel L2 %.3e" % (n, err))
    assert err <= TOL


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_zeldovich_plane_wave(axis):
    n, A, j, box = 16, 0.3, 2, 100.0
    phase = 2.0 * np.pi * j * np.arange(n) / n
    shape = [1, 1, 1]
    shape[axis] = n
    delta = np.broadcast_to((A * np.cos(phase)).reshape(shape), (n, n, n)).astype(np.float32)
    psi = _lpt().zeldovich_displacement(delta, boxsize=box)
    want = np.broadcast_to((-A * box / (2.0 * np.pi * j) * np.sin(phase)).reshape(shape), (n, n, n))
    others = [c for c in range(3) if c != axis]
    print("axis %d: rel L2 %.3e, other axes max %.3e" % (axis, rel_l2(psi[axis], want), np.abs(psi[others]).max()))
    assert rel_l2(psi[axis], want) <= TOL
    assert np.all(psi[others] == 0)


def test_zeldovich_exact_zeros():
    lpt = _lpt()
    n = 8
    sign = (1.0 - 2.0 * (np.arange(n) % 2)).astype(np.float32)
    for axis in range(3):
        shape = [1, 1, 1]
        shape[axis] = n
        delta = np.ascontiguousarray(np.broadcast_to(sign.reshape(shape), (n, n, n)))
        assert np.all(lpt.zeldovich_displacement(delta, boxsize=L) == 0)
    assert np.all(lpt.zeldovich_displacement(np.full((n, n, n), 0.75, np.float32), boxsize=L) == 0)
    two = np.random.default_rng(2).standard_normal((2, 2, 2)).astype(np.float32)
    assert np.all(lpt.zeldovich_displacement(two, boxsize=L) == 0)


def test_zeldovich_scale_residency_and_reproducibility():
    torch, lpt = _torch(), _lpt()
    x = red_field(24, 7, np.float32)
    one = lpt.zeldovich_displacement(x, boxsize=L)
    assert np.array_equal(lpt.zeldovich_displacement(x, boxsize=L, scale=2.0), 2.0 * one)     # a power of two: exact
    assert rel_l2(lpt.zeldovich_displacement(x, boxsize=L, scale=-0.3), -0.3 * one.astype(np.float64)) <= TOL
    xt = torch.from_numpy(x).cuda()
    t = lpt.zeldovich_displacement(xt, boxsize=L)
    assert isinstance(t, torch.Tensor) and t.device == xt.device and t.dtype == torch.float32 and t.is_contiguous()
    assert np.array_equal(t.cpu().numpy(), one)
    assert np.array_equal(lpt.zeldovich_displacement(xt, boxsize=L).cpu().numpy(), one)
    assert np.array_equal(lpt.zeldovich_displacement(xt, boxsize=L, _max_batch=1).cpu().numpy(), one)


def test_zeldovich_feeds_process_box():
    torch, lpt = _torch(), _lpt()
    import jax_nbody_emulator_with_dj_amd as J
    from oracle import params as P
    cfg = J.SubboxConfig(size=(16, 16, 16), ndiv=(1, 1, 1), output_dtype=np.float32)
    emu = J.create_emulator(load_params=False, processor_config=cfg, mid_chan=8)
    emu.processor.params = P.synthetic_params(seed=71, mid_chan=8)
    psi = lpt.zeldovich_displacement(torch.from_numpy(np.float32(0.03) * red_field(16, 16, np.float32)).cuda(), boxsize=L)
    d_t, v_t = emu.process_box(psi, 0.5, 0.3, show_progress=False)
    d_n, v_n = emu.process_box(psi.cpu().numpy(), 0.5, 0.3, show_progress=False)
    assert np.array_equal(d_t.cpu().numpy(), np.asarray(d_n)) and np.array_equal(v_t.cpu().numpy(), np.asarray(v_n))
    assert np.isfinite(np.asarray(d_n)).all() and np.asarray(d_n).shape == (3, 16, 16, 16)


# ---- resizing -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_in, n_out", [(8, 16), (6, 18), (5, 15), (12, 20), (16, 8), (18, 6), (20, 12)])
def test_fourier_resize_vs_reference(n_in, n_out):
    x = red_field(n_in, 300 + n_in + n_out, np.float32)
    out = _lpt().resize_density(x, n_out, boxsize=L, upsample_method="fourier", downsample_method="fourier")
    assert out.dtype == np.float32 and out.shape == (n_out,) * 3
    err = rel_l2(out, R.fourier_resize(x, n_out))
    print("%d -> %d: rel L2 %.3e" % (n_in, n_out, err))
    assert err <= TOL


@pytest.mark.parametrize("n_in, n_out", [(8, 16), (6, 18), (5, 15), (12, 20)])
def test_fourier_round_trip_on_the_device(n_in, n_out):
    torch, lpt = _torch(), _lpt()
    x = torch.from_numpy(red_field(n_in, 400 + n_in, np.float32)).cuda()
    up = lpt.resize_density(x, n_out, boxsize=L, upsample_method="fourier")
    back = lpt.resize_density(up, n_in, boxsize=L, upsample_method="fourier", downsample_method="fourier")
    assert isinstance(back, torch.Tensor) and back.device == x.device
    err = rel_l2(back.cpu().numpy(), x.cpu().numpy())
    print("%d -> %d -> %d: rel L2 %.3e" % (n_in, n_out, n_in, err))
    assert err <= TOL
    if n_out % n_in == 0:
        r = n_out // n_in
        assert rel_l2(up[::r, ::r, ::r].cpu().numpy(), x.cpu().numpy()) <= TOL


@pytest.mark.parametrize("n_in, n_out", [(8, 16), (6, 18), (5, 15), (40, 80)])
def test_linear_upsampling(n_in, n_out):
    x = red_field(n_in, 500 + n_in, np.float32)
    out = _lpt().resize_density(x, n_out, boxsize=L, upsample_method="linear")
    r = n_out // n_in
    assert np.array_equal(out[::r, ::r, ::r], x)
    assert within_ulps(out, R.trilinear(x, n_out))


@pytest.mark.parametrize("n_in, n_out", [(24, 8), (16, 8), (80, 40)])
def test_block_average(n_in, n_out):
    x = red_field(n_in, 600 + n_in, np.float32)
    out = _lpt().resize_density(x, n_out, boxsize=L, upsample_method="fourier", downsample_method="block_average")
    assert within_ulps(out, R.block_average(x, n_out))


@pytest.mark.parametrize("n_in, n_out", [(24, 8), (16, 8)])
@pytest.mark.parametrize("sigma", [None, 90.0])
def test_gaussian_downsampling(n_in, n_out, sigma):
    lpt = _lpt()
    x = red_field(n_in, 700 + n_in, np.float32)
    out = lpt.resize_density(x, n_out, boxsize=L, upsample_method="fourier", gaussian_sigma=sigma)
    ref = R.resize_density(x, n_out, L, downsample_method="gaussian", gaussian_sigma=sigma)
    err = rel_l2(out, ref)
    s = L / n_out if sigma is None else sigma
    err_s = rel_l2(lpt.gaussian_smooth(x, L, s), R.gaussian_smooth(x, L, s))
    print("%d -> %d, sigma %s: rel L2 %.3e, smoothing alone %.3e" % (n_in, n_out, sigma, err, err_s))
    assert err <= TOL and err_s <= TOL


# ---- mode injection -------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[(12, 24), (16, 32), (15, 30)], ids=lambda p: "%d-%d" % p)
def injection(request):
    """One injection per size pair: the device's own source spectrum, the device result and the restatement of it."""
    torch, lpt = _torch(), _lpt()
    n_in, n_out = request.param
    k, pk = power_law_table(n_out, L)
    x = red_field(n_in, 800 + n_in, np.float32)
    xt = torch.from_numpy(x).cuda()
    src = lpt._half_spectrum(xt)
    table = lpt._validate_table(k, pk)
    got = lpt._inject_spectrum(src, n_in, n_out, table, L, 12345).cpu().numpy()
    ref = R.spectrum_inject(src.cpu().numpy().astype(np.complex128), n_in, n_out, k, pk, L, 12345)
    inside = 4 * R.mode_grid(n_out)[3] <= n_in * n_in
    return dict(n_in=n_in, n_out=n_out, k=k, pk=pk, x=x, xt=xt, src=src, table=table, got=got, ref=ref, inside=inside)


def test_inject_spectrum_vs_reference(injection):
    """Every mode within 2^-22 |ref| + 1e-30: float64 draws rounded once, four half-ulps for the separate roundings of the
    real and imaginary words and for libm differences."""
    I = injection
    assert I["got"].dtype == np.complex64 and I["got"].shape == I["ref"].shape
    err = np.abs(I["got"].astype(np.complex128) - I["ref"])
    bound = 2.0 ** -22 * np.abs(I["ref"]) + 1e-30
    print("%d -> %d: worst error / bound %.3f (inside %.3f, outside %.3f)"
          % (I["n_in"], I["n_out"], (err / bound).max(), (err / bound)[I["inside"]].max(), (err / bound)[~I["inside"]].max()))
    assert (err <= bound).all()
    assert (np.abs(I["ref"][~I["inside"]]) > 0).all()
    public = _lpt().inject_spectrum(I["x"], I["n_out"], boxsize=L, k_target=I["k"], pk_target=I["pk"], seed=12345)
    assert isinstance(public, np.ndarray) and np.array_equal(public, I["got"])


def test_inject_spectrum_sphere_seed_and_reproducibility(injection):
    lpt = _lpt()
    I = injection
    n_in, n_out, inside = I["n_in"], I["n_out"], I["inside"]
    sphere = lpt._resize_spectrum(I["src"], n_in, n_out, sphere=True).cpu().numpy()
    assert np.array_equal(I["got"][inside].view(np.uint32), sphere[inside].view(np.uint32))
    assert np.all(sphere[~inside] == 0)
    again = lpt._inject_spectrum(I["src"], n_in, n_out, I["table"], L, 12345).cpu().numpy()
    assert np.array_equal(again.view(np.uint32), I["got"].view(np.uint32))
    other = lpt._inject_spectrum(I["src"], n_in, n_out, I["table"], L, 12345 + (1 << 32)).cpu().numpy()
    assert np.array_equal(other[inside].view(np.uint32), I["got"][inside].view(np.uint32))
    assert not np.any(other[~inside] == I["got"][~inside])


def test_mode_inject_field_vs_reference(injection):
    I = injection
    out = _lpt().resize_density(I["xt"], I["n_out"], boxsize=L, upsample_method="mode_inject", k_target=I["k"],
                                pk_target=I["pk"], seed=12345)
    ref = R.resize_density(I["x"], I["n_out"], L, upsample_method="mode_inject", k_target=I["k"], pk_target=I["pk"],
                           seed=12345)
    err = rel_l2(out.cpu().numpy(), ref)
    print("%d -> %d: rel L2 %.3e" % (I["n_in"], I["n_out"], err))
    assert out.device == I["xt"].device and err <= TOL
