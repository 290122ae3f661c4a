"""The emulator's input (jax_nbody_emulator_with_dj_amd.lpt, lpt_input) on the CPU: the float64 restatement's own
properties (Philox known answers, real fields, shell power, Fourier interpolation identities, the Zel'dovich identity)
and every argument error, raised before any device work."""

import numpy as np
import pytest

import lpt_ref as R
from lpt_ref import power_law_table, red_field
from jax_nbody_emulator_with_dj_amd import lpt as T
from jax_nbody_emulator_with_dj_amd import lpt_input as CLI


# ---- Philox -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("counter, key, answer", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
])
def test_philox_known_answers(counter, key, answer):
    out = R.philox4x32_10(*counter, *key)
    assert " ".join("%08x" % int(v) for v in out) == answer


def test_philox_is_elementwise():
    c = np.arange(24, dtype=np.uint64).reshape(2, 3, 4)
    a = R.philox4x32_10(c, c + 1, c * 7, 0 * c, 5, 9)
    for idx in [(0, 0, 0), (1, 2, 3)]:
        b = R.philox4x32_10(int(c[idx]), int(c[idx]) + 1, int(c[idx]) * 7, 0, 5, 9)
        assert [int(v[idx]) for v in a] == [int(v) for v in b]


# ---- mode injection ---------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def injected():
    out = {}
    for n_out in (24, 32):
        n_in = n_out // 2
        k, pk = power_law_table(n_out, 1000.0)
        src = np.fft.rfftn(red_field(n_in, 100 + n_out))
        out[n_out] = (n_in, k, pk, R.spectrum_inject(src, n_in, n_out, k, pk, 1000.0, 12345))
    return out


@pytest.mark.parametrize("n_out", [24, 32])
def test_injected_spectrum_is_that_of_a_real_field(injected, n_out):
    _, _, _, S = injected[n_out]
    back = np.fft.rfftn(np.fft.irfftn(S, s=(n_out,) * 3, axes=(0, 1, 2)))
    assert np.abs(back - S).max() <= 1e-12 * np.abs(S).max()
    field = np.fft.ifftn(R.full_spectrum(S, n_out))
    assert np.abs(field.imag).max() <= 1e-12 * np.abs(field.real).max()


@pytest.mark.parametrize("n_out", [24, 32])
def test_injected_shell_power(injected, n_out):
    """Outside the sphere every shell b = rint(|m|) with at least 200 modes of the full grid has a mean |F|^2 / sigma^2
    within four standard deviations of 1: the mean of nmodes / 2 independent exponentials."""
    n_in, k, pk, S = injected[n_out]
    _, _, _, q = R.mode_grid(n_out)
    w = np.broadcast_to(R.full_grid_weight(n_out), S.shape)
    sigma = R.inject_sigma(n_out, 1000.0, k, pk)
    outside = 4 * q > n_in * n_in
    shell = np.rint(np.sqrt(q)).astype(int)
    ratio = np.abs(S) ** 2 / sigma ** 2
    checked = 0
    for b in np.unique(shell[outside]):
        sel = outside & (shell == b)
        nmodes = int(w[sel].sum())
        if nmodes < 200:
            continue
        mean = float((w[sel] * ratio[sel]).sum() / nmodes)
        dev = abs(mean - 1.0) * np.sqrt(nmodes / 2.0)
        print("n_out %d shell %d: %d modes, mean %.4f, %.2f sigma" % (n_out, b, nmodes, mean, dev))
        assert dev <= 4.0
        checked += 1
    assert checked >= 5


def test_injection_keeps_the_sphere_and_depends_on_the_seed(injected):
    n_in, k, pk, S = injected[24]
    src = np.fft.rfftn(red_field(n_in, 124))
    _, _, _, q = R.mode_grid(24)
    inside = 4 * q <= n_in * n_in
    assert np.array_equal(S[inside], R.spectrum_resize(src, n_in, 24, sphere=True)[inside])
    other = R.spectrum_inject(src, n_in, 24, k, pk, 1000.0, 12346)
    assert np.array_equal(other[inside], S[inside]) and not np.any(other[~inside] == S[~inside])
    assert np.array_equal(R.spectrum_inject(src, n_in, 24, k, pk, 1000.0, 12345), S)


def test_table_power_is_interp_with_a_power_law_tail():
    k = np.array([0.1, 0.2, 0.4, 0.8])
    pk = 3.0 * k ** -2.0
    slope, intercept = R.tail_fit(k, pk)
    assert slope == pytest.approx(-2.0, abs=1e-12) and np.exp(intercept) == pytest.approx(3.0, rel=1e-12)
    got = R.table_power(np.array([0.05, 0.1, 0.3, 0.8, 1.6]), k, pk, slope, intercept)
    np.testing.assert_allclose(got, [pk[0], pk[0], 0.5 * (pk[1] + pk[2]), pk[3], 3.0 * 1.6 ** -2.0], rtol=1e-12)
    assert R.table_power(np.array([0.3]), k, -pk, slope, intercept)[0] == 0.0


# ---- Fourier interpolation --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n_in, n_out", [(8, 16), (6, 18), (5, 15), (8, 24)])
def test_fourier_upsampling_returns_the_input_at_the_coarse_nodes(n_in, n_out):
    x = red_field(n_in, n_in + n_out)
    r = n_out // n_in
    up = R.fourier_resize(x, n_out)
    assert np.abs(up[::r, ::r, ::r] - x).max() <= 1e-12
    S = R.spectrum_resize(np.fft.rfftn(x), n_in, n_out)
    assert np.abs(np.fft.ifftn(R.full_spectrum(S, n_out)).imag).max() <= 1e-12


@pytest.mark.parametrize("n_in, n_out", [(8, 16), (6, 18), (5, 15), (8, 24), (12, 20), (9, 12), (7, 8)])
def test_fourier_round_trip(n_in, n_out):
    x = red_field(n_in, 3 * n_in + n_out)
    assert np.abs(R.fourier_resize(R.fourier_resize(x, n_out), n_in) - x).max() <= 1e-12


@pytest.mark.parametrize("n_in, n_out", [(16, 8), (18, 6), (20, 12), (15, 5)])
def test_fourier_downsampling_is_real(n_in, n_out):
    S = R.spectrum_resize(np.fft.rfftn(red_field(n_in, n_in - n_out)), n_in, n_out)
    assert np.abs(np.fft.ifftn(R.full_spectrum(S, n_out)).imag).max() <= 1e-12
    assert np.abs(np.fft.rfftn(np.fft.irfftn(S, s=(n_out,) * 3, axes=(0, 1, 2))) - S).max() <= 1e-12 * np.abs(S).max()


# ---- Zel'dovich ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 15])
def test_zeldovich_divergence_is_minus_delta(n):
    L, scale = 250.0, 0.8
    spec = np.fft.rfftn(red_field(n, n))
    psi = R.zeldovich_spectrum(spec, n, L, scale)
    m0, m1, m2, q = R.mode_grid(n)
    kf = 2.0 * np.pi / L
    div = 1j * kf * (m0 * psi[0] + m1 * psi[1] + m2 * psi[2])
    plain = (q > 0) & np.broadcast_to((abs(m0) * 2 != n) & (abs(m1) * 2 != n) & (m2 * 2 != n), q.shape)
    assert np.abs(div[plain] + scale * spec[plain]).max() <= 1e-12 * np.abs(spec).max()
    assert np.all(psi[:, 0, 0, 0] == 0)
    if n % 2 == 0:
        assert np.all(psi[0, n // 2] == 0) and np.all(psi[1, :, n // 2] == 0) and np.all(psi[2, :, :, n // 2] == 0)
    assert np.abs(np.fft.ifftn(R.full_spectrum(psi[1], n)).imag).max() <= 1e-12


def test_zeldovich_plane_wave():
    n, L, A, j = 16, 100.0, 0.3, 2
    x = np.arange(n) * L / n
    psi = R.zeldovich_displacement(np.broadcast_to(A * np.cos(2 * np.pi * j * x / L)[None, :, None], (n, n, n)), L)
    want = -A * L / (2 * np.pi * j) * np.sin(2 * np.pi * j * x / L)
    assert np.abs(psi[1] - want[None, :, None]).max() <= 1e-12 and np.abs(psi[[0, 2]]).max() <= 1e-12


# ---- real-space passes --------------------------------------------------------------------------------------------------------

def test_trilinear_and_block_average_restatements():
    x = red_field(6, 5)
    up = R.trilinear(x, 18)
    assert np.array_equal(up[::3, ::3, ::3], x)
    assert up[1, 0, 0] == pytest.approx((2 * x[0, 0, 0] + x[1, 0, 0]) / 3, rel=1e-14)
    assert up[17, 3, 17] == pytest.approx(((x[5, 1, 5] + 2 * x[0, 1, 5]) / 3 + 2 * (x[5, 1, 0] + 2 * x[0, 1, 0]) / 3) / 3, rel=1e-13)
    assert R.block_average(up, 6).shape == (6, 6, 6)
    assert R.block_average(x, 3)[1, 2, 0] == pytest.approx(x[2:4, 4:6, 0:2].mean(), rel=1e-14)
    assert np.abs(R.gaussian_smooth(x, 100.0, 1e-9) - x).max() <= 1e-12


# ---- argument errors: before any device work ------------------------------------------------------------------------------------

F = np.zeros((8, 8, 8), np.float32)
K, PK = np.array([0.01, 0.1, 1.0]), np.array([1.0e4, 1.0e3, 10.0])


@pytest.mark.parametrize("call", [
    lambda: T.zeldovich_displacement(np.zeros((8, 8, 4), np.float32)),
    lambda: T.zeldovich_displacement(np.zeros((8, 8), np.float32)),
    lambda: T.zeldovich_displacement(F.astype(np.float64)),
    lambda: T.zeldovich_displacement([[[0.0]]]),
    lambda: T.zeldovich_displacement(np.zeros((1, 1, 1), np.float32)),
    lambda: T.zeldovich_displacement(F, boxsize=-1.0),
    lambda: T.zeldovich_displacement(F, boxsize=(1.0, 2.0, 1.0)),
    lambda: T.zeldovich_displacement(F, scale=float("nan")),
    lambda: T.zeldovich_displacement(F, scale="1"),
    lambda: T.gaussian_smooth(F, 100.0, 0.0),
    lambda: T.gaussian_smooth(F, 100.0, float("inf")),
    lambda: T.gaussian_smooth(F.astype(np.float16), 100.0, 1.0),
    lambda: T.gaussian_smooth(np.zeros((8, 4, 8), np.float32), 100.0, 1.0),
    lambda: T.resize_density(F, 16),
    lambda: T.resize_density(F, 16, upsample_method="cubic"),
    lambda: T.resize_density(F, 4, upsample_method="fourier", downsample_method="nearest"),
    lambda: T.resize_density(F, 8, upsample_method="nearest"),
    lambda: T.resize_density(F, 16.0, upsample_method="fourier"),
    lambda: T.resize_density(F, 1, upsample_method="fourier"),
    lambda: T.resize_density(F, 4096, upsample_method="fourier"),
    lambda: T.resize_density(F, 12, upsample_method="linear"),
    lambda: T.resize_density(F, 3, upsample_method="fourier", downsample_method="gaussian"),
    lambda: T.resize_density(F, 3, upsample_method="fourier", downsample_method="block_average"),
    lambda: T.resize_density(F, 4, upsample_method="fourier", gaussian_sigma=-1.0),
    lambda: T.resize_density(F.astype(np.float64), 16, upsample_method="fourier"),
    lambda: T.resize_density(np.zeros((8, 8, 6), np.float32), 16, upsample_method="fourier"),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject"),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K[::-1], pk_target=PK),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K[[0, 1, 1]], pk_target=PK),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K[:1], pk_target=PK[:1]),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K, pk_target=PK[:2]),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K, pk_target=-PK),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K, pk_target=PK, seed=-1),
    lambda: T.resize_density(F, 16, upsample_method="mode_inject", k_target=K, pk_target=PK, seed=1.5),
    lambda: T.inject_spectrum(F, 4, k_target=K, pk_target=PK),
    lambda: T.inject_spectrum(F, 16),
    lambda: T.inject_spectrum(F, 16, k_target=K[::-1], pk_target=PK),
])
def test_argument_errors_come_before_any_device_work(call, monkeypatch):
    from jax_nbody_emulator_with_dj_amd import density
    monkeypatch.setattr(density, "_device", lambda: pytest.fail("device work before validation"))
    monkeypatch.setattr(T, "_device_of", lambda x: pytest.fail("device work before validation"))
    with pytest.raises(ValueError):
        call()


def test_a_cpu_tensor_is_refused():
    import torch
    with pytest.raises(ValueError, match="CUDA"):
        T.zeldovich_displacement(torch.zeros(8, 8, 8))


def test_equal_sizes_return_the_input():
    assert T.resize_density(F, 8, upsample_method="fourier") is F


def test_valid_calls_need_a_device():
    import torch
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    for call in (lambda: T.zeldovich_displacement(F), lambda: T.resize_density(F, 16, upsample_method="fourier"),
                 lambda: T.gaussian_smooth(F, 100.0, 2.0), lambda: T.inject_spectrum(F, 16, k_target=K, pk_target=PK)):
        with pytest.raises(NBEError, match="no HIP device"):
            call()


def test_module_is_not_exported_from_the_package():
    import jax_nbody_emulator_with_dj_amd as J
    assert "lpt" not in J.__all__ and not set(T.__all__) & set(J.__all__)
    assert T.__all__ == ["zeldovich_displacement", "resize_density", "gaussian_smooth"] and callable(T.inject_spectrum)


# ---- driver ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def cli_files(tmp_path, monkeypatch):
    from jax_nbody_emulator_with_dj_amd import density
    monkeypatch.setattr(density, "_device", lambda: pytest.fail("device work before validation"))
    np.save(tmp_path / "delta.npy", F)
    np.save(tmp_path / "flat.npy", np.zeros((8, 8), np.float32))
    np.save(tmp_path / "slab.npy", np.zeros((8, 8, 4), np.float32))
    np.save(tmp_path / "complex.npy", np.zeros((8, 8, 8), np.complex64))
    np.savetxt(tmp_path / "pk.txt", np.column_stack([K, PK]), header="k_h_per_Mpc Pk_Mpc_over_h_cubed")
    np.savetxt(tmp_path / "unsorted.txt", np.column_stack([K[::-1], PK]))
    np.savetxt(tmp_path / "three.txt", np.column_stack([K, PK, PK]))

    def argv(delta="delta.npy", npart="16", up="fourier", extra=()):
        return ["--delta_files", str(tmp_path / delta), "--output_dirs", str(tmp_path), "--npart", npart,
                "--upsample_method", up] + [str(tmp_path / e) if e.endswith(".txt") else e for e in extra]
    return argv


@pytest.mark.parametrize("kw", [
    dict(delta="missing.npy"), dict(delta="flat.npy"), dict(delta="slab.npy"), dict(delta="complex.npy"),
    dict(npart="1"), dict(npart="4096"), dict(npart="x"), dict(up="cubic"),
    dict(extra=["--downsample_method", "nearest"]), dict(extra=["--boxsize", "-5"]), dict(extra=["--scale", "nan"]),
    dict(extra=["--gaussian_sigma", "0"]), dict(npart="12", up="linear"),
    dict(npart="3", extra=["--downsample_method", "block_average"]), dict(npart="3"),
    dict(up="mode_inject"), dict(up="mode_inject", extra=["--pk_table", "unsorted.txt"]),
    dict(up="mode_inject", extra=["--pk_table", "three.txt"]), dict(up="mode_inject", extra=["--pk_table", "none.txt"]),
    dict(up="mode_inject", extra=["--pk_table", "pk.txt", "--seed", "-3"]),
])
def test_cli_argument_errors(cli_files, kw):
    with pytest.raises(SystemExit) as e:
        CLI.main(cli_files(**kw))
    assert e.value.code not in (0, None)


def test_cli_reads_the_reference_table_format(cli_files, tmp_path):
    k, pk = CLI.read_table(tmp_path / "pk.txt")
    assert np.array_equal(k, K) and np.array_equal(pk, PK)
