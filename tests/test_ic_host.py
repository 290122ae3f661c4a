"""The linear field drawn from a seed (lpt.gaussian_spectrum and friends, ic_input) on the CPU: the properties of the
float64 restatement tests/ic_ref.py that the definition promises (Hermitian planes, draws that do not depend on the mesh
size, Gaussian statistics) and every argument error, raised before any device work."""

import numpy as np
import pytest

import ic_ref as I
import lpt_ref as R
from lpt_ref import power_law_table
from jax_nbody_emulator_with_dj_amd import ic_input as CLI
from jax_nbody_emulator_with_dj_amd import lpt as T

L = 1000.0


# ---- the restatement ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [3, 4, 8, 9])
@pytest.mark.parametrize("flags", [0, I.FIXED, I.INVERT, I.WHITE])
def test_half_spectrum_is_hermitian_on_the_paired_planes(n, flags):
    k, pk = power_law_table(n, L)
    S = I.gaussian_spectrum(n, L, k, pk, seed=77, scale=0.9, flags=flags)
    mirror = (-np.arange(n)) % n
    for i2 in sorted({0, n // 2} if n % 2 == 0 else {0}):
        plane = S[:, :, i2]
        assert np.array_equal(plane[mirror][:, mirror], np.conj(plane))
    assert S[0, 0, 0] == 0
    field = np.fft.ifftn(R.full_spectrum(S, n))
    assert np.abs(field.imag).max() <= 1e-12 * np.abs(field.real).max()
    back = np.fft.rfftn(np.fft.irfftn(S, s=(n,) * 3, axes=(0, 1, 2)))
    assert np.abs(back - S).max() <= 1e-12 * np.abs(S).max()


def _by_wave_vector(n, values, cut):
    """{(m0, m1, m2): value} of the half spectrum's modes with every |m_c| < cut."""
    m = R.wave_numbers(n)
    out = {}
    for i0 in range(n):
        for i1 in range(n):
            for i2 in range(n // 2 + 1):
                if max(abs(m[i0]), abs(m[i1]), i2) < cut:
                    out[(int(m[i0]), int(m[i1]), i2)] = values[i0, i1, i2]
    return out


def test_draws_do_not_depend_on_the_mesh_size():
    """Every mode with all |m_c| < 4 has the same draw g (==) at n = 8 and n = 16, the plane i2 = 0 included: which row
    of a pair draws does not depend on n either."""
    g8, second8, _ = I.gaussian_draws(8, 2024)
    g16, second16, _ = I.gaussian_draws(16, 2024)
    a, b = _by_wave_vector(8, g8, 4), _by_wave_vector(16, g16, 4)
    assert sorted(a) == sorted(b) and len(a) == 7 * 7 * 4
    assert all(a[m] == b[m] for m in a)
    sa, sb = _by_wave_vector(8, second8, 4), _by_wave_vector(16, second16, 4)
    assert all(sa[m] == sb[m] for m in sa)
    k, pk = power_law_table(16, L)
    ratio = _by_wave_vector(16, I.sigma(16, L, k, pk, 0.7), 4)
    base = _by_wave_vector(8, I.sigma(8, L, k, pk, 0.7), 4)
    assert all(ratio[m] == 8.0 * base[m] for m in base)


def test_a_nyquist_row_is_not_nested():
    """At n = 8 the mode (4, 1, 2) sits on a Nyquist row; its counter is that of (4, 1, 2) at n = 16 as well, but the mode
    (-4, 1, 2), which n = 8 cannot tell from it, is a draw of its own at n = 16."""
    g8, _, _ = I.gaussian_draws(8, 5)
    g16, _, _ = I.gaussian_draws(16, 5)
    assert g8[4, 1, 2] == g16[4, 1, 2] and g16[12, 1, 2] != g16[4, 1, 2]


def test_streams_of_the_draw_and_of_the_injection_differ():
    g, _, _ = I.gaussian_draws(8, 9)
    h, _ = R.gaussian_draws(8, 9)
    assert not np.any(g[:, :, 1:4] == h[:, :, 1:4])


def test_statistics_of_the_draws():
    """n = 32, seed 12345, over the independent modes (not the second of a pair, not self, not DC): |g|^2 / 2 is
    exponential with mean 1 and variance 1, the phasor has mean 0 and variance 1/2 per component, and every shell of
    rounded |m| with at least 10 modes has a mean |g|^2 / 2 within 4 standard deviations of 1."""
    n = 32
    g, _, _ = I.gaussian_draws(n, 12345)
    ind = I.independent(n)
    e = np.abs(g[ind]) ** 2 / 2.0
    N = e.size
    z_mean = (e.mean() - 1.0) * np.sqrt(N)
    ph = (g[ind] / np.abs(g[ind])).mean()
    z_phase = np.abs(ph) * np.sqrt(N)                    # |mean phasor|^2 N is exponential with mean 1
    shell = np.rint(np.sqrt(R.mode_grid(n)[3])).astype(int)
    worst = 0.0
    for b in np.unique(shell[ind]):
        sel = ind & (shell == b)
        cnt = int(sel.sum())
        if cnt >= 10:
            worst = max(worst, abs((np.abs(g[sel]) ** 2 / 2.0).mean() - 1.0) * np.sqrt(cnt))
    print("z of mean |g|^2/2: %.2f, of the mean phasor: %.2f, worst shell: %.2f" % (z_mean, z_phase, worst))
    assert abs(z_mean) <= 4 and z_phase <= 4 and worst <= 4
    assert np.abs(g).max() <= np.sqrt(-2.0 * np.log(2.0 ** -33))


def test_fixed_amplitude_inverted_phase_and_white_noise():
    n = 8
    k, pk = power_law_table(n, L)
    s = np.broadcast_to(I.sigma(n, L, k, pk, 0.5), (n, n, n // 2 + 1))
    plain = I.gaussian_spectrum(n, L, k, pk, 3, 0.5)
    fixed = I.gaussian_spectrum(n, L, k, pk, 3, 0.5, I.FIXED)
    live = R.mode_grid(n)[3] > 0
    np.testing.assert_allclose(np.abs(fixed[live]), s[live], rtol=1e-14)
    own = I.pairing(n)[1]
    assert np.all(fixed[own].imag == 0) and np.all(plain[own].imag == 0)
    moving = live & ~own
    assert np.abs(np.angle(fixed[moving] / plain[moving])).max() <= 1e-12           # the same phases
    assert np.array_equal(I.gaussian_spectrum(n, L, k, pk, 3, 0.5, I.INVERT), np.where(live, -plain, 0))
    w = np.fft.irfftn(I.gaussian_spectrum(32, flags=I.WHITE, seed=4), s=(32,) * 3, axes=(0, 1, 2))
    assert abs(w.var() - 1.0) <= 4 * np.sqrt(2.0 / 32 ** 3) and abs(w.mean()) <= 1e-12
    white8 = np.fft.irfftn(I.gaussian_spectrum(n, flags=I.WHITE, seed=3), s=(n,) * 3, axes=(0, 1, 2))
    np.testing.assert_allclose(I.colour_noise(white8, L, k, pk, 0.5), np.fft.irfftn(plain, s=(n,) * 3, axes=(0, 1, 2)),
                               atol=1e-12 * np.abs(plain).max())


# ---- argument errors: before any device work ----------------------------------------------------------------------------------

K, PK = np.array([0.01, 0.1, 1.0]), np.array([1.0e4, 1.0e3, 10.0])
W = np.zeros((8, 8, 8), np.float32)


@pytest.mark.parametrize("call", [
    lambda: T.gaussian_field(1, L, K, PK),
    lambda: T.gaussian_field(4096, L, K, PK),
    lambda: T.gaussian_field(8.0, L, K, PK),
    lambda: T.gaussian_field(True, L, K, PK),
    lambda: T.gaussian_field(8, L),
    lambda: T.gaussian_field(8, L, K),
    lambda: T.gaussian_field(8, L, K[::-1], PK),
    lambda: T.gaussian_field(8, L, K[:1], PK[:1]),
    lambda: T.gaussian_field(8, L, K, -PK),
    lambda: T.gaussian_field(8, L, K, PK, seed=-1),
    lambda: T.gaussian_field(8, L, K, PK, seed=2 ** 64),
    lambda: T.gaussian_field(8, L, K, PK, seed=1.5),
    lambda: T.gaussian_field(8, L, K, PK, scale=0.0),
    lambda: T.gaussian_field(8, L, K, PK, scale=-1.0),
    lambda: T.gaussian_field(8, L, K, PK, scale=float("nan")),
    lambda: T.gaussian_field(8, -L, K, PK),
    lambda: T.gaussian_field(8, (L, L, 2 * L), K, PK),
    lambda: T.gaussian_field(8, L, K, PK, fixed_amplitude=1),
    lambda: T.gaussian_field(8, L, K, PK, invert_phase="no"),
    lambda: T.gaussian_field(8, L, K, PK, out="jax"),
    lambda: T.gaussian_field(8, L, K, PK, device="cpu"),
    lambda: T.gaussian_field(8, L, K, PK, _max_blocks=0),
    lambda: T.gaussian_spectrum(1, L, K, PK),
    lambda: T.gaussian_spectrum(8, L, K, PK, scale=0.0),
    lambda: T.gaussian_spectrum(8, L, K[::-1], PK),
    lambda: T.gaussian_spectrum(8, L, K, PK, seed=-1),
    lambda: T.white_noise(1),
    lambda: T.white_noise(8, seed=-1),
    lambda: T.white_noise(8, out="jax"),
    lambda: T.white_noise(8, device="cpu"),
    lambda: T.colour_noise(W, L, None, None),
    lambda: T.colour_noise(W, L, K[::-1], PK),
    lambda: T.colour_noise(W, L, K, PK, scale=0.0),
    lambda: T.colour_noise(W.astype(np.float64), L, K, PK),
    lambda: T.colour_noise(np.zeros((8, 8, 4), np.float32), L, K, PK),
    lambda: T.colour_noise(W, -1.0, K, PK),
    lambda: T.linear_ics(1, L, K, PK, 0),
    lambda: T.linear_ics(8, L, None, None, 0),
    lambda: T.linear_ics(8, L, K[::-1], PK, 0),
    lambda: T.linear_ics(8, L, K, PK, -1),
    lambda: T.linear_ics(8, L, K, PK, 0, scale=-2.0),
    lambda: T.linear_ics(8, L, K, PK, 0, return_delta=None),
])
def test_argument_errors_come_before_any_device_work(call, monkeypatch):
    from jax_nbody_emulator_with_dj_amd import density
    monkeypatch.setattr(density, "_device", lambda: pytest.fail("device work before validation"))
    monkeypatch.setattr(T, "_device_of", lambda x: pytest.fail("device work before validation"))
    with pytest.raises(ValueError):
        call()


def test_valid_calls_need_a_device():
    import torch
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    for call in (lambda: T.gaussian_spectrum(8, L, K, PK), lambda: T.gaussian_field(8, L, K, PK), lambda: T.white_noise(8),
                 lambda: T.colour_noise(W, L, K, PK), lambda: T.linear_ics(8, L, K, PK, 1)):
        with pytest.raises(NBEError, match="no HIP device"):
            call()


def test_names_symbols_and_constants():
    import os
    import re
    from jax_nbody_emulator_with_dj_amd import _lib
    for name in ("gaussian_spectrum", "gaussian_field", "white_noise", "colour_noise", "linear_ics"):
        assert callable(getattr(T, name))
    for name in ("nbe_gaussian_spectrum", "nbe_spectrum_colour"):
        assert name in _lib.SIGNATURES
    header = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nbe.h")
    H = {name: int(value) for name, value in re.findall(r"^#define (NBE_\w+)[ \t]+(\d+)\s*$", open(header).read(), re.M)}
    assert (T.FIXED_AMPLITUDE, T.INVERT_PHASE, T.WHITE_NOISE) == (H["NBE_IC_FIXED_AMPLITUDE"], H["NBE_IC_INVERT_PHASE"],
                                                                  H["NBE_IC_WHITE_NOISE"]) == (I.FIXED, I.INVERT, I.WHITE)


# ---- driver ---------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def cli_files(tmp_path, monkeypatch):
    from jax_nbody_emulator_with_dj_amd import density
    monkeypatch.setattr(density, "_device", lambda: pytest.fail("device work before validation"))
    for name in ("a", "b"):
        (tmp_path / name).mkdir()
    np.save(tmp_path / "white.npy", W)
    np.savetxt(tmp_path / "pk.txt", np.column_stack([K, PK]), header="k_h_per_Mpc Pk_Mpc_over_h_cubed")
    np.savetxt(tmp_path / "unsorted.txt", np.column_stack([K[::-1], PK]))

    def argv(seeds="1,2", dirs="seed_{seed}", npart="8", table="pk.txt", extra=()):
        out = ["--output_dirs", str(tmp_path / dirs), "--npart", npart]
        if seeds is not None:
            out += ["--seeds", seeds]
        if table is not None:
            out += ["--pk_table", str(tmp_path / table)]
        return out + [str(tmp_path / e) if e.endswith(".npy") else e for e in extra]
    return argv


@pytest.mark.parametrize("kw", [
    dict(npart="1"), dict(npart="4096"), dict(npart="x"),
    dict(table=None), dict(table="unsorted.txt"), dict(table="none.txt"),
    dict(seeds="-1,2"), dict(seeds="1,1"), dict(seeds="x"), dict(seeds="3:3"), dict(seeds=None),
    dict(extra=["--scale", "0"]), dict(extra=["--scale", "-1"]), dict(extra=["--scale", "nan"]),
    dict(extra=["--scale", "0.5", "--z", "1", "--omega_m", "0.3"]),
    dict(extra=["--z", "1"]), dict(extra=["--omega_m", "0.3"]), dict(extra=["--z", "-2", "--omega_m", "0.3"]),
    dict(extra=["--boxsize", "-5"]),
    dict(extra=["--white_noise_file", "white.npy"]),                       # with --seeds
    dict(seeds=None, dirs="a", extra=["--white_noise_file", "white.npy", "--fixed_amplitude"]),
    dict(seeds=None, dirs="seed_{seed}", extra=["--white_noise_file", "white.npy"]),
    dict(seeds=None, dirs="[ab]", extra=["--white_noise_file", "white.npy"]),
    dict(dirs="a"),                                                        # two seeds, one directory
    dict(seeds="1,2,3", dirs="[ab]"),
    dict(dirs="missing*"),
])
def test_cli_argument_errors(cli_files, kw, tmp_path):
    with pytest.raises(SystemExit) as e:
        CLI.main(cli_files(**kw))
    assert e.value.code not in (0, None)
    assert not list(tmp_path.glob("seed_*")) and not list(tmp_path.glob("*/lpt_dis.npy"))


def test_cli_seeds_dirs_and_scale(tmp_path):
    assert CLI.seed_list("1,2,3") == [1, 2, 3] and CLI.seed_list("4:7") == [4, 5, 6]
    assert CLI.output_dirs(str(tmp_path / "s{seed}"), [3, 5]) == [tmp_path / "s3", tmp_path / "s5"]
    (tmp_path / "x1").mkdir()
    (tmp_path / "x0").mkdir()
    assert CLI.output_dirs(str(tmp_path / "x*"), [8, 9]) == [tmp_path / "x0", tmp_path / "x1"]
    assert CLI.paired_dir(tmp_path / "x0") == tmp_path / "x0_paired"
    from jax_nbody_emulator_with_dj_amd.cosmology import growth_factor
    assert CLI.growth_scale(0.0, 0.3) == 1.0
    assert CLI.growth_scale(1.0, 0.3) == pytest.approx(float(growth_factor(1.0, 0.3)), rel=1e-6)
    a = CLI.build_parser().parse_args(["--seeds", "1", "--output_dirs", "d", "--npart", "8", "--pk_table", "t"])
    assert (a.boxsize, a.scale, a.z, a.fixed_amplitude, a.paired, a.save_delta, a.white_noise_file) == \
        (1000.0, None, None, False, False, True, None)
