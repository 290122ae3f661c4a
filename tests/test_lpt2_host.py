"""Second-order LPT on the CPU: the float64 restatement's own properties in exact-arithmetic
terms, the second-order growth against its limits and fits, every argument error, raised before any device work, and the
names the header and the binding share."""

import os
import re

import numpy as np
import pytest

import lpt2_ref as R2
from jax_nbody_emulator_with_dj_amd import _lib
from jax_nbody_emulator_with_dj_amd import cosmology as COS
from jax_nbody_emulator_with_dj_amd import density as D
from jax_nbody_emulator_with_dj_amd import lpt as T

EXACT = 1e-12


# ---- the restatement ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plane_wave_has_no_source(axis):
    delta = R2.plane_wave(16, 3, axis)
    assert np.abs(R2.lpt2_source(delta)).max() <= EXACT
    assert np.abs(R2.lpt2_source(delta, dealias=True)).max() <= EXACT
    psi1, psi2 = R2.lpt2_orders(delta, 100.0)
    assert np.abs(psi2).max() <= EXACT * np.abs(psi1).max()


@pytest.mark.parametrize("dealias", [False, True])
def test_crossed_waves(dealias):
    n, j1, j2, A, B, phi, L, scale, g = 16, 2, 3, 0.3, -0.2, 0.7, 100.0, 0.8, 0.43
    delta, cx, sx, cy, sy = R2.crossed_waves(n, j1, j2, A, B, phi)
    assert np.abs(R2.lpt2_source(delta, dealias) - A * B * cx * cy).max() <= EXACT
    b = g * scale * scale
    c = b * A * B * L / (2.0 * np.pi * (j1 * j1 + j2 * j2))
    _, psi2 = R2.lpt2_orders(delta, L, scale, g, dealias)
    assert np.abs(psi2[0] + c * j1 * sx * cy).max() <= EXACT * L
    assert np.abs(psi2[1] + c * j2 * cx * sy).max() <= EXACT * L
    assert np.abs(psi2[2]).max() <= EXACT * L


@pytest.mark.parametrize("n", [12, 15])
def test_source_has_zero_mean(n):
    """Parseval: sum_x h_ii h_jj = sum_k (d_i d_j)^2 / |m|^4 |delta_k|^2 = sum_x h_ij^2, with the same d in both."""
    s = R2.lpt2_source(R2.red_field(n, 40 + n))
    assert abs(s.mean()) <= EXACT * np.abs(s).max()


def test_trace_of_the_hessian_is_the_field():
    n = 12
    spec = np.fft.rfftn(R2.red_field(n, 5))
    d0, d1, d2, _ = R2.derivative_numbers(n)
    m0, m1, m2, _ = R2.mode_grid(n)
    spec = np.where((d0 == m0) & (d1 == m1) & (d2 == m2), spec, 0.0)             # no power on the Nyquist rows
    spec[0, 0, 0] = 0.0
    delta = np.fft.irfftn(spec, s=(n, n, n), axes=(0, 1, 2))
    h = R2.hessian_fields(spec, n, n)
    assert np.abs(h[0] + h[1] + h[2] - delta).max() <= EXACT * np.abs(delta).max()


def test_two_points_a_side_give_zeros():
    x = np.random.default_rng(2).standard_normal((2, 2, 2))
    assert np.all(R2.hessian_spectrum(np.fft.rfftn(x), 2) == 0)
    assert np.all(R2.lpt2_source(x) == 0) and np.all(R2.lpt2_source(x, dealias=True) == 0)
    assert np.all(R2.lpt2_displacement(x) == 0)


def test_band_limited_field_needs_no_dealiasing():
    """|m_c| <= 3 at n = 16: the products reach |m_c| = 6 < 8, so nothing folds back."""
    x = R2.band_limited(16, 9, 3)
    plain, fine = R2.lpt2_source(x), R2.lpt2_source(x, dealias=True)
    assert np.abs(plain - fine).max() <= EXACT * np.abs(plain).max() and np.abs(plain).max() > 0.1
    wide = R2.red_field(16, 9)
    assert np.abs(R2.lpt2_source(wide) - R2.lpt2_source(wide, dealias=True)).max() > 1e-3     # and a full band does


# ---- growth ---------------------------------------------------------------------------------------------------------------

def test_einstein_de_sitter_growth():
    z = np.array([0.0, 0.5, 1.0, 3.0, 49.0])
    a = 1.0 / (1.0 + z)
    d2, f2 = COS.growth_factor_2(z, 1.0), COS.growth_rate_2(z, 1.0)
    assert d2.dtype == np.float64 and d2.shape == z.shape
    assert np.abs(d2 / (-3.0 / 7.0 * a * a) - 1.0).max() <= 1e-9 and np.abs(f2 - 2.0).max() <= 1e-9


GRID_OM = np.array([0.1, 0.2, 0.3, 0.3175, 0.5, 1.0])[:, None]
GRID_Z = np.array([0.0, 0.5, 1.0, 3.0, 49.0])[None, :]


def test_growth_against_the_restatement_and_the_fits():
    """The ODE is the definition; -3/7 D1^2 Om(z)^(-1/143) and 2 Om(z)^(6/11) are fits to it.  With 20000 RK4 steps the
    fits are at worst 1.8e-4 (D2) and 1.23e-2 (f2, at Om = 0.1, z = 0) off."""
    d2, f2 = COS.growth_factor_2(GRID_Z, GRID_OM), COS.growth_rate_2(GRID_Z, GRID_OM)
    d1_ref, d2_ref, f2_ref = R2.growth2_ode(GRID_Z, GRID_OM)
    assert np.abs(d2 / d2_ref - 1.0).max() <= 1e-9 and np.abs(f2 / f2_ref - 1.0).max() <= 1e-9
    assert (d2 < 0).all()
    d1 = COS._growth_factor64(*COS._f64(GRID_Z, GRID_OM))
    assert np.abs(d1_ref / d1 - 1.0).max() <= 1e-6                # the matter-era start against the closed form
    omz = R2.matter_fraction(GRID_Z, GRID_OM)
    err_d = np.abs(d2 / (-3.0 / 7.0 * d1 * d1 * omz ** (-1.0 / 143.0)) - 1.0)
    err_f = np.abs(f2 / (2.0 * omz ** (6.0 / 11.0)) - 1.0)
    print("fits: D2 worst %.3e, f2 worst %.3e (Om >= 0.2: %.3e)" % (err_d.max(), err_f.max(), err_f[1:].max()))
    assert err_d.max() <= 5e-4 and err_f.max() <= 2e-2
    with pytest.raises(ValueError):
        COS.growth_factor_2(-1.0, 0.3)
    with pytest.raises(ValueError):
        COS.growth_rate_2(0.0, 0.0)


# ---- argument errors: before any device work ------------------------------------------------------------------------------

F = np.zeros((8, 8, 8), np.float32)
ODD = np.zeros((9, 9, 9), np.float32)
K = np.geomspace(0.003, 0.3, 24)
PK = 2.0e4 * (K / 0.1) ** -1.7


def _huge(n):
    return np.lib.stride_tricks.as_strided(np.zeros(1, np.float32), (n,) * 3, (0, 0, 0))


@pytest.mark.parametrize("call", [
    lambda: T.lpt2_source(np.zeros((8, 8, 4), np.float32)),
    lambda: T.lpt2_displacement(np.zeros((8, 8, 4), np.float32)),
    lambda: T.lpt2_displacement(np.zeros((8, 8), np.float32)),
    lambda: T.lpt2_displacement(F.astype(np.float64)),
    lambda: T.lpt2_displacement(np.zeros((1, 1, 1), np.float32)),
    lambda: T.lpt2_displacement(F, boxsize=(1.0, 2.0, 1.0)),
    lambda: T.lpt2_displacement(F, boxsize=0.0),
    lambda: T.lpt2_source(ODD, dealias=True),
    lambda: T.lpt2_displacement(ODD, dealias=True),
    lambda: T.lpt2_source(_huge(1366), dealias=True),             # 3 n / 2 = 2049
    lambda: T.lpt2_displacement(_huge(1366), dealias=True),
    lambda: T.lpt2_source(F, dealias=1),
    lambda: T.lpt2_displacement(F, growth2=np.inf),
    lambda: T.lpt2_displacement(F, growth2=np.nan),
    lambda: T.lpt2_displacement(F, growth2=True),
    lambda: T.lpt2_displacement(F, scale=np.inf),
    lambda: T.lpt2_displacement(F, return_orders=1),
    lambda: T.linear_ics(8, 100.0, K, PK, 1, order=0),
    lambda: T.linear_ics(8, 100.0, K, PK, 1, order=3),
    lambda: T.linear_ics(8, 100.0, K, PK, 1, order=2.0),
    lambda: T.linear_ics(8, 100.0, K, PK, 1, order=True),
    lambda: T.linear_ics(8, 100.0, K, PK, 1, order=2, growth2=np.nan),
    lambda: T.linear_ics(9, 100.0, K, PK, 1, order=2, dealias=True),
    lambda: T.linear_ics(1366, 100.0, K, PK, 1, order=2, dealias=True),
])
def test_argument_errors_come_before_any_device_work(call, monkeypatch):
    monkeypatch.setattr(D, "_device", lambda: pytest.fail("device work before validation"))
    monkeypatch.setattr(T, "_device_of", lambda x: pytest.fail("device work before validation"))
    with pytest.raises(ValueError):
        call()


def test_error_messages_name_the_argument():
    with pytest.raises(ValueError, match="lpt2_displacement needs a cubic"):
        T.lpt2_displacement(np.zeros((8, 8, 4), np.float32))
    with pytest.raises(ValueError, match="dealias=True needs an even n"):
        T.lpt2_source(ODD, dealias=True)
    with pytest.raises(ValueError, match="3 n / 2 <= 2048, got 1366"):
        T.lpt2_displacement(_huge(1366), dealias=True)
    with pytest.raises(ValueError, match="growth2 must be a finite number"):
        T.lpt2_displacement(F, growth2=np.inf)
    with pytest.raises(ValueError, match="order must be 1 or 2"):
        T.linear_ics(8, 100.0, K, PK, 1, order=3)


def test_no_device_means_loud_failure(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    for call in (lambda: T.lpt2_source(F), lambda: T.lpt2_displacement(F, dealias=True),
                 lambda: T.linear_ics(8, 100.0, K, PK, 1, order=2)):
        with pytest.raises(_lib.NBEError, match="no HIP device"):
            call()


def test_names_symbols_and_constants():
    header = open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include", "nbe.h")).read()
    for name in ("nbe_lpt2_hessian_spectrum", "nbe_lpt2_source", "nbe_lpt2_spectrum"):
        assert name in _lib.SIGNATURES and re.search(r"^int %s\(" % name, header, re.M)
    for name in ("lpt2_source", "lpt2_displacement"):
        assert callable(getattr(T, name))        # like divergence and linear_ics, not in __all__, which test_lpt_host.py pins
    H = {name: int(value) for name, value in re.findall(r"^#define (NBE_\w+)[ \t]+(\d+)\s*$", header, re.M)}
    assert T.COMPONENTS == H["NBE_LPT2_COMPONENTS"] == len(R2.PAIRS) == 6
    assert T.EDS_GROWTH2 == 3.0 / 7.0
    assert (COS.GROWTH2_STEPS, COS.GROWTH2_START) == (20000, 1.0e-4)


def test_driver_flags(tmp_path):
    from jax_nbody_emulator_with_dj_amd import ic_input, lpt_input
    ns = ic_input.build_parser().parse_args(["--output_dirs", "x", "--npart", "16", "--pk_table", "t"])
    assert (ns.lpt_order, ns.growth2, ns.lpt2_dealias) == (1, None, False)
    assert lpt_input.lpt2_options(ns, False, "--lpt_order 2") is None
    assert lpt_input.lpt2_options(ns, True, "--lpt_order 2") == 3.0 / 7.0
    ns.growth2 = 0.43
    assert lpt_input.lpt2_options(ns, True, "--lpt_order 2") == 0.43
    with pytest.raises(ValueError, match="need --lpt_order 2"):
        lpt_input.lpt2_options(ns, False, "--lpt_order 2")
    ns.npart, ns.lpt2_dealias = 15, True
    with pytest.raises(ValueError, match="even n"):
        lpt_input.lpt2_options(ns, True, "--lpt_order 2")
    g = ic_input.growth2_of(0.5, 0.3175)
    assert abs(g / (3.0 / 7.0) - 1.0) < 5e-3 and g == ic_input.growth2_of(0.5, 0.3175)
    np.savetxt(tmp_path / "pk.txt", np.column_stack([K, PK]))
    base = ["--seeds", "1", "--output_dirs", str(tmp_path / "s{seed}"), "--npart", "16", "--pk_table", str(tmp_path / "pk.txt")]
    parse = ic_input.build_parser().parse_args
    assert ic_input.validate(parse(base))[5] is None
    assert ic_input.validate(parse(base + ["--lpt_order", "2"]))[5] == 3.0 / 7.0
    assert ic_input.validate(parse(base + ["--lpt_order", "2", "--z", "0.5", "--omega_m", "0.3175"]))[5] == g
    assert ic_input.validate(parse(base + ["--lpt_order", "2", "--z", "0.5", "--omega_m", "0.3175", "--growth2", "0.4"]))[5] == 0.4
    for bad in (["--lpt_order", "3"], ["--growth2", "0.4"], ["--lpt2_dealias"]):
        with pytest.raises(ValueError):
            ic_input.validate(parse(base + bad))
