"""Per-particle fields (density.paint_field, the line-of-sight shift of paint_density, rsd_factor) on the CPU: the float64
reference by hand, the integer scheme's bounds on its NumPy restatement, argument validation before any device work, the
missing-device error and the --paint_vel / --rsd flags."""

import argparse

import numpy as np
import pytest

import field_ref as F
from jax_nbody_emulator_with_dj_amd import _lib
from jax_nbody_emulator_with_dj_amd import cosmology
from jax_nbody_emulator_with_dj_amd import density as D
from jax_nbody_emulator_with_dj_amd import run_emulator as CLI
from test_density_host import _base_argv, two_particle_cic_case


def test_reference_two_particles_by_hand():
    """The two particles of two_particle_cic_case carry q = 2 and q = -3 (second channel: 0.5 and 0.25)."""
    disp, m = two_particle_cic_case()
    eps = 1.0 / 64.0
    m0, m1 = np.zeros((4, 4, 4)), np.zeros((4, 4, 4))
    for (x, wx) in ((3, eps), (0, 1.0 - eps)):
        for (y, wy) in ((0, 0.75), (1, 0.25)):
            m0[x, y, 0] += wx * wy
        for (y, wy) in ((0, 0.5), (1, 0.5)):
            for (z, wz) in ((1, 0.5), (2, 0.5)):
                m1[x, y, z] += wx * wy * wz
    np.testing.assert_allclose(m0 + m1, m, rtol=0, atol=1e-15)
    q = np.array([[2.0, -3.0], [0.5, 0.25]], np.float32).reshape(2, 2, 1, 1)
    num, mass, count, absq = F.paint(disp, q, 4.0, 4, 2)
    np.testing.assert_allclose(mass, m, rtol=0, atol=1e-15)
    np.testing.assert_allclose(num[0], 2.0 * m0 - 3.0 * m1, rtol=0, atol=1e-15)
    np.testing.assert_allclose(num[1], 0.5 * m0 + 0.25 * m1, rtol=0, atol=1e-15)
    np.testing.assert_array_equal(count, (m0 > 0).astype(np.int64) + (m1 > 0))
    np.testing.assert_array_equal(absq[0], 2.0 * (m0 > 0) + 3.0 * (m1 > 0))
    # a single (N0, N1, N2) quantity is channel 0; no displacement is the lattice itself
    np.testing.assert_array_equal(F.paint(disp, q[0], 4.0, 4, 2)[0][0], num[0])
    lat = F.paint(None, q[0], 4.0, (2, 1, 1), 1)
    np.testing.assert_array_equal(lat[0][0].ravel(), [2.0, -3.0])
    A, e = F.exponents(q)
    assert A.tolist() == [3.0, 0.5] and e.tolist() == [2, 0]            # A < 2^e: 3 < 4, 0.5 < 1


def _case(n, seed):
    rng = np.random.default_rng(seed)
    disp = (rng.standard_normal((3, n, n, n)) * 1.7 * (100.0 / n)).astype(np.float32)
    q = (rng.standard_normal((3, n, n, n)) * np.array([1.0, 300.0, 1e-3])[:, None, None, None]).astype(np.float32)
    return disp, q


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("scale", [0.5, 1, 2])
def test_integer_scheme_meets_the_test_bounds(worder, scale):
    """The arithmetic contract restated in NumPy (field_ref.emulate) against the float64 reference, through the checks the
    GPU tests use: the bounds hold for the scheme itself, with room (the measured worst ratio is below 0.5)."""
    n = 12
    disp, q = _case(n, 100 + worder)
    res = int(n * scale)
    ref = F.paint(disp, q, 100.0, res, worder)
    mean, mass = F.emulate(disp, q, 100.0, res, worder, "mean")
    assert int(mass.sum()) == n ** 3 * 2 ** 22                              # every particle adds exactly its unit mass
    assert F.check_mean(mean, q, ref, n ** 3) < 0.5
    dens, _ = F.emulate(disp, q, 100.0, res, worder, "density", 0.0)
    F.check_density(dens, q, ref)
    filled, _ = F.emulate(disp, q, 100.0, res, worder, "density", -7.5)
    assert (filled[:, ref[2] == 0] == np.float32(-7.5)).all()
    # the tight bound of the scheme: 2^-22 sum |q| + m 2^(e - 25)
    A, e = F.exponents(q)
    g = mean.astype(np.float64) * (n ** 3 / mass.size)
    for c in range(3):
        tight = F.UNIT * ref[3][c] + ref[1] * 2.0 ** (e[c] - 25) + 6e-8 * np.abs(ref[0][c])
        assert (np.abs(g[c] - ref[0][c]) <= tight + 1e-300).all()


def test_checks_reject_a_wrong_field():
    n = 12
    disp, q = _case(n, 7)
    ref = F.paint(disp, q, 100.0, n, 2)
    mean, _ = F.emulate(disp, q, 100.0, n, 2, "mean")
    bad = mean.copy()
    bad[1][np.unravel_index(np.argmax(np.abs(ref[0][1])), ref[1].shape)] *= np.float32(1.0 + 1e-4)
    with pytest.raises(AssertionError):
        F.check_mean(bad, q, ref, n ** 3)
    dens, _ = F.emulate(disp, q, 100.0, n, 2, "density")
    bad = dens.copy()
    bad[2][np.unravel_index(np.argmax(np.abs(ref[0][2])), ref[1].shape)] *= np.float32(1.0 + 1e-4)
    with pytest.raises(AssertionError):
        F.check_density(bad, q, ref)


# ---- argument validation: ValueError before any device work ---------------------------------------------------------

def test_names_are_public():
    for name in ("paint_field", "paint_density", "rsd_factor"):
        assert name in D.__all__ and callable(getattr(D, name))


def test_paint_field_validation():
    import torch
    disp = np.zeros((3, 4, 4, 4), np.float32)
    q = np.zeros((4, 4, 4), np.float32)
    for bad in (np.zeros((5, 4, 4, 4), np.float32), np.zeros((4, 4), np.float32), np.zeros((0, 4, 4, 4), np.float32),
                np.zeros((2, 3, 4, 4, 4), np.float32)):
        with pytest.raises(ValueError, match="quantity must have shape"):
            D.paint_field(disp, bad, 100.0, 4)
    with pytest.raises(ValueError, match="lattice shape"):
        D.paint_field(disp, np.zeros((4, 4, 5), np.float32), 100.0, 4)
    with pytest.raises(ValueError, match="lattice shape"):
        D.paint_field(disp, np.zeros((2, 4, 5, 4), np.float32), 100.0, 4)
    with pytest.raises(ValueError, match="quantity must be float32 or float16"):
        D.paint_field(disp, q.astype(np.float64), 100.0, 4)
    with pytest.raises(ValueError, match="NumPy array"):
        D.paint_field(disp, q.tolist(), 100.0, 4)
    with pytest.raises(ValueError, match="CUDA"):
        D.paint_field(None, torch.zeros(4, 4, 4), 100.0, 4)
    with pytest.raises(ValueError, match="shape"):
        D.paint_field(np.zeros((2, 4, 4, 4), np.float32), q, 100.0, 4)
    with pytest.raises(ValueError, match="float32 or float16"):
        D.paint_field(disp.astype(np.float64), q, 100.0, 4)
    for w in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="worder"):
            D.paint_field(disp, q, 100.0, 4, worder=w)
        with pytest.raises(ValueError, match="worder"):
            D.paint_field(None, q, 100.0, 4, worder=w)
    for r in (0, (4, 4), 4.0):
        with pytest.raises(ValueError, match="res"):
            D.paint_field(None, q, 100.0, r)
    for L in (0.0, float("inf"), (1.0, 2.0)):
        with pytest.raises(ValueError, match="boxsize"):
            D.paint_field(None, q, L, 4)
    for nm in ("Density", "sum", None, 0):
        with pytest.raises(ValueError, match="normalize"):
            D.paint_field(disp, q, 100.0, 4, normalize=nm)
    for fill in (float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError, match="fill"):
            D.paint_field(disp, q, 100.0, 4, fill=fill)


@pytest.mark.parametrize("call", ["paint_field", "paint_density"])
def test_line_of_sight_validation(call):
    disp = np.zeros((3, 4, 4, 4), np.float32)
    q = np.zeros((4, 4, 4), np.float32)
    v = np.zeros((3, 4, 4, 4), np.float32)
    fn = (lambda **kw: D.paint_field(disp, q, 100.0, 4, **kw)) if call == "paint_field" else \
        (lambda **kw: D.paint_density(disp, 100.0, 4, **kw))
    for los in (3, -1, 1.0, True, "z"):
        with pytest.raises(ValueError, match="los"):
            fn(velocity=v, los=los, velocity_to_length=1.0)
        with pytest.raises(ValueError, match="los"):
            fn(los=los)
    with pytest.raises(ValueError, match="velocity_to_length is required"):
        fn(velocity=v)
    for f in (float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="velocity_to_length"):
            fn(velocity=v, velocity_to_length=f)
    for bad in (np.zeros((2, 4, 4, 4), np.float32), np.zeros((3, 4, 4, 5), np.float32), np.zeros((4, 4), np.float32)):
        with pytest.raises(ValueError, match="velocity must have shape"):
            fn(velocity=bad, velocity_to_length=1.0)
    with pytest.raises(ValueError, match="velocity must be float32 or float16"):
        fn(velocity=v.astype(np.float64), velocity_to_length=1.0)
    with pytest.raises(ValueError, match="NumPy array"):
        fn(velocity=v.tolist(), velocity_to_length=1.0)


class _FakeCuda:
    """Stands in for a tensor on a device, for the mixed-kind checks, which read no data."""
    def __init__(self, shape, index):
        import torch
        self.shape, self.ndim, self.dtype, self.is_cuda = shape, len(shape), torch.float32, True
        self.device = torch.device("cuda", index)


def test_mixed_kinds_and_devices(monkeypatch):
    disp = np.zeros((3, 4, 4, 4), np.float32)
    q = np.zeros((4, 4, 4), np.float32)
    monkeypatch.setattr(D, "_is_torch", lambda x: isinstance(x, _FakeCuda))
    t0, t1 = _FakeCuda((3, 4, 4, 4), 0), _FakeCuda((3, 4, 4, 4), 1)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.paint_field(disp, t0, 100.0, 4)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.paint_field(t0, q, 100.0, 4)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.paint_field(t0, t1, 100.0, 4)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.paint_field(disp, q, 100.0, 4, velocity=t0, velocity_to_length=1.0)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.paint_density(t0, 100.0, 4, velocity=t1, velocity_to_length=1.0)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.paint_density(disp, 100.0, 4, velocity=t0, velocity_to_length=1.0)


def test_no_device_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        return                                                 # test_gpu_field.py covers the device
    q = np.zeros((4, 4, 4), np.float32)
    disp = np.zeros((3, 4, 4, 4), np.float32)
    with pytest.raises(_lib.NBEError, match="no HIP device|no CPU fallback"):
        D.paint_field(disp, q, 100.0, 4)
    with pytest.raises(_lib.NBEError):
        D.paint_field(None, q, 100.0, 4)
    with pytest.raises(_lib.NBEError):
        D.paint_density(disp, 100.0, 4, velocity=disp, velocity_to_length=0.01)


def test_rsd_factor():
    for z, Om in ((0.0, 0.3), (0.5, 0.3175), (3.0, 0.1)):
        f = D.rsd_factor(z, Om)
        assert isinstance(f, float)
        assert f == (1.0 + z) / float(cosmology.hubble_rate(z, Om))
        assert f == pytest.approx((1.0 + z) / (100.0 * np.sqrt(Om * (1.0 + z) ** 3 + 1.0 - Om)), rel=1e-6)
    assert D.rsd_factor(0.0, 0.3) == pytest.approx(0.01, rel=1e-7)       # H0 = 100 h km/s/Mpc
    for bad in (float("nan"), "0", True, None):
        with pytest.raises(ValueError):
            D.rsd_factor(bad, 0.3)


def test_symbols_are_bound():
    for name in ("nbe_quantity_range", "nbe_paint_fields", "nbe_mesh_to_field"):
        assert name in _lib.SIGNATURES


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def test_flags_parse_and_need_vel_and_density_res(tmp_path):
    ap = CLI.build_parser()
    base = _base_argv(tmp_path)
    plain = vars(ap.parse_args(base))
    assert "paint_vel" not in plain and "rsd" not in plain                     # absent unless given
    assert CLI.velocity_options(ap.parse_args(base)) == (False, None)
    assert CLI.velocity_options(argparse.Namespace()) == (False, None)
    ns = ap.parse_args(base + ["--density_res", "32", "--paint_vel", "--rsd", "1"])
    assert ns.paint_vel is True and ns.rsd == 1
    assert CLI.velocity_options(ns) == (True, 1)
    assert CLI.velocity_options(ap.parse_args(base + ["--density_res", "32", "--rsd", "0"])) == (False, 0)
    assert CLI.velocity_options(ap.parse_args(base + ["--density_res", "32", "--paint_vel"])) == (True, None)
    # density_options' dict is what it was
    assert CLI.density_options(ns) == dict(res=32, boxsize=1000.0, worder=2, deconvolve=True, pk=False)
    for flag in (["--paint_vel"], ["--rsd", "2"]):
        with pytest.raises(SystemExit, match="--density_res"):
            CLI.velocity_options(ap.parse_args(base + flag))
        with pytest.raises(SystemExit, match="needs --vel"):
            CLI.velocity_options(ap.parse_args(base + ["--density_res", "32", "--no-vel"] + flag))
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--density_res", "32", "--rsd", "3"])
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--density_res", "32", "--rsd"])
