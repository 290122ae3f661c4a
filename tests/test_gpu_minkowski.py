"""Minkowski functionals on the MI355X (density.minkowski_functionals): exact element counts against the NumPy
restatement (mf_ref.py) fed the device's float32 mean and std, the float64 moments, reproducibility, residency, the
non-finite check, 64-bit indexing on a 1291^3 ramp and the batch driver's --minkowski."""

import numpy as np
import pytest

import mf_ref as R

pytestmark = pytest.mark.gpu

DEFAULT = np.linspace(-3, 3, 41, dtype=np.float32)


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


def _mf(*a, **k):
    from jax_nbody_emulator_with_dj_amd.density import minkowski_functionals
    return minkowski_functionals(*a, **k)


def smooth_field(n, seed, lognormal=True):
    """(n, n, n) float32: Gaussian-smoothed white noise (a few cells), exponentiated into a lognormal-like field."""
    rng = np.random.default_rng(seed)
    f = np.fft.rfftn(rng.standard_normal((n, n, n)))
    k2 = sum(np.meshgrid(np.fft.fftfreq(n) ** 2, np.fft.fftfreq(n) ** 2, np.fft.rfftfreq(n) ** 2, indexing="ij"))
    g = np.fft.irfftn(f * np.exp(-k2 * (2 * np.pi * 2.0) ** 2 / 2), s=(n, n, n), axes=(0, 1, 2))
    g /= g.std()
    return (np.exp(g) - 1.0 if lognormal else g).astype(np.float32)


def check(field, out, thresholds=DEFAULT, standardize=True, boxsize=1000.0):
    """The device result against the restatement with the device's moments, and the moments against float64 NumPy."""
    x = np.asarray(field, dtype=np.float32)
    n = x.shape[0]
    x64 = x.astype(np.float64)
    mean, std = x64.mean(), x64.std()
    assert abs(out["mean"] - mean) <= 1e-12 * (abs(mean) + std)
    assert abs(out["std"] - std) <= 1e-12 * (abs(mean) + std)
    ref = R.counts(x, thresholds, standardize, out["mean"], out["std"])
    assert out["counts"].dtype == np.int64 and out["counts"].shape == ref.shape
    np.testing.assert_array_equal(out["counts"], ref)
    for key, v in zip(("v0", "v1", "v2", "v3"), R.functionals(ref, n, boxsize)):
        assert out[key].dtype == np.float64
        np.testing.assert_allclose(out[key], v, rtol=1e-13, atol=0)
    np.testing.assert_array_equal(out["thresholds"], np.asarray(thresholds, np.float32).ravel().astype(np.float64))
    assert out["standardize"] is bool(standardize) and out["convention"] == "periodic_voxel_cubical_complex"
    assert isinstance(out["mean"], float) and isinstance(out["std"], float)


@pytest.mark.parametrize("n", [2, 3, 17, 48, 100, 128])
@pytest.mark.parametrize("standardize", [True, False])
def test_counts_match_the_restatement(n, standardize):
    x = smooth_field(n, n, lognormal=n >= 48) if n >= 17 else \
        np.random.default_rng(n).standard_normal((n, n, n)).astype(np.float32)
    check(x, _mf(x, boxsize=500.0, standardize=standardize), standardize=standardize, boxsize=500.0)


def test_threshold_sets():
    x = smooth_field(48, 5)
    t = np.array([0.5, -1.0, 2.0, 0.5, -3.0, 0.0, 2.0, 1e-3], np.float32)           # unsorted, duplicates
    check(x, _mf(x, thresholds=t), thresholds=t)
    t2 = np.array([0.25, -0.25], np.float32)
    check(x, _mf(x, thresholds=t2, standardize=False), thresholds=t2, standardize=False)
    t1024 = np.random.default_rng(6).uniform(-3.5, 3.5, 1024).astype(np.float32)
    t1024[::7] = t1024[3]
    check(x, _mf(x, thresholds=t1024), thresholds=t1024)


def test_constant_field():
    x = np.full((40, 40, 40), 1.5, np.float32)
    out = _mf(x)
    assert out["mean"] == 1.5 and out["std"] == 0.0
    check(x, out)                                                    # std 0: w = 0, counted where t <= 0
    n3 = 40 ** 3
    np.testing.assert_array_equal(out["counts"][DEFAULT <= 0], [[n3, 3 * n3, 3 * n3, n3]] * int((DEFAULT <= 0).sum()))
    assert (out["counts"][DEFAULT > 0] == 0).all()
    check(x, _mf(x, standardize=False), standardize=False)


def test_painted_delta():
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    from test_gpu_density import smooth_field as displacement
    disp = displacement((32, 32, 32), 1000.0, 1.5, 11)
    delta = paint_density(torch.from_numpy(disp).cuda(), 1000.0, 64, 2, deconvolve=True)
    out = _mf(delta, boxsize=1000.0)
    check(delta.cpu().numpy(), out)


def test_reproducible_and_resident():
    torch = _torch()
    x = smooth_field(128, 9)
    a = _mf(x)
    b = _mf(x)
    t = torch.from_numpy(x).cuda()
    c = _mf(t)
    for o in (b, c):
        for key in ("counts", "v0", "v1", "v2", "v3", "thresholds"):
            assert np.array_equal(a[key], o[key]), key
        assert a["mean"] == o["mean"] and a["std"] == o["std"]
    assert a["v3"].tobytes() == b["v3"].tobytes()


def test_non_finite_field_raises():
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    for bad in (np.nan, np.inf):
        x = smooth_field(17, 3)
        x[4, 16, 0] = bad
        for s in (True, False):
            with pytest.raises(NBEError, match="not finite"):
                _mf(x, standardize=s)


def test_ramp_1291_uses_64_bit_indices():
    torch = _torch()
    n = 1291                                                          # n^3 = 2.15e9 voxels > 2^31, 8.6 GB
    x = torch.arange(n, dtype=torch.float32, device="cuda").view(n, 1, 1).expand(n, n, n).contiguous()
    h = np.array([-1, 0, 1, 100, 645, 1289, 1290], np.int64)
    t = (h + 0.5).astype(np.float32)                                  # {w >= h + 1/2} = planes h + 1 .. n - 1
    out = _mf(x, boxsize=1000.0, thresholds=t, standardize=False)
    del x
    torch.cuda.empty_cache()
    n3 = n ** 3
    for hv, c in zip(h, out["counts"]):
        s = n - 1 - hv
        want = (n3, 3 * n3, 3 * n3, n3) if s == n else (0, 0, 0, 0) if s == 0 else R.slab_counts(s, n)
        assert tuple(int(v) for v in c) == want, (hv, c)
    assert out["mean"] == pytest.approx((n - 1) / 2.0, rel=1e-14)


def test_cli_writes_minkowski_functionals(tmp_path):
    from jax_nbody_emulator_with_dj_amd import run_emulator as CLI
    from test_cli_density import _sim
    p, sim, box, (Om, z), argv = _sim(tmp_path)
    CLI.main(argv + ["--density_res", "16", "--minkowski"])
    mf = np.load(sim / "emu_minkowski.npz")
    assert sorted(mf.files) == sorted(["thresholds", "v0", "v1", "v2", "v3", "counts", "mean", "std"])
    delta = np.load(sim / "emu_delta.npy")
    ref = _mf(delta, boxsize=1000.0)
    for key in mf.files:
        np.testing.assert_array_equal(mf[key], ref[key])
    check(delta, ref)
