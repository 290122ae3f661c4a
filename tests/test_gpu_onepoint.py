"""One-point statistics on the MI355X (density.field_statistics, density.field_pdf): moments against float64 NumPy within
the rounding of float64 sums of n^3 terms, reproducibility, histogram counts equal to np.histogram's (inner edges, both
ends, outside, NaN, +-inf, a painted delta) and 64-bit indexing on a 1291^3 ramp."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U = 2.0 ** -53


def _torch():
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible device"
    return torch


def _D():
    from jax_nbody_emulator_with_dj_amd import density
    return density


def field(n, seed):
    rng = np.random.default_rng(seed)
    return (np.exp(0.8 * rng.standard_normal((n, n, n))) - 1.0).astype(np.float32)       # skewed, heavy-tailed


@pytest.mark.parametrize("n", [1, 3, 17, 100, 128])
def test_moments_against_float64_numpy(n):
    x = field(n, n)
    st = _D().field_statistics(x)
    assert set(st) == {"mean", "std", "skewness", "kurtosis_excess"} and all(type(v) is float for v in st.values())
    x64 = x.astype(np.float64)
    mean, std = x64.mean(), x64.std()
    dm = 1e-12 * (abs(mean) + std)                   # the tolerance tests/test_gpu_minkowski.py holds mean and std to
    assert abs(st["mean"] - mean) <= dm and abs(st["std"] - std) <= dm
    if n == 1:
        assert st == {"mean": float(x64[0, 0, 0]), "std": 0.0, "skewness": 0.0, "kurtosis_excess": 0.0}
        return
    d = x64 - mean
    m3, m4 = (d ** 3).mean(), (d ** 4).mean()
    skew, kurt = m3 / std ** 3, m4 / std ** 4 - 3.0
    # Condition of the central sums.  A float64 sum of N terms t_i added in runs of r terms and then in trees errs by at
    # most (r + log2 N + a few roundings per term) u sum |t_i|; r = 8 on the device at these sizes (runs of N / (256
    # ceil(N / 2048)) voxels), and NumPy adds pairwise in blocks of 8.
    # Both sides are allowed that.  A shift dm of the mean moves m3 by 3 m2 dm and m4 by 4 |m3| dm, and a shift dm of the
    # std moves m_p / std^p by p |m_p / std^p| dm / std.
    g = 2.0 * (8 + np.log2(x.size) + 8) * U
    tol3 = (g * np.abs(d ** 3).mean() + 3.0 * std ** 2 * dm) / std ** 3 + 3.0 * abs(skew) * dm / std
    tol4 = (g * m4 + 4.0 * abs(m3) * dm) / std ** 4 + 4.0 * (kurt + 3.0) * dm / std
    print("n %d: skewness off by %.3g (tol %.3g), kurtosis by %.3g (tol %.3g)"
          % (n, abs(st["skewness"] - skew), tol3, abs(st["kurtosis_excess"] - kurt), tol4))
    assert abs(st["skewness"] - skew) <= tol3
    assert abs(st["kurtosis_excess"] - kurt) <= tol4


def test_moments_shapes_constant_field_and_reproducibility():
    torch = _torch()
    D = _D()
    c = D.field_statistics(np.full((9, 20, 31), 2.5, np.float32))
    assert c == {"mean": 2.5, "std": 0.0, "skewness": 0.0, "kurtosis_excess": 0.0}
    x = field(96, 5)[:, :50, :77].copy()                                     # any 3-D shape
    a, b = D.field_statistics(x), D.field_statistics(x)
    t = D.field_statistics(torch.from_numpy(x).cuda())
    assert a == b == t
    x64 = x.astype(np.float64)
    assert abs(a["mean"] - x64.mean()) <= 1e-12 * (abs(x64.mean()) + x64.std())
    # the two-valued field +-1 has skewness 0 and excess kurtosis -2 exactly
    pm = np.ones((8, 8, 8), np.float32)
    pm[::2] = -1.0
    assert D.field_statistics(pm) == {"mean": 0.0, "std": 1.0, "skewness": 0.0, "kurtosis_excess": -2.0}


def check_pdf(x, lo, hi, nbins):
    out = _D().field_pdf(x, lo, hi, nbins)
    xs = np.asarray(x.cpu().numpy() if hasattr(x, "cpu") else x)
    fin = xs[np.isfinite(xs)]
    edges = np.linspace(lo, hi, nbins + 1)
    want, _ = np.histogram(fin, bins=edges)
    assert out["counts"].dtype == np.int64 and out["counts"].shape == (nbins,)
    np.testing.assert_array_equal(out["counts"], want)
    np.testing.assert_array_equal(out["edges"], edges)
    np.testing.assert_array_equal(out["centers"], 0.5 * (edges[:-1] + edges[1:]))
    assert out["nonfinite"] == xs.size - fin.size and type(out["nonfinite"]) is int
    assert out["outside"] == fin.size - int(want.sum()) and type(out["outside"]) is int
    if want.sum():
        dens, _ = np.histogram(fin, bins=edges, density=True)
        np.testing.assert_array_equal(out["pdf"], dens)
    else:
        assert np.isnan(out["pdf"]).all()
    return out


def test_pdf_of_a_painted_delta():
    torch = _torch()
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    from test_gpu_density import smooth_field as displacement
    disp = displacement((32, 32, 32), 1000.0, 6.0, 11)
    for deconvolve in (False, True):
        delta = paint_density(torch.from_numpy(disp).cuda(), 1000.0, 64, 2, deconvolve=deconvolve)
        lo, hi = (float(v) for v in torch.aminmax(delta))
        out = check_pdf(delta, lo, hi, 120)
        assert out["outside"] == 0 and out["counts"].sum() == 64 ** 3
        check_pdf(delta, -1.0, 8.0, 120)
        check_pdf(delta, -0.5, 0.5, 4096)


def test_pdf_values_on_edges_outside_and_non_finite():
    lo, hi, nbins = -1.0, 2.0, 30
    edges = np.linspace(lo, hi, nbins + 1)
    e32 = edges.astype(np.float32)
    near = np.concatenate([np.nextafter(e32, np.float32(-np.inf)), e32, np.nextafter(e32, np.float32(np.inf))])
    rng = np.random.default_rng(3)
    vals = np.concatenate([near, edges[3:9].astype(np.float32), [lo, hi, hi, lo - 1e-6, hi + 1e-6, -50.0, 1e30, -1e30],
                           [np.nan, np.nan, np.inf, -np.inf, -np.inf], rng.uniform(-1.5, 2.5, 4000)]).astype(np.float32)
    x = np.resize(vals, (17, 19, 23)).astype(np.float32)
    out = check_pdf(x, lo, hi, nbins)
    assert out["nonfinite"] >= 5 and out["outside"] >= 5
    # a bin width that is not a float32 number, many bins, and a field that is entirely outside or entirely non-finite
    check_pdf(x, -0.7, 1.9, 4096)
    check_pdf(x, 0.1, 0.1 + 1e-3, 7)
    assert check_pdf(np.full((4, 4, 4), 9.0, np.float32), 0.0, 1.0, 4)["outside"] == 64
    assert check_pdf(np.full((4, 4, 4), np.nan, np.float32), 0.0, 1.0, 4)["nonfinite"] == 64
    # a constant field inside one bin, and on the upper edge
    assert check_pdf(np.full((40, 40, 40), 0.5, np.float32), 0.0, 1.0, 4)["counts"][2] == 64000
    assert check_pdf(np.full((40, 40, 40), 1.0, np.float32), 0.0, 1.0, 4)["counts"][3] == 64000
    a = _D().field_pdf(x, lo, hi, nbins)
    assert a["counts"].tobytes() == out["counts"].tobytes() and a["pdf"].tobytes() == out["pdf"].tobytes()


def test_ramp_1291_uses_64_bit_indices():
    torch = _torch()
    D = _D()
    n = 1291                                                          # n^3 = 2.15e9 voxels > 2^31, 8.6 GB
    x = torch.arange(n, dtype=torch.float32, device="cuda").view(n, 1, 1).expand(n, n, n).contiguous()
    out = D.field_pdf(x, 0.0, float(n - 1), n - 1)                    # unit bins: plane i in bin i, the last two in the last
    st = D.field_statistics(x)
    del x
    torch.cuda.empty_cache()
    want = np.full(n - 1, n * n, np.int64)
    want[-1] *= 2
    np.testing.assert_array_equal(out["counts"], want)
    assert out["outside"] == 0 and out["nonfinite"] == 0
    assert st["mean"] == pytest.approx((n - 1) / 2.0, rel=1e-14)
    assert st["std"] == pytest.approx(np.sqrt((n * n - 1) / 12.0), rel=1e-13)
    # runs of n^3 / (2048 * 256) = 4104 terms: at most 4200 u mean |d|^3 / std^3 = 6e-13
    assert abs(st["skewness"]) < 1e-12
    assert st["kurtosis_excess"] == pytest.approx(-1.2 * (n * n + 1) / (n * n - 1), rel=1e-12)
