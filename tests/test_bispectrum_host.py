"""Host-side checks of the bispectrum and one-point code: the two float64 restatements of bk_ref.py against each other
and against a closed form, the shell rules, argument validation before any device work, and field_pdf's edges and
normalisation against np.histogram.  No GPU."""

import numpy as np
import pytest

import bk_ref as R
from jax_nbody_emulator_with_dj_amd import _lib
from jax_nbody_emulator_with_dj_amd import density as D

THETA = np.linspace(0.0, np.pi, 25)


@pytest.mark.parametrize("n, k1, k2, dk, seed", [(32, 3.3, 6.1, 1.0, 1), (32, 5.0, 5.0, 1.0, 2), (24, 2.5, 4.0, 2.0, 3)])
def test_direct_and_fft_restatements_agree(n, k1, k2, dk, seed):
    x = R.quadratic_field(n, seed)
    s_d, c_d = R.direct(x, k1, k2, THETA, dk)
    s_f, c_f, A = R.fft_form(x, k1, k2, THETA, dk)
    assert np.abs(c_f - np.rint(c_f)).max() < 1e-3                    # float64 sums of n^3 terms: far from 1/2
    np.testing.assert_array_equal(np.rint(c_f).astype(np.int64), c_d)
    assert (np.abs(s_f - s_d) <= 1e-12 * A).all(), np.abs(s_f - s_d) / A
    assert c_d.max() > 0 and np.abs(s_d).max() > 0


def test_closed_form_three_cosines():
    n, L = 32, 1000.0
    a, b = np.array([3, 0, 0]), np.array([0, 5, 0])
    c = -(a + b)
    g = np.arange(n) * (2.0 * np.pi / n)
    X, Y, Z = np.meshgrid(g, g, g, indexing="ij")
    x = sum(np.cos(v[0] * X + v[1] * Y + v[2] * Z) for v in (a, b, c))
    # only (a, b, c) and (-a, -b, -c) carry amplitude n^3 / 2 each: the sum over the triangles is 2 (n^3 / 2)^3
    want = 2.0 * (n ** 3 / 2.0) ** 3
    assert want == 8796093022208.0
    th = np.array([np.pi / 2])
    s_d, c_d = R.direct(x, 3.0, 5.0, th, 1.0)
    assert c_d[0] == 6312
    assert abs(s_d[0] - want) <= 1e-9 * want
    s_f, c_f, _ = R.fft_form(x, 3.0, 5.0, th, 1.0)
    assert np.rint(c_f[0]) == 6312 and abs(s_f[0] - want) <= 1e-9 * want
    kF = 2.0 * np.pi / L
    out = R.bispectrum(x, L, 3.0 * kF, 5.0 * kF, th, 1.0)
    assert abs(out["B"][0] * out["ntriangles"][0] * float(n) ** 9 / L ** 6 - want) <= 1e-9 * want


def test_kappa3_at_0_half_pi_and_pi():
    for f in (R.kappa3, D.bispectrum_kappa3):
        k3 = f(3.0, 5.0, np.array([0.0, np.pi / 2, np.pi]))
        np.testing.assert_allclose(k3, [8.0, np.sqrt(34.0), 2.0], rtol=1e-15)
        assert f(5.0, 5.0, np.array([np.pi]))[0] < 1e-15 * 5 * 4     # k1 = k2, theta = pi: the third shell is empty


def test_shell_rules():
    n = 16
    # a shell whose edges are exact integer radii: |m|^2 = 9 is in, |m|^2 = 16 is out
    m = R.shell_modes(n, 3.5, 1.0)
    q = (m * m).sum(axis=1)
    assert set(q.tolist()) == {9, 10, 11, 12, 13, 14}                 # 15 is no sum of three squares; 16 is outside
    assert len(R.shell_modes(n, 4.5, 1.0)) and (R.shell_modes(n, 4.5, 1.0) ** 2).sum(axis=1).min() == 16
    lo2, hi2 = D.bispectrum_shell_bounds(np.array([3.5]), 1.0)
    assert (int(lo2[0]), int(hi2[0])) == (9, 16)
    mine = D._shell_modes(9, 16)
    assert mine.dtype == np.int32 and mine.shape[1] == 4 and (mine[:, 3] == 0).all()
    assert sorted(map(tuple, mine[:, :3])) == sorted(map(tuple, m))
    # the DC mode is in no shell, even where lo = 0
    m0 = R.shell_modes(n, 0.25, 1.0)                                  # lo = 0, hi = 0.75: nothing but the DC mode inside
    assert len(m0) == 0
    lo2, hi2 = D.bispectrum_shell_bounds(np.array([0.25, 0.5]), 1.0)
    assert list(lo2) == [1, 1] and list(hi2) == [1, 1]
    assert len(D._shell_modes(1, 1)) == 0
    m1 = R.shell_modes(n, 0.6, 1.0)                                   # [0.1, 1.1): the six |m| = 1 modes, not the DC mode
    assert len(m1) == 6 and ((m1 * m1).sum(axis=1) == 1).all()
    lo2, hi2 = D.bispectrum_shell_bounds(np.array([0.6]), 1.0)
    assert sorted(map(tuple, D._shell_modes(int(lo2[0]), int(hi2[0]))[:, :3])) == sorted(map(tuple, m1))
    # random shells: the device path's integer bounds select what the float64 rule selects
    rng = np.random.default_rng(0)
    for ka, dk in zip(rng.uniform(0.2, 6.5, 20), rng.uniform(0.3, 2.5, 20)):
        lo2, hi2 = D.bispectrum_shell_bounds(np.array([ka]), dk)
        got = D._shell_modes(int(lo2[0]), int(hi2[0]))
        assert sorted(map(tuple, got[:, :3])) == sorted(map(tuple, R.shell_modes(n, ka, dk)))


def test_validation_happens_before_any_device_work(monkeypatch):
    def touched():
        raise AssertionError("the library was touched before the arguments were validated")
    monkeypatch.setattr(_lib, "lib", touched)
    monkeypatch.setattr(D, "_device", touched)
    ok = np.zeros((32, 32, 32), np.float32)
    kF = 2.0 * np.pi / 1000.0
    kw = dict(boxsize=1000.0, k1=3 * kF, k2=5 * kF, theta=THETA, dk=1.0)

    def bad(match, field=ok, **over):
        with pytest.raises(ValueError, match=match):
            D.bispectrum(field, **{**kw, **over})

    bad("cubic", field=np.zeros((32, 32, 16), np.float32))
    bad("cubic", field=np.zeros((32, 32), np.float32))
    bad("float32", field=ok.astype(np.float64))
    bad("cubic box", boxsize=(1000.0, 1000.0, 500.0))
    bad("boxsize", boxsize=-1.0)
    bad("unsupported", field=np.zeros((2, 2, 2), np.float32))
    bad("theta", theta=[0.0, 3.2])
    bad("theta", theta=[-0.1])
    bad("theta", theta=[np.nan])
    bad("theta", theta=[])
    bad("theta", theta=np.zeros(257))
    bad("k1", k1=0.0)
    bad("k2", k2=-1.0)
    bad("dk", dk=0.0)
    bad("k1", k1=float("inf"))
    bad("worder", mas_worder=5)
    bad("worder", mas_worder=0)
    bad("modulo n", k1=7.5 * kF, k2=7.75 * kF)                       # 2 (7.5 + 7.75) + 1.5 = 32 = n
    bad("holds no mode", k1=0.2 * kF, dk=0.5)                         # [0, 0.45): only the DC mode
    bad("holds no mode", k2=1.2 * kF, dk=0.1)                         # [1.15, 1.25): no integer |m|^2 between
    with pytest.raises(ValueError, match="NumPy array"):
        D.bispectrum(ok.tolist(), **kw)
    import torch
    with pytest.raises(ValueError, match="CUDA"):
        D.bispectrum(torch.zeros(32, 32, 32), **kw)
    # one-point
    with pytest.raises(ValueError, match="3-D"):
        D.field_statistics(np.zeros((4, 4), np.float32))
    with pytest.raises(ValueError, match="float32"):
        D.field_statistics(np.zeros((4, 4, 4), np.float64))
    with pytest.raises(ValueError, match="3-D"):
        D.field_pdf(np.zeros((0, 4, 4), np.float32), 0.0, 1.0)
    for lo, hi, nb, match in ((1.0, 1.0, 10, "exceed"), (2.0, 1.0, 10, "exceed"), (0.0, 1.0, 1, "nbins"),
                              (0.0, 1.0, 4097, "nbins"), (0.0, 1.0, 2.5, "nbins"), (np.nan, 1.0, 4, "lo"),
                              (0.0, np.inf, 4, "hi"), (1.0, 1.0 + 2e-16, 8, "too close")):
        with pytest.raises(ValueError, match=match):
            D.field_pdf(ok, lo, hi, nb)


def test_no_device_means_loud_failure(monkeypatch):
    import torch
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    ok = np.zeros((32, 32, 32), np.float32)
    kF = 2.0 * np.pi / 1000.0
    with pytest.raises(_lib.NBEError, match="no HIP device|no CPU fallback"):
        D.bispectrum(ok, 1000.0, 3 * kF, 5 * kF, THETA)
    with pytest.raises(_lib.NBEError):
        D.field_statistics(ok)
    with pytest.raises(_lib.NBEError):
        D.field_pdf(ok, -1.0, 1.0, 8)


def test_shell_sum_units_never_overflow():
    for n in (4, 32, 1024, 2048):
        ka = np.array([0.3, 1.0, n / 8.0, n / 2.0 - 1.0, 0.87 * n])
        for dk in (0.1, 1.0, 8.0):
            lo2, hi2 = D.bispectrum_shell_bounds(ka, dk)
            par = D._bk_shell_params(n, lo2, hi2)
            assert (par[:, 2] ** 2 <= lo2).all() and ((par[:, 2] + 1) ** 2 > lo2).all()      # koff = floor(sqrt(lo2))
            assert (par[:, 3] >= 0).all() and (par[:, 3] <= 36).all()
            span = np.sqrt(hi2.astype(np.float64)) - par[:, 2]
            worst = np.minimum(float(n) ** 3, (2 * np.sqrt(hi2.astype(np.float64)) + 1) ** 3) * 2 * span * 2.0 ** par[:, 3]
            assert (worst < 2.0 ** 63).all()
    # the reference's configurations at 512^3 and 1024^3 keep the full 2^-36
    for n in (512, 1024):
        lo2, hi2 = D.bispectrum_shell_bounds(np.array([7.96, 15.92, 31.8]), 1.0)
        assert (D._bk_shell_params(n, lo2, hi2)[:, 3] == 36).all()


def test_pdf_edges_and_normalisation_match_numpy_histogram():
    rng = np.random.default_rng(5)
    x = rng.lognormal(size=20000).astype(np.float32) - 1.0
    for lo, hi, nb in ((-1.0, 8.0, 120), (0.0, 1.0, 2), (-0.37, 3.3, 4096)):
        edges = D.pdf_edges(lo, hi, nb)
        assert edges.dtype == np.float64
        np.testing.assert_array_equal(edges, np.linspace(lo, hi, nb + 1))
        counts, e2 = np.histogram(x[np.isfinite(x)], bins=edges)
        dens, _ = np.histogram(x[np.isfinite(x)], bins=edges, density=True)
        np.testing.assert_array_equal(D.pdf_from_counts(counts, edges), dens)
    assert np.isnan(D.pdf_from_counts(np.zeros(4, np.int64), D.pdf_edges(0.0, 1.0, 4))).all()


def test_names_stay_out_of_the_package_namespace():
    import jax_nbody_emulator_with_dj_amd as J
    for name in ("bispectrum", "field_statistics", "field_pdf"):
        assert name in D.__all__ and name not in J.__all__ and not hasattr(J, name)
