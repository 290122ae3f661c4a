"""Particle catalogues (density.paint_particles, cross_correlation, shot_noise; halos.paint_halos, halo_bias) on the CPU: the
float64 reference against the lattice reference, the integer scheme's order independence on its NumPy restatement,
argument validation before any device work, the host arithmetic of r(k), bias and shot noise, and the new symbols."""

import ctypes

import numpy as np
import pytest

import field_ref as F
import mas_ref as R
import particles_ref as PR
from jax_nbody_emulator_with_dj_amd import _lib
from jax_nbody_emulator_with_dj_amd import density as D
from jax_nbody_emulator_with_dj_amd import halos as H
from jax_nbody_emulator_with_dj_amd import run_emulator as CLI
from test_density_host import _base_argv
from test_field_host import _FakeCuda


def _disp(n, L, seed):
    return (np.random.default_rng(seed).standard_normal((3, n, n, n)) * 1.7 * (L / n)).astype(np.float32)


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
@pytest.mark.parametrize("res", [6, 12, 20])
def test_reference_on_a_displaced_lattice_is_the_lattice_reference(worder, res):
    n, L = 12, 100.0
    disp = _disp(n, L, 3 + worder)
    num, mass, count, absq = PR.paint(PR.lattice_positions(disp, L), L, res, worder)
    want, _ = R.paint(disp, L, res, worder)
    assert num.shape == (0, res, res, res) and absq.shape == num.shape
    np.testing.assert_allclose(mass, want, rtol=0, atol=1e-12)
    assert mass.sum() == pytest.approx(n ** 3, rel=1e-12)
    # a quantity and a shift follow field_ref.paint of the same lattice
    q = np.random.default_rng(9).standard_normal((2, n, n, n)).astype(np.float32)
    v = np.random.default_rng(10).standard_normal((n, n, n)).astype(np.float32)
    got = PR.paint(PR.lattice_positions(disp, L), L, res, worder, quantity=q.reshape(2, -1), shift=(1, v.ravel(), 0.5))
    moved = disp.astype(np.float64)
    moved[1] += 0.5 * v
    ref = F.paint(moved, q, L, res, worder)
    np.testing.assert_allclose(got[0], ref[0], rtol=0, atol=1e-11)
    np.testing.assert_allclose(got[1], ref[1], rtol=0, atol=1e-12)


@pytest.mark.parametrize("worder", [1, 2, 3, 4])
def test_integer_scheme_does_not_depend_on_the_order(worder):
    rng = np.random.default_rng(20 + worder)
    L, res, count = 50.0, 10, 700
    pos = rng.uniform(-2 * L, 3 * L, (count, 3))
    q = rng.standard_normal((2, count)) * np.array([[1.0], [300.0]])
    v = rng.standard_normal(count)
    mass, S = PR.emulate(pos, L, res, worder, quantity=q, shift=(2, v, 0.25))
    assert int(mass.sum()) == count * 2 ** 22                               # every particle adds exactly its unit mass
    for seed in range(3):
        p = np.random.default_rng(seed).permutation(count)
        m2, S2 = PR.emulate(pos[p], L, res, worder, quantity=q[:, p], shift=(2, v[p], 0.25))
        assert np.array_equal(mass, m2) and np.array_equal(S, S2)
    # the integers meet the bound the GPU tests use
    num, ref, cnt, _ = PR.paint(pos, L, res, worder, quantity=q, shift=(2, v, 0.25))
    assert (np.abs(mass * 2.0 ** -22 - ref) <= 4 * 2.0 ** -22 * cnt + 1e-12).all()
    A, e = F.exponents(q[:, :, None, None])
    for c in range(2):
        err = np.abs(np.ldexp(S[c].astype(np.float64), int(e[c]) - 46) - num[c])
        assert (err <= F.numerator_bound(A[c], e[c], ref, cnt) + 1e-300).all()


def test_weights_ride_as_channel_zero():
    rng = np.random.default_rng(5)
    L, res, count = 50.0, 8, 300
    pos = rng.uniform(0, L, (count, 3))
    w = rng.uniform(0.0, 5.0, count)
    mass, S = PR.emulate(pos, L, res, 2, weights=w)
    V = np.rint(np.ldexp(w, 24 - int(F.exponents(w[None, :, None, None])[1][0]))).astype(np.int64)
    assert int(S[0].sum()) == int(V.sum()) * 2 ** 22                      # the total is exact: the mean is deterministic
    delta = PR.weighted_delta(S[0])
    num = PR.paint(pos, L, res, 2, weights=w)[0][0]
    np.testing.assert_allclose(delta, num * (res ** 3 / w.sum()) - 1.0, rtol=0, atol=2e-5)
    with pytest.raises(ValueError):
        PR.paint(pos, L, res, 2, weights=w, quantity=w)


# ---- argument validation: ValueError before any device work ---------------------------------------------------------

def test_names_are_public():
    for name in ("paint_particles", "cross_correlation", "shot_noise"):
        assert name in D.__all__ and callable(getattr(D, name))
    for name in ("paint_halos", "halo_bias"):
        assert name in H.__all__ and callable(getattr(H, name))


def test_paint_particles_validation():
    import torch
    pos = np.zeros((5, 3), np.float64)
    with pytest.raises(ValueError, match="empty"):
        D.paint_particles(np.zeros((0, 3), np.float32), 100.0, 4)
    for bad in (np.zeros((5, 2)), np.zeros((3, 5)), np.zeros(15), np.zeros((5, 3, 1))):
        with pytest.raises(ValueError, match=r"positions must have shape \(count, 3\)"):
            D.paint_particles(bad, 100.0, 4)
    for bad in (pos.astype(np.float16), pos.astype(np.int64)):
        with pytest.raises(ValueError, match="positions must be float32 or float64"):
            D.paint_particles(bad, 100.0, 4)
    with pytest.raises(ValueError, match="NumPy array"):
        D.paint_particles(pos.tolist(), 100.0, 4)
    with pytest.raises(ValueError, match="CUDA"):
        D.paint_particles(torch.zeros(5, 3), 100.0, 4)
    for w in (0, 5, 2.0, True):
        with pytest.raises(ValueError, match="worder"):
            D.paint_particles(pos, 100.0, 4, worder=w)
    for r in (0, (4, 4), 4.0):
        with pytest.raises(ValueError, match="res"):
            D.paint_particles(pos, 100.0, r)
    for L in (0.0, float("inf"), (1.0, 2.0)):
        with pytest.raises(ValueError, match="boxsize"):
            D.paint_particles(pos, L, 4)
    for s in ("yes", None, 1, 0):
        with pytest.raises(ValueError, match="sort"):
            D.paint_particles(pos, 100.0, 4, sort=s)
    # weights
    for bad in (np.ones(4), np.ones((5, 1)), np.ones((1, 5))):
        with pytest.raises(ValueError, match="weights must have shape"):
            D.paint_particles(pos, 100.0, 4, weights=bad)
    with pytest.raises(ValueError, match="weights must be float32 or float64"):
        D.paint_particles(pos, 100.0, 4, weights=np.ones(5, np.int64))
    for bad in (np.array([1, 1, -1e-30, 1, 1]), np.array([1, np.nan, 1, 1, 1]), np.array([1, np.inf, 1, 1, 1])):
        with pytest.raises(ValueError, match="finite and non-negative"):
            D.paint_particles(pos, 100.0, 4, weights=bad)
    with pytest.raises(ValueError, match="total weight is zero"):
        D.paint_particles(pos, 100.0, 4, weights=np.zeros(5))
    with pytest.raises(ValueError, match="weights together with a quantity"):
        D.paint_particles(pos, 100.0, 4, weights=np.ones(5), quantity=np.ones(5, np.float32))
    # quantity
    for bad in (np.ones(4, np.float32), np.ones((5, 5), np.float32)[:, :4], np.ones((0, 5), np.float32),
                np.ones((5, 5), np.float32), np.ones((2, 5, 1), np.float32)):
        with pytest.raises(ValueError, match="quantity must have shape"):
            D.paint_particles(pos, 100.0, 4, quantity=bad)
    with pytest.raises(ValueError, match="quantity must be float32 or float16"):
        D.paint_particles(pos, 100.0, 4, quantity=np.ones(5))
    for nm in ("Density", "sum", None, 0):
        with pytest.raises(ValueError, match="normalize"):
            D.paint_particles(pos, 100.0, 4, quantity=np.ones(5, np.float32), normalize=nm)
    for fill in (float("nan"), float("inf"), "0", None, True):
        with pytest.raises(ValueError, match="fill"):
            D.paint_particles(pos, 100.0, 4, quantity=np.ones(5, np.float32), fill=fill)
    # line of sight
    v = np.zeros((5, 3))
    for los in (3, -1, 1.0, True, "z"):
        with pytest.raises(ValueError, match="los"):
            D.paint_particles(pos, 100.0, 4, velocity=v, los=los, velocity_to_length=1.0)
    with pytest.raises(ValueError, match="velocity_to_length is required"):
        D.paint_particles(pos, 100.0, 4, velocity=v)
    for f in (float("nan"), float("inf"), "1", True):
        with pytest.raises(ValueError, match="velocity_to_length"):
            D.paint_particles(pos, 100.0, 4, velocity=v, velocity_to_length=f)
    for bad in (np.zeros((5, 2)), np.zeros(4), np.zeros((3, 5))):
        with pytest.raises(ValueError, match="velocity must have shape"):
            D.paint_particles(pos, 100.0, 4, velocity=bad, velocity_to_length=1.0)
    with pytest.raises(ValueError, match="velocity must be float32, float64 or float16"):
        D.paint_particles(pos, 100.0, 4, velocity=np.zeros(5, np.int32), velocity_to_length=1.0)


def test_mixed_kinds_and_devices(monkeypatch):
    import torch
    pos = np.zeros((5, 3), np.float32)
    monkeypatch.setattr(D, "_is_torch", lambda x: isinstance(x, _FakeCuda))
    t0, t1 = _FakeCuda((5, 3), 0), _FakeCuda((5, 3), 1)
    w0, w1 = _FakeCuda((5,), 0), _FakeCuda((5,), 1)
    for kw in (dict(weights=w0), dict(quantity=w0), dict(velocity=w0, velocity_to_length=1.0)):
        with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
            D.paint_particles(pos, 100.0, 4, **kw)
    for kw in (dict(weights=w1), dict(quantity=w1), dict(velocity=t1, velocity_to_length=1.0),
               dict(quantity=np.zeros(5, np.float32))):
        with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
            D.paint_particles(t0, 100.0, 4, **kw)
    a = np.zeros((4, 4, 4), np.float32)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.cross_correlation(a, _FakeCuda((4, 4, 4), 0), 100.0)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        D.cross_correlation(_FakeCuda((4, 4, 4), 0), _FakeCuda((4, 4, 4), 1), 100.0)


def test_cross_correlation_validation():
    a = np.zeros((4, 4, 4), np.float32)
    with pytest.raises(ValueError, match="two fields"):
        D.cross_correlation(a, None, 100.0)
    with pytest.raises(ValueError, match="cubic"):
        D.cross_correlation(np.zeros((4, 4, 5), np.float32), a, 100.0)
    with pytest.raises(ValueError, match="other must match"):
        D.cross_correlation(a, np.zeros((6, 6, 6), np.float32), 100.0)
    with pytest.raises(ValueError, match="other must match"):
        D.cross_correlation(a, a.astype(np.float64), 100.0)
    with pytest.raises(ValueError, match="float32"):
        D.cross_correlation(a.astype(np.float64), a, 100.0)
    with pytest.raises(ValueError, match="cubic box"):
        D.cross_correlation(a, a, (100.0, 100.0, 50.0))


def test_no_device_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        return                                                 # test_gpu_particles.py covers the device
    pos = np.zeros((5, 3), np.float32)
    with pytest.raises(_lib.NBEError, match="no HIP device|no CPU fallback"):
        D.paint_particles(pos, 100.0, 4)
    with pytest.raises(_lib.NBEError):
        D.paint_particles(pos, 100.0, 4, weights=np.ones(5))
    with pytest.raises(_lib.NBEError):
        D.cross_correlation(np.zeros((4, 4, 4), np.float32), np.zeros((4, 4, 4), np.float32), 100.0)


# ---- host arithmetic ---------------------------------------------------------------------------------------------------

def test_shot_noise():
    assert D.shot_noise(10.0, count=8) == 125.0
    assert D.shot_noise((2.0, 3.0, 4.0), count=6) == 4.0
    assert D.shot_noise(10.0, weights=np.ones(8)) == 125.0                 # equal weights: L^3 / count
    assert D.shot_noise(10.0, weights=[1.0, 1.0, 2.0]) == 1000.0 * 6.0 / 16.0
    assert D.shot_noise(10.0, weights=np.array([0, 3], np.int64)) == 1000.0
    assert isinstance(D.shot_noise(10.0, count=np.int64(3)), float)
    for kw in (dict(), dict(count=0), dict(count=2.0), dict(count=True), dict(weights=[]), dict(weights=[0.0, 0.0]),
               dict(weights=[1.0, -1.0]), dict(weights=[1.0, np.nan])):
        with pytest.raises(ValueError):
            D.shot_noise(10.0, **kw)
    with pytest.raises(ValueError, match="boxsize"):
        D.shot_noise(0.0, count=3)


def test_correlation_arrays_follow_from_the_spectra():
    k = np.array([0.1, 0.2, 0.3, 0.4])
    paa, pbb, pab = np.array([4.0, 9.0, 0.0, 1.0]), np.array([1.0, 4.0, 2.0, 0.0]), np.array([1.0, -3.0, 0.0, 0.0])
    nm = np.array([6.0, 18.0, 26.0, 30.0])
    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("error")                          # a zero denominator gives NaN without a warning
        cc = D.correlation_arrays(k, paa, pbb, pab, nm)
    assert sorted(cc) == ["bias", "k", "nmodes", "p_aa", "p_ab", "p_bb", "r", "transfer"]
    assert all(v.dtype == np.float64 and v.shape == (4,) for v in cc.values())
    for key, v in (("k", k), ("p_aa", paa), ("p_bb", pbb), ("p_ab", pab), ("nmodes", nm)):
        assert np.array_equal(cc[key], v)
    np.testing.assert_array_equal(cc["r"][:2], [0.5, -0.5])
    np.testing.assert_array_equal(cc["transfer"][:3], [2.0, 1.5, 0.0])
    np.testing.assert_array_equal(cc["bias"][:3], [1.0, -0.75, 0.0])
    assert np.isnan(cc["r"][2:]).all() and np.isnan(cc["transfer"][3]) and np.isnan(cc["bias"][3])


# ---- halos -------------------------------------------------------------------------------------------------------------

def _cat():
    return {"CMPosition": np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0], [7.0, 8.0, 9.0]]),
            "Length": np.array([50, 30, 20], np.int64), "label": np.array([3, 1, 7], np.int64)}


def test_paint_halos_validation():
    cat = _cat()
    with pytest.raises(ValueError, match="no halo is left"):
        H.paint_halos(cat, 100.0, 4, min_length=51)
    with pytest.raises(ValueError, match="no halo is left"):
        H.paint_halos(cat, 100.0, 4, max_length=19)
    with pytest.raises(ValueError, match="no halo is left"):
        H.paint_halos(cat, 100.0, 4, min_length=31, max_length=49)
    empty = {"CMPosition": np.zeros((0, 3)), "Length": np.zeros(0, np.int64)}
    with pytest.raises(ValueError, match="no halo is left"):
        H.paint_halos(empty, 100.0, 4)
    for w in ("length", "mass", 1):
        with pytest.raises(ValueError, match="weight"):
            H.paint_halos(cat, 100.0, 4, weight=w)
    with pytest.raises(ValueError, match="CMVelocity"):
        H.paint_halos(cat, 100.0, 4, redshift_space=True, velocity_to_length=1.0)
    with pytest.raises(ValueError, match="velocity_to_length is required"):
        H.paint_halos(dict(cat, CMVelocity=np.zeros((3, 3))), 100.0, 4, redshift_space=True)
    for bad in ("20", True, float("nan")):
        with pytest.raises(ValueError, match="min_length"):
            H.paint_halos(cat, 100.0, 4, min_length=bad)
    with pytest.raises(ValueError, match="fof_halos's dict"):
        H.paint_halos({"Length": cat["Length"]}, 100.0, 4)
    with pytest.raises(ValueError, match="mesh size from delta_m"):
        H.halo_bias(cat, np.zeros((4, 4, 4), np.float32), 100.0, res=4)
    with pytest.raises(ValueError, match="cubic"):
        H.halo_bias(cat, np.zeros((4, 4), np.float32), 100.0)
    # what is validated further down is paint_particles's
    with pytest.raises(ValueError, match="worder"):
        H.paint_halos(cat, 100.0, 4, worder=7)


# ---- symbols and flags ---------------------------------------------------------------------------------------------------

def test_symbols_are_bound_and_exported():
    for name in ("nbe_paint_particles", "nbe_particle_keys"):
        assert name in _lib.SIGNATURES
    l = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("nbe_paint_particles", "nbe_particle_keys", "nbe_quantity_range"):
        assert hasattr(l, name)


def test_flags_parse_and_need_their_parents(tmp_path):
    ap = CLI.build_parser()
    base = _base_argv(tmp_path)
    plain = vars(ap.parse_args(base))
    assert not {"halo_pk", "halo_weight", "xcorr"} & set(plain)               # absent unless given
    assert CLI.halo_options(ap.parse_args(base)) is None and CLI.xcorr_option(ap.parse_args(base)) is None
    ns = ap.parse_args(base + ["--fof", "--halo_pk", "32", "--mas_worder", "3", "--halo_weight", "length"])
    assert CLI.halo_options(ns) == dict(res=32, worder=3, weight="Length")
    assert CLI.halo_options(ap.parse_args(base + ["--fof", "--halo_pk", "16"])) == dict(res=16, worder=2, weight=None)
    assert CLI.fof_options(ns) == dict(boxsize=1000.0, linking_length=0.2, nmin=20)     # what it was
    with pytest.raises(SystemExit, match="needs --fof"):
        CLI.halo_options(ap.parse_args(base + ["--halo_pk", "16"]))
    with pytest.raises(SystemExit, match="needs --halo_pk"):
        CLI.halo_options(ap.parse_args(base + ["--fof", "--halo_weight", "length"]))
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--fof", "--halo_pk", "0"])
    with pytest.raises(SystemExit):
        ap.parse_args(base + ["--fof", "--halo_pk", "16", "--halo_weight", "mass"])
    target = tmp_path / "target.npy"
    np.save(target, np.zeros((8, 8, 8)))
    with pytest.raises(SystemExit, match="--density_res"):
        CLI.xcorr_option(ap.parse_args(base + ["--xcorr", str(target)]))
    with pytest.raises(SystemExit, match="expected"):
        CLI.xcorr_option(ap.parse_args(base + ["--density_res", "16", "--xcorr", str(target)]))
    got = CLI.xcorr_option(ap.parse_args(base + ["--density_res", "8", "--xcorr", str(target)]))
    assert got.dtype == np.float32 and got.shape == (8, 8, 8)
    hp = H.build_parser().parse_args(["--displacement_file", "x.npy", "--output_dir", "o", "--halo_pk", "24",
                                      "--halo_weight", "length", "--mas_worder", "4"])
    assert (hp.halo_pk, hp.halo_weight, hp.mas_worder) == (24, "length", 4)
    hp = H.build_parser().parse_args(["--displacement_file", "x.npy", "--output_dir", "o"])
    assert (hp.halo_pk, hp.halo_weight, hp.mas_worder) == (None, "number", 2)
