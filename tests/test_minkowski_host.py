"""Minkowski functionals (density.minkowski_functionals) on the CPU: the NumPy restatement against closed forms, the
functional formulas, argument validation before any device work, the missing-device error and the --minkowski flag."""

import argparse

import numpy as np
import pytest

import mf_ref as R
from jax_nbody_emulator_with_dj_amd import _lib
from jax_nbody_emulator_with_dj_amd import density as D
from jax_nbody_emulator_with_dj_amd import run_emulator as CLI

N = 12


def _mask(n=N):
    return np.zeros((n, n, n), bool)


def test_single_voxel():
    for at in ((0, 0, 0), (5, 7, 11), (N - 1, N - 1, N - 1)):
        m = _mask()
        m[at] = True
        assert R.element_counts(m) == (8, 12, 6, 1)


def test_block_closed_form():
    assert R.block_counts(3, 4, 5) == (120, 286, 227, 60)
    for (a, b, c), at in (((3, 4, 5), (2, 3, 1)), ((1, 6, 2), (0, 0, 0)), ((3, 4, 5), (10, 9, 8))):
        m = _mask()
        idx = np.ix_(*[(np.arange(s) + o) % N for s, o in zip((a, b, c), at)])   # the last one wraps across all axes
        m[idx] = True
        assert R.element_counts(m) == R.block_counts(a, b, c), (a, b, c, at)


def _euler(c):
    n0, n1, n2, n3 = c
    return n0 - n1 + n2 - n3


def test_hollow_shell_and_ring():
    m = _mask()
    m[2:7, 2:7, 2:7] = True
    m[3:6, 3:6, 3:6] = False
    assert _euler(R.element_counts(m)) == 2
    ring = _mask()
    ring[4, 2:7, 2:7] = True
    ring[4, 3:6, 3:6] = False
    assert _euler(R.element_counts(ring)) == 0


def test_full_empty_and_one_voxel_box():
    n3 = N ** 3
    assert R.element_counts(~_mask()) == (n3, 3 * n3, 3 * n3, n3)
    assert R.element_counts(_mask()) == (0, 0, 0, 0)
    assert R.element_counts(np.ones((1, 1, 1), bool)) == (1, 3, 3, 1)


@pytest.mark.parametrize("axis", [0, 1, 2])
@pytest.mark.parametrize("s", [1, 4, N - 1])
def test_slab_of_whole_planes(axis, s):
    m = _mask()
    sl = [slice(None)] * 3
    sl[axis] = slice(3, 3 + s) if 3 + s <= N else np.arange(3, 3 + s) % N
    m[tuple(sl)] = True
    assert R.element_counts(m) == R.slab_counts(s, N)


def test_thresholds_and_standardization_of_the_restatement():
    x = np.arange(N, dtype=np.float32)[:, None, None] * np.ones((1, N, N), np.float32)
    c = R.counts(x, [0.5, -0.5, N - 0.5, 3.5], standardize=False)
    assert [tuple(r) for r in c] == [R.slab_counts(N - 1, N), (N ** 3, 3 * N ** 3, 3 * N ** 3, N ** 3), (0, 0, 0, 0),
                                     R.slab_counts(N - 4, N)]
    np.testing.assert_array_equal(R.standardized(np.full((2, 2, 2), 5.0, np.float32), 5.0, 0.0), 0.0)


def test_functional_formulas():
    L, n = 100.0, 10
    c = np.array([R.block_counts(2, 3, 4), (0, 0, 0, 0)], np.int64)
    v0, v1, v2, v3 = D._mf_values(c, n, L)
    h = L / n
    n0, n1, n2, n3 = c[0]
    assert v0[0] == pytest.approx(h ** 3 * n3 / L ** 3, rel=1e-15)
    assert v1[0] == pytest.approx(h ** 2 * (-2 / 3 * n3 + 2 / 9 * n2) / L ** 3, rel=1e-15)
    assert v2[0] == pytest.approx(h * (2 / 3 * n3 - 4 / 9 * n2 + 2 / 9 * n1) / L ** 3, rel=1e-15)
    assert v3[0] == pytest.approx(1.0 / L ** 3, rel=1e-15)                     # a block has Euler characteristic 1
    assert v0[1] == v1[1] == v2[1] == v3[1] == 0.0
    for a, b in zip(D._mf_values(c, n, L), R.functionals(c, n, L)):
        np.testing.assert_allclose(a, b, rtol=1e-14)


# ---- argument validation: ValueError before any device work ---------------------------------------------------------

def test_validation():
    ok = np.zeros((4, 4, 4), np.float32)
    for bad in (np.zeros((4, 4, 8), np.float32), np.zeros((4, 4), np.float32), np.zeros((1, 4, 4, 4), np.float32),
                np.zeros((0, 0, 0), np.float32)):
        with pytest.raises(ValueError, match="cubic|mesh size"):
            D.minkowski_functionals(bad)
    for dt in (np.float64, np.float16, np.int32):
        with pytest.raises(ValueError, match="float32"):
            D.minkowski_functionals(ok.astype(dt))
    with pytest.raises(ValueError, match="NumPy array"):
        D.minkowski_functionals(ok.tolist())
    for t in ([0.0], [], np.zeros(1025), [0.0, np.nan], [0.0, np.inf], [0.0, 1e39], ["a", "b"]):
        with pytest.raises(ValueError, match="thresholds"):
            D.minkowski_functionals(ok, thresholds=t)
    for L in (0.0, -1.0, float("inf"), float("nan"), (1.0, 2.0), True):
        with pytest.raises(ValueError, match="boxsize"):
            D.minkowski_functionals(ok, boxsize=L)
    with pytest.raises(ValueError, match="cubic box"):
        D.minkowski_functionals(ok, boxsize=(100.0, 100.0, 200.0))
    import torch
    with pytest.raises(ValueError, match="CUDA"):
        D.minkowski_functionals(torch.zeros(4, 4, 4))
    assert D._mf_thresholds(None).dtype == np.float32 and D._mf_thresholds(None).size == 41
    t = D._mf_thresholds([[0.1, -2], [5, 5]])
    assert t.dtype == np.float32 and t.tolist() == [np.float32(0.1), -2.0, 5.0, 5.0]
    assert D._mf_thresholds(np.linspace(0, 1, 1024)).size == 1024


def test_no_device_means_loud_failure():
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    with pytest.raises(_lib.NBEError, match="no HIP device|no CPU fallback"):
        D.minkowski_functionals(np.zeros((4, 4, 4), np.float32))


def test_name_stays_out_of_the_package_namespace():
    import jax_nbody_emulator_with_dj_amd as J
    assert "minkowski_functionals" in D.__all__
    assert not hasattr(J, "minkowski_functionals") and "minkowski_functionals" not in J.__all__


# ---- CLI ---------------------------------------------------------------------------------------------------------------

def _base_argv(tmp_path):
    cos = tmp_path / "params.npy"
    np.save(cos, np.array([0.3, 0.05, 0.7, 0.96, 0.8, 0.5]))
    dis = tmp_path / "dis.npy"
    np.save(dis, np.zeros((3, 8, 8, 8), np.float32))
    return ["--cosmo_param_files", str(cos), "--displacement_files", str(dis), "--output_dirs", str(tmp_path),
            "--ndiv", "1"]


def test_cli_minkowski_flag(tmp_path):
    ap = CLI.build_parser()
    base = _base_argv(tmp_path)
    assert "minkowski" not in vars(ap.parse_args(base))                       # absent unless given
    ns = ap.parse_args(base + ["--density_res", "16", "--minkowski"])
    assert ns.minkowski is True and CLI.minkowski_option(ns) is True
    assert CLI.density_options(ns) == dict(res=16, boxsize=1000.0, worder=2, deconvolve=True, pk=False)
    assert CLI.minkowski_option(ap.parse_args(base + ["--density_res", "16"])) is False
    assert CLI.minkowski_option(ap.parse_args(base)) is False
    assert CLI.minkowski_option(argparse.Namespace()) is False
    with pytest.raises(SystemExit, match="--density_res"):
        CLI.minkowski_option(ap.parse_args(base + ["--minkowski"]))
