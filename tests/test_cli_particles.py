"""The two drivers on the MI355X: --halo_pk writes halo_delta.npy and halo_pk.npz from the catalogue and the displacement
of the run, --xcorr writes emu_xcorr.npz; without the flags, and without a halo, the file list is what it was."""

import numpy as np
import pytest

import fof_ref
from jax_nbody_emulator_with_dj_amd import halos as H
from jax_nbody_emulator_with_dj_amd import run_emulator as CLI

pytestmark = pytest.mark.gpu

HALO_KEYS = ["bias", "count", "k", "nmodes", "p_hh", "p_hm", "p_mm", "r", "shot_noise"]


def check_halo_files(out_dir, disp, L, res, worder, weight, nmin):
    from jax_nbody_emulator_with_dj_amd.density import cross_correlation, paint_density
    cat = H.fof_halos(disp, boxsize=L, linking_length=0.2, nmin=nmin)
    delta_h, info = H.paint_halos(cat, L, res=res, worder=worder, weight=weight)
    cc = cross_correlation(delta_h, paint_density(disp, L, res, worder), L)
    got = np.load(out_dir / "halo_delta.npy")
    assert got.dtype == np.float32 and got.shape == (res,) * 3
    np.testing.assert_array_equal(got, delta_h)
    pk = np.load(out_dir / "halo_pk.npz")
    assert sorted(pk.files) == HALO_KEYS
    for key, src in (("k", "k"), ("p_hh", "p_aa"), ("p_mm", "p_bb"), ("p_hm", "p_ab"), ("r", "r"), ("bias", "bias"),
                     ("nmodes", "nmodes")):
        assert pk[key].dtype == np.float64 and pk[key].shape == (res // 2,)
        np.testing.assert_array_equal(pk[key], cc[src])
    assert pk["count"].dtype == np.int64 and int(pk["count"]) == info["count"] == len(cat["Length"])
    assert pk["shot_noise"].dtype == np.float64 and float(pk["shot_noise"]) == info["shot_noise"]


def test_halos_driver_writes_halo_spectra(tmp_path, capsys):
    psi = fof_ref.clustered_field(16, 100.0, 1)
    np.save(tmp_path / "dis.npy", psi)
    out = tmp_path / "out"
    base = ["--displacement_file", str(tmp_path / "dis.npy"), "--output_dir", str(out), "--boxsize", "100"]
    H.main(base)
    assert sorted(f.name for f in out.iterdir()) == ["fof_catalog.npz"]             # what it wrote before the flag
    H.main(base + ["--halo_pk", "16", "--mas_worder", "3", "--halo_weight", "length"])
    assert sorted(f.name for f in out.iterdir()) == ["fof_catalog.npz", "halo_delta.npy", "halo_pk.npz"]
    check_halo_files(out, psi, 100.0, 16, 3, "Length", 20)
    # no halo: no halo_* file, one line that says so, and no error
    empty = tmp_path / "empty"
    np.save(tmp_path / "zero.npy", np.zeros((3, 16, 16, 16), np.float32))
    capsys.readouterr()
    H.main(["--displacement_file", str(tmp_path / "zero.npy"), "--output_dir", str(empty), "--boxsize", "100",
            "--halo_pk", "16"])
    assert sorted(f.name for f in empty.iterdir()) == ["fof_catalog.npz"]
    lines = [l for l in capsys.readouterr().out.splitlines() if "no halo" in l]
    assert len(lines) == 1 and "halo_delta.npy" in lines[0]


def test_cli_writes_halo_spectra_and_the_cross_correlation(tmp_path):
    from jax_nbody_emulator_with_dj_amd.density import cross_correlation
    from test_cli_density import _sim
    p, sim, box, (Om, z), argv = _sim(tmp_path)
    CLI.main(argv + ["--density_res", "16", "--boxsize", "250", "--output-precision", "f32", "--fof", "--fof_nmin", "1",
                     "--halo_pk", "16"])
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_delta.npy", "emu_dis.npy", "emu_vel.npy",
                                                     "fof_catalog.npz", "halo_delta.npy", "halo_pk.npz", "params.npy"]
    check_halo_files(sim, np.load(sim / "emu_dis.npy"), 250.0, 16, 2, None, 1)
    # --xcorr of the field against itself: r = 1
    delta = np.load(sim / "emu_delta.npy")
    np.save(tmp_path / "target.npy", delta)
    CLI.main(argv + ["--density_res", "16", "--boxsize", "250", "--xcorr", str(tmp_path / "target.npy")])
    xc = np.load(sim / "emu_xcorr.npz")
    assert sorted(xc.files) == ["bias", "k", "nmodes", "p_aa", "p_ab", "p_bb", "r", "transfer"]
    assert all(xc[key].dtype == np.float64 and xc[key].shape == (8,) for key in xc.files)
    np.testing.assert_allclose(xc["r"], 1.0, rtol=0, atol=1e-12)
    np.testing.assert_allclose(xc["transfer"], 1.0, rtol=0, atol=1e-12)
    want = cross_correlation(delta, delta, 250.0)
    for key in xc.files:
        np.testing.assert_array_equal(xc[key], want[key])


def test_cli_without_a_halo_writes_no_halo_file(tmp_path, capsys):
    from test_cli_density import _sim
    _, sim, _, _, argv = _sim(tmp_path)
    CLI.main(argv + ["--boxsize", "250", "--fof", "--fof_nmin", "4096", "--halo_pk", "16"])
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_dis.npy", "emu_vel.npy", "fof_catalog.npz",
                                                     "params.npy"]
    assert sum("no halo" in l for l in capsys.readouterr().out.splitlines()) == 1
