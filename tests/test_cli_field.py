"""Batch driver on the MI355X: --paint_vel and --rsd write emu_vel_mesh.npy, emu_delta_rsd.npy and emu_pk_rsd.npz whose
contents equal direct calls on the fields the run saved; without them the file list is what it was."""

import numpy as np
import pytest

from jax_nbody_emulator_with_dj_amd import run_emulator as CLI

pytestmark = pytest.mark.gpu


def test_cli_writes_velocity_mesh_and_redshift_space_density(tmp_path):
    from jax_nbody_emulator_with_dj_amd.density import paint_density, paint_field, power_spectrum, rsd_factor
    from test_cli_density import _sim
    p, sim, box, (Om, z), argv = _sim(tmp_path)
    CLI.main(argv + ["--density_res", "16", "--boxsize", "250", "--mas_worder", "3", "--no-deconvolve", "--pk",
                     "--paint_vel", "--rsd", "1", "--output-precision", "f32"])
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_delta.npy", "emu_delta_rsd.npy", "emu_dis.npy",
                                                     "emu_pk.npz", "emu_pk_rsd.npz", "emu_vel.npy", "emu_vel_mesh.npy",
                                                     "params.npy"]
    d32, v32 = np.load(sim / "emu_dis.npy"), np.load(sim / "emu_vel.npy")      # float32: the fields that were painted
    assert d32.dtype == v32.dtype == np.float32
    vm = np.load(sim / "emu_vel_mesh.npy")
    assert vm.dtype == np.float32 and vm.shape == (3, 16, 16, 16)
    np.testing.assert_array_equal(vm, paint_field(d32, v32, 250.0, 16, 3))
    want = paint_density(d32, 250.0, 16, 3, deconvolve=False, velocity=v32, los=1, velocity_to_length=rsd_factor(z, Om))
    np.testing.assert_array_equal(np.load(sim / "emu_delta_rsd.npy"), want)
    assert not np.array_equal(np.load(sim / "emu_delta_rsd.npy"), np.load(sim / "emu_delta.npy"))
    pk = np.load(sim / "emu_pk_rsd.npz")
    k, P, nm = power_spectrum(want, 250.0)
    assert sorted(pk.files) == ["k", "nmodes", "pk"]
    np.testing.assert_array_equal(pk["k"], k)
    np.testing.assert_array_equal(pk["pk"], P)
    np.testing.assert_array_equal(pk["nmodes"], nm)


def test_cli_without_the_flags_writes_what_it_wrote(tmp_path):
    from test_cli_density import _sim
    _, sim, _, _, argv = _sim(tmp_path)
    CLI.main(argv + ["--density_res", "16", "--pk"])
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_delta.npy", "emu_dis.npy", "emu_pk.npz",
                                                     "emu_vel.npy", "params.npy"]
