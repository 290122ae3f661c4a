"""Batch driver on the MI355X: --pk_multipoles and --pk_wedges write emu_pk_rsd_multipoles.npz and emu_pk_rsd_wedges.npz
whose arrays equal the public calls on the emu_delta_rsd.npy the run saved; without them the file list is what it was."""

import numpy as np
import pytest

from jax_nbody_emulator_with_dj_amd import run_emulator as CLI

pytestmark = pytest.mark.gpu

FLAGS = ["--vel", "--density_res", "32", "--rsd", "1", "--pk"]
BEFORE = ["dis.npy", "emu_delta.npy", "emu_delta_rsd.npy", "emu_dis.npy", "emu_pk.npz", "emu_pk_rsd.npz", "emu_vel.npy",
          "params.npy"]


def test_cli_writes_multipoles_and_wedges(tmp_path):
    from jax_nbody_emulator_with_dj_amd.density import power_spectrum_multipoles, power_spectrum_wedges
    from test_cli_density import _sim
    _, sim, _, _, argv = _sim(tmp_path)
    CLI.main(argv + FLAGS + ["--pk_multipoles", "--pk_wedges", "4"])
    assert sorted(f.name for f in sim.iterdir()) == sorted(BEFORE + ["emu_pk_rsd_multipoles.npz", "emu_pk_rsd_wedges.npz"])
    delta = np.load(sim / "emu_delta_rsd.npy")
    assert delta.dtype == np.float32 and delta.shape == (32, 32, 32)
    for name, want in (("emu_pk_rsd_multipoles.npz", power_spectrum_multipoles(delta, 1000.0, los=1)),
                       ("emu_pk_rsd_wedges.npz", power_spectrum_wedges(delta, 1000.0, los=1, nmu=4))):
        got = np.load(sim / name)
        assert sorted(got.files) == sorted(want)
        for key in want:
            np.testing.assert_array_equal(got[key], want[key], err_msg="%s %s" % (name, key))
    mp, wd = np.load(sim / "emu_pk_rsd_multipoles.npz"), np.load(sim / "emu_pk_rsd_wedges.npz")
    assert mp["p2"].shape == (16,) and wd["pk"].shape == (4, 16) and np.isfinite(mp["p2"]).all()
    pk = np.load(sim / "emu_pk_rsd.npz")
    assert np.array_equal(pk["pk"], mp["p0"]) and np.array_equal(pk["k"], mp["k"])
    # about another axis the same field gives another quadrupole: the flag's axis is the one that was used
    assert not np.array_equal(power_spectrum_multipoles(delta, 1000.0, los=0)["p2"], mp["p2"])


def test_cli_without_the_flags_writes_what_it_wrote(tmp_path):
    from test_cli_density import _sim
    _, sim, _, _, argv = _sim(tmp_path)
    CLI.main(argv + FLAGS)
    assert sorted(f.name for f in sim.iterdir()) == BEFORE
