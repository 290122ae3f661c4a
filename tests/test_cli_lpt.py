"""The input driver on the MI355X: python -m jax_nbody_emulator_with_dj_amd.lpt_input writes lpt_dis.npy, the module's own
result bit for bit, and run_emulator reads it as its --displacement_files."""

import numpy as np
import pytest

from lpt_ref import red_field
from test_cli_density import _sim

pytestmark = pytest.mark.gpu


def test_cli_writes_the_displacement_run_emulator_reads(tmp_path):
    from jax_nbody_emulator_with_dj_amd import lpt, lpt_input, run_emulator
    _, sim, _, _, argv = _sim(tmp_path)
    delta = np.float32(0.03) * red_field(8, 81, np.float32)
    np.save(sim / "delta.npy", delta)
    lpt_input.main(["--delta_files", str(sim / "delta.npy"), "--output_dirs", str(sim), "--npart", "16", "--boxsize", "500",
                    "--scale", "0.75", "--upsample_method", "fourier"])
    psi = np.load(sim / "lpt_dis.npy")
    assert psi.dtype == np.float32 and psi.shape == (3, 16, 16, 16)
    want = lpt.zeldovich_displacement(lpt.resize_density(delta, 16, boxsize=500.0, upsample_method="fourier"),
                                      boxsize=500.0, scale=0.75)
    assert np.array_equal(psi.view(np.uint32), want.view(np.uint32))

    argv[argv.index("--displacement_files") + 1] = str(sim / "lpt_dis.npy")
    run_emulator.main(argv)
    dis = np.load(sim / "emu_dis.npy")
    assert dis.shape == (3, 16, 16, 16) and np.isfinite(dis.astype(np.float32)).all()


def test_cli_mode_inject_reads_the_table_and_the_seed(tmp_path):
    from jax_nbody_emulator_with_dj_amd import lpt, lpt_input
    delta = red_field(8, 82, np.float32)
    k = np.geomspace(0.005, 0.05, 16)
    pk = 2.0e4 * (k / 0.1) ** -1.7
    np.save(tmp_path / "delta.npy", delta)
    np.savetxt(tmp_path / "pk.txt", np.column_stack([k, pk]), header="k_h_per_Mpc Pk_Mpc_over_h_cubed")
    lpt_input.main(["--delta_files", str(tmp_path / "delta.npy"), "--output_dirs", str(tmp_path), "--npart", "16",
                    "--upsample_method", "mode_inject", "--pk_table", str(tmp_path / "pk.txt"), "--seed", "9"])
    k2, pk2 = lpt_input.read_table(tmp_path / "pk.txt")
    want = lpt.zeldovich_displacement(lpt.resize_density(delta, 16, upsample_method="mode_inject", k_target=k2,
                                                         pk_target=pk2, seed=9))
    assert np.array_equal(np.load(tmp_path / "lpt_dis.npy").view(np.uint32), want.view(np.uint32))
