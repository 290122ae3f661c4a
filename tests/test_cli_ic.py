"""The initial-conditions driver on the MI355X: python -m jax_nbody_emulator_with_dj_amd.ic_input writes lpt_dis.npy,
linear_ics's own result bit for bit, which run_emulator reads as its --displacement_files; the paired set and the
white-noise route."""

import json

import numpy as np
import pytest

from test_cli_density import _sim

pytestmark = pytest.mark.gpu

K = np.geomspace(0.003, 0.3, 24)
PK = 2.0e4 * (K / 0.1) ** -1.7


def _table(tmp_path):
    np.savetxt(tmp_path / "pk.txt", np.column_stack([K, PK]), header="k_h_per_Mpc Pk_Mpc_over_h_cubed")
    return str(tmp_path / "pk.txt")


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_cli_writes_what_linear_ics_gives_and_run_emulator_reads(tmp_path):
    from jax_nbody_emulator_with_dj_amd import ic_input, lpt, run_emulator
    _, sim, _, _, argv = _sim(tmp_path)
    table = _table(tmp_path)
    ic_input.main(["--seeds", "7", "--output_dirs", str(sim), "--npart", "16", "--pk_table", table, "--boxsize", "500",
                   "--scale", "0.05", "--paired"])
    k, pk = ic_input.read_table(table)
    for out_dir, invert in ((sim, False), (tmp_path / "sim0_paired", True)):
        assert sorted(p.name for p in out_dir.iterdir() if p.name.startswith(("lpt_", "delta_", "ic_"))) == \
            ["delta_linear.npy", "ic_metadata.json", "lpt_dis.npy"]
        delta, psi = lpt.linear_ics(16, 500.0, k, pk, 7, scale=0.05, invert_phase=invert)
        assert same_bits(np.load(out_dir / "lpt_dis.npy"), psi.cpu().numpy()) and psi.shape == (3, 16, 16, 16)
        assert same_bits(np.load(out_dir / "delta_linear.npy"), delta.cpu().numpy())
        meta = json.load(open(out_dir / "ic_metadata.json"))
        assert (meta["seed"], meta["n"], meta["boxsize"], meta["scale"], meta["fixed_amplitude"], meta["invert_phase"],
                meta["pk_table"]) == (7, 16, 500.0, 0.05, False, invert, table)
    assert np.array_equal(np.load(tmp_path / "sim0_paired" / "lpt_dis.npy"), -np.load(sim / "lpt_dis.npy"))

    argv[argv.index("--displacement_files") + 1] = str(sim / "lpt_dis.npy")
    run_emulator.main(argv)
    dis = np.load(sim / "emu_dis.npy")
    assert dis.shape == (3, 16, 16, 16) and np.isfinite(dis.astype(np.float32)).all()


def test_cli_seed_pattern_growth_scale_and_fixed_amplitude(tmp_path):
    from jax_nbody_emulator_with_dj_amd import ic_input, lpt
    table = _table(tmp_path)
    ic_input.main(["--seeds", "3:5", "--output_dirs", str(tmp_path / "s{seed}"), "--npart", "12", "--pk_table", table,
                   "--z", "1.0", "--omega_m", "0.3", "--fixed_amplitude", "--no-save-delta"])
    scale = ic_input.growth_scale(1.0, 0.3)
    for seed in (3, 4):
        out_dir = tmp_path / ("s%d" % seed)
        assert not (out_dir / "delta_linear.npy").exists() and not (tmp_path / ("s%d_paired" % seed)).exists()
        _, psi = lpt.linear_ics(12, 1000.0, K, PK, seed, scale=scale, fixed_amplitude=True, return_delta=False)
        assert same_bits(np.load(out_dir / "lpt_dis.npy"), psi.cpu().numpy())
        meta = json.load(open(out_dir / "ic_metadata.json"))
        assert meta["seed"] == seed and meta["fixed_amplitude"] is True and meta["scale"] == scale
    assert not (tmp_path / "s5").exists()


def test_cli_colours_a_white_noise_file(tmp_path):
    from jax_nbody_emulator_with_dj_amd import ic_input, lpt
    table = _table(tmp_path)
    white = np.random.default_rng(5).standard_normal((12, 12, 12)).astype(np.float32)
    np.save(tmp_path / "white.npy", white)
    out = tmp_path / "out"
    out.mkdir()
    ic_input.main(["--white_noise_file", str(tmp_path / "white.npy"), "--output_dirs", str(out), "--npart", "12",
                   "--pk_table", table, "--scale", "0.5"])
    k, pk = ic_input.read_table(table)
    delta = lpt.colour_noise(white, 1000.0, k, pk, scale=0.5)
    assert same_bits(np.load(out / "delta_linear.npy"), delta)
    assert same_bits(np.load(out / "lpt_dis.npy"), lpt.zeldovich_displacement(delta, boxsize=1000.0))
    meta = json.load(open(out / "ic_metadata.json"))
    assert meta["seed"] is None and meta["white_noise_file"] == str(tmp_path / "white.npy")
    with pytest.raises(SystemExit):
        ic_input.main(["--white_noise_file", str(tmp_path / "white.npy"), "--output_dirs", str(out), "--npart", "16",
                       "--pk_table", table])
