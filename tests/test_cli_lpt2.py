"""The second-order flags of the two input drivers on the MI355X: lpt_input --lpt2 and ic_input --lpt_order 2 write
lpt2_dis.npy, the module's own result bit for bit, beside an lpt_dis.npy that stays first order byte for byte."""

import json

import numpy as np
import pytest

from lpt_ref import red_field

pytestmark = pytest.mark.gpu

K = np.geomspace(0.003, 0.3, 24)
PK = 2.0e4 * (K / 0.1) ** -1.7


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_lpt_input_writes_both_orders(tmp_path):
    from jax_nbody_emulator_with_dj_amd import lpt, lpt_input
    delta = np.float32(0.03) * red_field(8, 81, np.float32)
    np.save(tmp_path / "delta.npy", delta)
    base = ["--delta_files", str(tmp_path / "delta.npy"), "--npart", "16", "--boxsize", "500", "--scale", "0.75",
            "--upsample_method", "fourier"]
    dirs = {}
    for name, flags in (("first", []), ("second", ["--lpt2"]), ("fine", ["--lpt2", "--growth2", "0.41", "--lpt2_dealias"])):
        dirs[name] = tmp_path / name
        dirs[name].mkdir()
        lpt_input.main(base + ["--output_dirs", str(dirs[name])] + flags)
    assert not (dirs["first"] / "lpt2_dis.npy").exists()
    first = (dirs["first"] / "lpt_dis.npy").read_bytes()
    assert (dirs["second"] / "lpt_dis.npy").read_bytes() == first and (dirs["fine"] / "lpt_dis.npy").read_bytes() == first
    resized = lpt.resize_density(delta, 16, boxsize=500.0, upsample_method="fourier")
    for name, kw in (("second", {}), ("fine", dict(growth2=0.41, dealias=True))):
        psi = np.load(dirs[name] / "lpt2_dis.npy")
        assert psi.dtype == np.float32 and psi.shape == (3, 16, 16, 16)
        assert same_bits(psi, lpt.lpt2_displacement(resized, boxsize=500.0, scale=0.75, **kw))
    assert not np.array_equal(np.load(dirs["second"] / "lpt2_dis.npy"), np.load(dirs["second"] / "lpt_dis.npy"))
    for bad in (["--growth2", "0.4"], ["--lpt2_dealias"], ["--lpt2", "--growth2", "nan"]):
        with pytest.raises(SystemExit):
            lpt_input.main(base + ["--output_dirs", str(dirs["first"])] + bad)
    with pytest.raises(SystemExit):
        lpt_input.main(base[:3] + ["15"] + base[4:] + ["--output_dirs", str(dirs["first"]), "--lpt2", "--lpt2_dealias"])


def test_ic_input_writes_both_orders_and_records_them(tmp_path):
    from jax_nbody_emulator_with_dj_amd import ic_input, lpt
    np.savetxt(tmp_path / "pk.txt", np.column_stack([K, PK]), header="k_h_per_Mpc Pk_Mpc_over_h_cubed")
    table = str(tmp_path / "pk.txt")
    k, pk = ic_input.read_table(table)
    base = ["--seeds", "7", "--npart", "16", "--pk_table", table, "--boxsize", "500", "--z", "1.0", "--omega_m", "0.3"]
    ic_input.main(base + ["--output_dirs", str(tmp_path / "first{seed}")])
    ic_input.main(base + ["--output_dirs", str(tmp_path / "second{seed}"), "--lpt_order", "2", "--lpt2_dealias"])
    ic_input.main(base + ["--output_dirs", str(tmp_path / "given{seed}"), "--lpt_order", "2", "--growth2", "0.5"])
    first, second, given = (tmp_path / (name + "7") for name in ("first", "second", "given"))
    assert not (first / "lpt2_dis.npy").exists()
    for name in ("lpt_dis.npy", "delta_linear.npy"):
        assert (second / name).read_bytes() == (first / name).read_bytes() == (given / name).read_bytes()
    scale, g = ic_input.growth_scale(1.0, 0.3), ic_input.growth2_of(1.0, 0.3)
    assert abs(g / (3.0 / 7.0) - 1.0) < 5e-3 and g != 3.0 / 7.0
    _, _, psi = lpt.linear_ics(16, 500.0, k, pk, 7, scale=scale, order=2, growth2=g, dealias=True)
    assert same_bits(np.load(second / "lpt2_dis.npy"), psi.cpu().numpy())
    _, _, psi = lpt.linear_ics(16, 500.0, k, pk, 7, scale=scale, order=2, growth2=0.5)
    assert same_bits(np.load(given / "lpt2_dis.npy"), psi.cpu().numpy())
    metas = [json.load(open(d / "ic_metadata.json")) for d in (first, second, given)]
    assert [(m["lpt_order"], m["growth2"]) for m in metas] == [(1, None), (2, g), (2, 0.5)]
    assert all(m["seed"] == 7 and m["scale"] == scale for m in metas)


def test_ic_input_second_order_of_a_white_noise_file(tmp_path):
    from jax_nbody_emulator_with_dj_amd import ic_input, lpt
    np.savetxt(tmp_path / "pk.txt", np.column_stack([K, PK]))
    white = np.random.default_rng(5).standard_normal((12, 12, 12)).astype(np.float32)
    np.save(tmp_path / "white.npy", white)
    out = tmp_path / "out"
    out.mkdir()
    ic_input.main(["--white_noise_file", str(tmp_path / "white.npy"), "--output_dirs", str(out), "--npart", "12",
                   "--pk_table", str(tmp_path / "pk.txt"), "--scale", "0.05", "--lpt_order", "2"])
    k, pk = ic_input.read_table(tmp_path / "pk.txt")
    delta = lpt.colour_noise(white, 1000.0, k, pk, scale=0.05)
    assert same_bits(np.load(out / "lpt_dis.npy"), lpt.zeldovich_displacement(delta, boxsize=1000.0))
    assert same_bits(np.load(out / "lpt2_dis.npy"), lpt.lpt2_displacement(delta, boxsize=1000.0))
    meta = json.load(open(out / "ic_metadata.json"))
    assert (meta["lpt_order"], meta["growth2"]) == (2, 3.0 / 7.0)
