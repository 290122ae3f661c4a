"""Batch driver with density fields on the MI355X: --density_res / --mas_worder / --pk write emu_delta.npy and emu_pk.npz
from the float32 displacement; without the flags no new file appears."""

import numpy as np
import pytest

from jax_nbody_emulator_with_dj_amd import run_emulator as R

pytestmark = pytest.mark.gpu


def _sim(tmp_path, style_seed=71):
    from oracle import params as P
    p = P.synthetic_params(seed=style_seed, mid_chan=8)
    np.savez(tmp_path / "weights.npz", params=p["params"])
    sim = tmp_path / "sim0"
    sim.mkdir()
    Om, z = 0.3, 0.5
    np.save(sim / "params.npy", np.array([Om, 0.05, 0.7, 0.96, 0.8, z]))
    box = np.random.default_rng(72).standard_normal((3, 16, 16, 16)).astype(np.float32) * 5
    np.save(sim / "dis.npy", box)
    argv = ["--cosmo_param_files", str(sim / "params.npy"), "--displacement_files", str(sim / "dis.npy"),
            "--output_dirs", str(sim), "--ndiv", "1", "--quiet", "--params", str(tmp_path / "weights.npz")]
    return p, sim, box, (Om, z), argv


def test_cli_writes_density_and_power_spectrum(tmp_path):
    import torch
    import jax_nbody_emulator_with_dj_amd as J
    from jax_nbody_emulator_with_dj_amd.density import paint_density, power_spectrum
    p, sim, box, (Om, z), argv = _sim(tmp_path)
    R.main(argv + ["--density_res", "16", "--mas_worder", "3", "--pk"])
    delta = np.load(sim / "emu_delta.npy")
    pk = np.load(sim / "emu_pk.npz")
    dis = np.load(sim / "emu_dis.npy")
    assert delta.dtype == np.float32 and delta.shape == (16, 16, 16)
    assert dis.dtype == np.float16 and dis.shape == (3, 16, 16, 16)
    assert sorted(pk.files) == ["k", "nmodes", "pk"]

    cfg = J.SubboxConfig(size=(16, 16, 16), ndiv=(1, 1, 1), output_dtype=np.float32)
    emu = J.create_emulator(load_params=False, processor_config=cfg, mid_chan=8)
    emu.processor.params = p
    d32, _ = emu.process_box(torch.from_numpy(box).cuda(), z, Om, show_progress=False)
    ref = paint_density(d32, 1000.0, 16, 3, deconvolve=True)
    np.testing.assert_allclose(delta, ref.cpu().numpy(), rtol=1e-6, atol=1e-6)
    k, P, nm = power_spectrum(ref, 1000.0)
    np.testing.assert_allclose(pk["k"], k, rtol=1e-12)
    np.testing.assert_allclose(pk["pk"], P, rtol=1e-5)
    assert np.array_equal(pk["nmodes"], nm)
    np.testing.assert_array_equal(dis, d32.cpu().numpy().astype(np.float16))


def test_cli_without_density_flags_writes_no_new_file(tmp_path):
    _, sim, _, _, argv = _sim(tmp_path)
    R.main(argv)
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_dis.npy", "emu_vel.npy", "params.npy"]
