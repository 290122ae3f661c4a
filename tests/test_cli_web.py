"""The drivers of the cosmic web: `run_emulator --density_res N --cosmic_web`, `python -m ...halos
--halo_environment RES` and `run_emulator --fof --halo_environment RES`.  The parsers and their checks run on the CPU; on the
MI355X the three paths write, at 16^3 particles, files that are the module's own results bit for bit, and without the new
flags the files that were written before."""

import argparse

import numpy as np
import pytest

import fof_ref as F
from jax_nbody_emulator_with_dj_amd import halos as H, run_emulator as CLI

BASE = ["--displacement_file", "f.npy", "--output_dir", "d"]
RUN = ["--cosmo_param_files", __file__, "--displacement_files", __file__, "--output_dirs", ".", "--ndiv", "1"]
ENV_KEYS = ["Length", "count", "delta_s", "eigenvalues", "smoothing", "threshold", "web_type"]
WEB_KEYS = ["counts", "mass_fraction", "smoothing", "thresholds", "volume_fraction"]


def die(msg):
    raise SystemExit(msg)


def test_halos_parser_round_trips():
    a = H.build_parser().parse_args(BASE)
    assert (a.halo_environment, a.web_smoothing, a.web_threshold) == (None, None, None)
    assert H.environment_options(a, 1000.0, pytest.fail) is None
    a = H.build_parser().parse_args(BASE + ["--halo_environment", "64"])
    assert H.environment_options(a, 1000.0, pytest.fail, a.mas_worder) == dict(res=64, worder=2, smoothing=31.25, threshold=0.0)
    a = H.build_parser().parse_args(BASE + ["--halo_environment", "64", "--web_smoothing", "8", "--web_threshold", "0.2",
                                            "--mas_worder", "4"])
    assert H.environment_options(a, 1000.0, pytest.fail, a.mas_worder) == dict(res=64, worder=4, smoothing=8.0, threshold=0.2)
    for extra, match in ((["--web_smoothing", "8"], "--web_smoothing needs --halo_environment"),
                         (["--web_threshold", "0.1"], "--web_threshold needs --halo_environment"),
                         (["--halo_environment", "1"], "must be in 2 .. 2048"),
                         (["--halo_environment", "4096"], "must be in 2 .. 2048"),
                         (["--halo_environment", "16", "--web_smoothing", "0"], "--web_smoothing must be positive"),
                         (["--halo_environment", "16", "--web_smoothing", "nan"], "--web_smoothing must be positive"),
                         (["--halo_environment", "16", "--web_threshold", "inf"], "finite")):
        with pytest.raises(SystemExit, match=match):
            H.environment_options(H.build_parser().parse_args(BASE + extra), 1000.0, die)
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(BASE + ["--halo_environment", "16", "--web_threshold", "0", "1"])      # one threshold here
    with pytest.raises(SystemExit, match="--web_smoothing needs --halo_environment"):
        H.main(BASE + ["--web_smoothing", "3"])                                 # before it reads a file


def test_run_emulator_parser_round_trips():
    ap = CLI.build_parser()
    ns = ap.parse_args(RUN)
    for name in ("cosmic_web", "halo_environment", "web_smoothing", "web_threshold"):
        assert not hasattr(ns, name)                                                # absent unless given
    assert CLI.cosmic_web_options(ns) is None and CLI.halo_environment_options(ns) is None
    assert CLI.cosmic_web_options(argparse.Namespace()) is None and CLI.halo_environment_options(argparse.Namespace()) is None
    ns = ap.parse_args(RUN + ["--density_res", "32", "--cosmic_web", "--boxsize", "256"])
    assert CLI.cosmic_web_options(ns) == dict(smoothing=16.0, thresholds=[0.0])
    assert CLI.density_options(ns) == dict(res=32, boxsize=256.0, worder=2, deconvolve=True, pk=False)
    ns = ap.parse_args(RUN + ["--density_res", "32", "--cosmic_web", "--web_smoothing", "5", "--web_threshold", "0", "0.2", "0.4"])
    assert CLI.cosmic_web_options(ns) == dict(smoothing=5.0, thresholds=[0.0, 0.2, 0.4])
    ns = ap.parse_args(RUN + ["--fof", "--halo_environment", "32", "--web_threshold", "0.3", "0.5", "--mas_worder", "3",
                              "--density_res", "16", "--cosmic_web"])
    assert CLI.halo_environment_options(ns) == dict(res=32, worder=3, smoothing=62.5, threshold=0.3)
    assert CLI.cosmic_web_options(ns) == dict(smoothing=125.0, thresholds=[0.3, 0.5])
    for extra, check in ((["--cosmic_web"], CLI.cosmic_web_options),                             # needs --density_res
                         (["--density_res", "4096", "--cosmic_web"], CLI.cosmic_web_options),
                         (["--density_res", "16", "--cosmic_web", "--web_smoothing", "-1"], CLI.cosmic_web_options),
                         (["--density_res", "16", "--cosmic_web", "--web_threshold"] + ["0"] * 65, CLI.cosmic_web_options),
                         (["--halo_environment", "16"], CLI.halo_environment_options),             # needs --fof
                         (["--fof", "--halo_environment", "1"], CLI.halo_environment_options),
                         (["--fof", "--web_smoothing", "4"], CLI.halo_environment_options),       # no consumer
                         (["--density_res", "16", "--web_threshold", "0.1"], CLI.halo_environment_options)):
        with pytest.raises(SystemExit):
            check(ap.parse_args(RUN + extra))
    with pytest.raises(SystemExit):
        ap.parse_args(RUN + ["--density_res", "16", "--cosmic_web", "--web_threshold"])           # no value


@pytest.mark.gpu
def test_run_emulator_writes_the_web_and_nothing_else_changes(tmp_path):
    from jax_nbody_emulator_with_dj_amd.web import cosmic_web
    from test_cli_density import _sim
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    _, plain, _, _, argv_plain = _sim(tmp_path / "a")
    _, sim, _, _, argv = _sim(tmp_path / "b")
    CLI.main(argv_plain + ["--density_res", "16", "--boxsize", "250", "--pk"])
    before = ["dis.npy", "emu_delta.npy", "emu_dis.npy", "emu_pk.npz", "emu_vel.npy", "params.npy"]
    assert sorted(f.name for f in plain.iterdir()) == before
    CLI.main(argv + ["--density_res", "16", "--boxsize", "250", "--pk", "--cosmic_web", "--web_smoothing", "30",
                     "--web_threshold", "0", "0.05", "0.2"])
    assert sorted(f.name for f in sim.iterdir()) == sorted(before + ["emu_web.npz", "emu_web_type.npy"])
    for name in before:
        if name.endswith(".npy"):
            assert (plain / name).read_bytes() == (sim / name).read_bytes(), name
        else:                                              # an .npz carries the time it was written
            x, y = np.load(plain / name), np.load(sim / name)
            assert x.files == y.files and all(x[k].tobytes() == y[k].tobytes() and x[k].dtype == y[k].dtype for k in x.files)
    delta = np.load(sim / "emu_delta.npy")
    want = cosmic_web(delta, 250.0, 30.0, threshold=[0.0, 0.05, 0.2], mass=delta)
    types, web = np.load(sim / "emu_web_type.npy"), np.load(sim / "emu_web.npz")
    assert types.dtype == np.uint8 and types.shape == (16, 16, 16) and np.array_equal(types, want["types"])
    assert sorted(web.files) == WEB_KEYS
    assert web["counts"].dtype == np.int64 and np.array_equal(web["counts"], want["counts"])
    assert web["counts"][:, :4].sum(1).tolist() == [16 ** 3] * 3 and len(set(types.ravel().tolist())) >= 3
    assert web["thresholds"].dtype == np.float32 and np.array_equal(web["thresholds"], want["thresholds"])
    for key in ("volume_fraction", "mass_fraction"):
        assert web[key].dtype == np.float64 and web[key].shape == (3, 4) and np.array_equal(web[key], want[key])
    assert float(web["smoothing"]) == 30.0


@pytest.mark.gpu
def test_halo_environment_files_equal_the_api(tmp_path, capsys):
    import torch
    from jax_nbody_emulator_with_dj_amd.density import paint_density
    psi = F.clustered_field(16)
    np.save(tmp_path / "dis.npy", psi)
    args = ["--displacement_file", str(tmp_path / "dis.npy"), "--output_dir", str(tmp_path / "out"), "--boxsize", "100",
            "--nmin", "1", "--halo_environment", "16", "--web_smoothing", "12", "--web_threshold", "0.1", "--mas_worder", "3"]
    H.main(args)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["fof_catalog.npz", "halo_environment.npz"]
    cat = H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=1)
    delta = paint_density(psi, boxsize=100.0, res=16, worder=3, deconvolve=True)
    want = H.halo_environment(cat, delta, 100.0, 12.0, threshold=0.1, worder=1)
    got = np.load(tmp_path / "out" / "halo_environment.npz")
    assert sorted(got.files) == ENV_KEYS
    assert got["eigenvalues"].dtype == np.float32 and got["eigenvalues"].shape == (len(cat["Length"]), 3)
    for key in ("eigenvalues", "delta_s", "web_type", "Length"):
        assert np.array_equal(got[key], want[key]), key
    assert got["web_type"].dtype == np.uint8 and int(got["count"]) == len(cat["Length"]) > 10
    assert float(got["smoothing"]) == 12.0 and got["threshold"] == np.float32(0.1)
    e = got["eigenvalues"]
    assert (e[:, 0] >= e[:, 1]).all() and (e[:, 1] >= e[:, 2]).all()
    assert np.array_equal(got["web_type"], (e > np.float32(0.1)).sum(1))
    # the catalogue file is what a run without the flag writes
    H.main(args[:3] + [str(tmp_path / "plain")] + args[4:8])
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["fof_catalog.npz"]
    x, y = np.load(tmp_path / "plain" / "fof_catalog.npz"), np.load(tmp_path / "out" / "fof_catalog.npz")
    assert x.files == y.files and all(x[k].tobytes() == y[k].tobytes() and x[k].dtype == y[k].dtype for k in x.files)
    # run_emulator's step on the device field: the same arrays; without the option, the keys as before
    fof = dict(boxsize=100.0, linking_length=0.2, nmin=1)
    env = dict(res=16, worder=3, smoothing=12.0, threshold=0.1)
    extra = CLI.fof_catalog(torch.from_numpy(psi).cuda(), fof, 0.3175, env=env)
    assert sorted(extra) == ["fof", "halo_environment"]
    for key in got.files:
        assert np.array_equal(extra["halo_environment"][key], got[key]), key
    assert sorted(CLI.fof_catalog(torch.from_numpy(psi).cuda(), fof, 0.3175)) == ["fof"]
    # a catalogue without a halo: one line, no file
    capsys.readouterr()
    H.main(args[:3] + [str(tmp_path / "none")] + args[4:6] + ["--nmin", "100000"] + args[8:])
    assert "no halo in the catalogue: halo_environment.npz is not written" in capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "none").iterdir()) == ["fof_catalog.npz"]
