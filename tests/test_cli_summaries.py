"""Batch driver: --bispectrum and --onepoint.  The flags parse, need --density_res and leave density_options' dict as it
was (no GPU); on the MI355X they write emu_bispectrum.npz and emu_onepoint.npz whose contents equal direct calls, and
without them the file list is what it was."""

import argparse

import numpy as np
import pytest

from jax_nbody_emulator_with_dj_amd import run_emulator as CLI

BK_KEYS = ("theta", "k3", "B", "Q", "ntriangles", "pk", "k", "nmodes")
ONEPOINT_KEYS = ("mean", "std", "skewness", "kurtosis_excess", "edges", "centers", "counts", "pdf", "outside", "nonfinite")


def test_flags_parse_and_need_density_res(tmp_path):
    from test_density_host import _base_argv
    ap = CLI.build_parser()
    base = _base_argv(tmp_path)
    plain = vars(ap.parse_args(base))
    assert "bispectrum" not in plain and "onepoint" not in plain                # absent unless given
    assert CLI.summary_options(ap.parse_args(base)) == (False, False)
    assert CLI.summary_options(argparse.Namespace()) == (False, False)
    ns = ap.parse_args(base + ["--density_res", "32", "--bispectrum", "--onepoint"])
    assert ns.bispectrum is True and ns.onepoint is True
    assert CLI.summary_options(ns) == (True, True)
    assert CLI.summary_options(ap.parse_args(base + ["--density_res", "32", "--onepoint"])) == (False, True)
    # density_options' dict is what it was
    assert CLI.density_options(ns) == dict(res=32, boxsize=1000.0, worder=2, deconvolve=True, pk=False)
    for flag in ("--bispectrum", "--onepoint"):
        with pytest.raises(SystemExit, match="--density_res"):
            CLI.summary_options(ap.parse_args(base + [flag]))
    assert CLI.BISPECTRUM_CONFIGS == ((0.1, 0.1), (0.05, 0.1)) and CLI.ONEPOINT_BINS == 120


def test_bispectrum_that_cannot_close_on_the_mesh_stops_before_any_work(tmp_path):
    from test_density_host import _base_argv
    # 1000 Mpc/h on 32^3: kappa = 15.9 for k = 0.1 h/Mpc, far beyond the mesh
    with pytest.raises(SystemExit, match="do not fit"):
        CLI.main(_base_argv(tmp_path) + ["--density_res", "32", "--bispectrum"])


@pytest.mark.gpu
@pytest.mark.parametrize("deconvolve", [True, False])
def test_cli_writes_bispectrum_and_onepoint(tmp_path, deconvolve):
    import torch
    from jax_nbody_emulator_with_dj_amd.density import bispectrum, field_pdf, field_statistics
    from test_cli_density import _sim
    p, sim, box, (Om, z), argv = _sim(tmp_path)
    extra = [] if deconvolve else ["--no-deconvolve", "--mas_worder", "3"]
    CLI.main(argv + ["--density_res", "32", "--boxsize", "250", "--bispectrum", "--onepoint"] + extra)
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_bispectrum.npz", "emu_delta.npy", "emu_dis.npy",
                                                     "emu_onepoint.npz", "emu_vel.npy", "params.npy"]
    delta = np.load(sim / "emu_delta.npy")
    bk = np.load(sim / "emu_bispectrum.npz")
    assert sorted(bk.files) == sorted("%s_cfg%d" % (k, i) for k in BK_KEYS for i in (1, 2))
    for i, (k1, k2) in enumerate(((0.1, 0.1), (0.05, 0.1)), 1):
        ref = bispectrum(delta, boxsize=250.0, k1=k1, k2=k2, theta=np.linspace(0, np.pi, 25),
                         mas_worder=None if deconvolve else 3)
        for key in BK_KEYS:
            np.testing.assert_array_equal(bk["%s_cfg%d" % (key, i)], ref[key])
        assert (ref["ntriangles"][:-1] > 0).all() and np.isfinite(ref["Q"][:-1]).all()
    op = np.load(sim / "emu_onepoint.npz")
    assert sorted(op.files) == sorted(ONEPOINT_KEYS)
    st = field_statistics(delta)
    for key in ("mean", "std", "skewness", "kurtosis_excess"):
        assert float(op[key]) == st[key]
    pdf = field_pdf(delta, float(delta.min()), float(delta.max()), 120)
    for key in ("edges", "centers", "counts", "pdf", "outside", "nonfinite"):
        np.testing.assert_array_equal(op[key], pdf[key])
    assert int(op["outside"]) == 0 and int(op["counts"].sum()) == 32 ** 3
    want, _ = np.histogram(delta, bins=np.linspace(float(delta.min()), float(delta.max()), 121))
    np.testing.assert_array_equal(op["counts"], want)


@pytest.mark.gpu
def test_onepoint_of_a_constant_field_widens_like_numpy():
    import torch
    delta = torch.full((8, 8, 8), 0.25, device="cuda")
    _, op = CLI.density_summaries(delta, dict(boxsize=1000.0, res=8, worder=2, deconvolve=True), False, True)
    want, edges = np.histogram(np.full(512, 0.25, np.float32), bins=120)
    np.testing.assert_array_equal(op["edges"], np.linspace(-0.25, 0.75, 121))
    np.testing.assert_array_equal(op["counts"], want)
    assert op["std"] == 0.0 and op["skewness"] == 0.0


@pytest.mark.gpu
def test_cli_without_the_flags_writes_what_it_wrote(tmp_path):
    from test_cli_density import _sim
    _, sim, _, _, argv = _sim(tmp_path)
    CLI.main(argv + ["--density_res", "16", "--pk"])
    assert sorted(f.name for f in sim.iterdir()) == ["dis.npy", "emu_delta.npy", "emu_dis.npy", "emu_pk.npz",
                                                     "emu_vel.npy", "params.npy"]
