"""The drivers of the halo velocity moments: `python -m ...halos --velocity_file V --halo_vprofiles
--halo_v12` and `run_emulator --fof --vel --halo_vprofiles --halo_v12`.  The parsers and their checks run on the CPU; one case
on the MI355X writes halo_vprofiles.npz and halo_v12.npz."""

import numpy as np
import pytest

import fof_ref as F
from jax_nbody_emulator_with_dj_amd import halos as H, profiles as P, run_emulator as CLI

BASE = ["--displacement_file", "f.npy", "--output_dir", "d"]
RUN = ["--cosmo_param_files", __file__, "--displacement_files", __file__, "--output_dirs", ".", "--ndiv", "1"]
VPROFILE_KEYS = ["Length", "count", "counts", "exponent", "r_edges", "r_mid", "sigma_r", "sigma_t", "sums", "v_r"]
V12_KEYS = ["count", "exponent", "npairs", "r_edges", "r_mid", "sigma_r", "sigma_t", "sums", "v12"]


def die(msg):
    raise SystemExit(msg)


def test_halos_parser_round_trips():
    a = H.build_parser().parse_args(BASE)
    assert (a.velocity_file, a.halo_vprofiles, a.halo_v12) == (None, False, False)
    assert H.velocity_moment_options(a, 1000.0, False, pytest.fail) is None
    assert H.xi_options(a, 1000.0, pytest.fail) is None and H.profile_options(a, 1000.0, pytest.fail) is None
    a = H.build_parser().parse_args(BASE + ["--velocity_file", "v.npy", "--halo_vprofiles", "--halo_v12"])
    vm = H.velocity_moment_options(a, 1000.0, True, pytest.fail)
    assert np.array_equal(vm["vprofiles"], P.profile_edges(0.05, 5.0, 20)) and np.array_equal(vm["v12"], np.linspace(1.0, 50.0, 21))
    assert H.xi_options(a, 1000.0, pytest.fail) is None and H.profile_options(a, 1000.0, pytest.fail) is None
    # the edges come from the options of --halo_profiles and --halo_xi, with or without those flags
    a = H.build_parser().parse_args(BASE + ["--velocity_file", "v.npy", "--halo_vprofiles", "--profile_rmin", "0.5", "--profile_rmax", "20",
                                            "--profile_nbins", "12"])
    vm = H.velocity_moment_options(a, 1000.0, True, pytest.fail)
    assert np.array_equal(vm["vprofiles"], P.profile_edges(0.5, 20.0, 12)) and vm["v12"] is None
    assert H.profile_options(a, 1000.0, pytest.fail) is None
    a = H.build_parser().parse_args(BASE + ["--velocity_file", "v.npy", "--halo_v12", "--halo_xi", "--xi_rmin", "0.5", "--xi_rmax", "40",
                                            "--xi_nbins", "8", "--xi_log"])
    vm = H.velocity_moment_options(a, 1000.0, True, pytest.fail)
    assert vm["vprofiles"] is None and np.allclose(vm["v12"], np.geomspace(0.5, 40.0, 9), rtol=1e-15)
    assert np.array_equal(H.xi_options(a, 1000.0, pytest.fail)["r_edges"], vm["v12"])
    for extra, velocity, match in ((["--halo_vprofiles"], False, "--halo_vprofiles needs --velocity_file"),
                                   (["--halo_v12"], False, "--halo_v12 needs --velocity_file"),
                                   (["--halo_v12", "--xi_rmax", "400"], True, "must stay below L / 3"),
                                   (["--halo_v12", "--xi_nbins", "0"], True, "xi_nbins >= 1"),
                                   (["--halo_vprofiles", "--profile_rmax", "400"], True, "must stay below L / 3"),
                                   (["--halo_vprofiles", "--profile_nbins", "1"], True, "nbins must be an int >= 2")):
        with pytest.raises(SystemExit, match=match):
            H.velocity_moment_options(H.build_parser().parse_args(BASE + extra), 1000.0, velocity, die)
    # what belongs to --halo_profiles and --halo_xi alone still needs them
    for extra, check, match in ((["--halo_vprofiles", "--so_overdensity", "100"], H.profile_options, "--so_overdensity needs --halo_profiles"),
                                (["--halo_v12", "--xi_nmu", "4"], H.xi_options, "--xi_nmu needs --halo_xi"),
                                (["--profile_rmax", "4"], H.profile_options, "--profile_rmax needs --halo_profiles"),
                                (["--xi_rmax", "40"], H.xi_options, "--xi_rmax needs --halo_xi")):
        with pytest.raises(SystemExit, match=match):
            check(H.build_parser().parse_args(BASE + extra), 1000.0, die)


def test_halos_main_checks_its_prerequisites_before_it_reads_a_file():
    with pytest.raises(SystemExit, match="--halo_v12 needs --velocity_file"):
        H.main(BASE + ["--halo_v12"])
    with pytest.raises(SystemExit, match="--halo_vprofiles needs --velocity_file"):
        H.main(BASE + ["--halo_vprofiles", "--halo_v12"])
    with pytest.raises(SystemExit, match="--velocity_file needs --halo_vprofiles or --halo_v12"):
        H.main(BASE + ["--velocity_file", "v.npy"])


def test_run_emulator_parser_round_trips():
    ns = CLI.build_parser().parse_args(RUN)
    assert not hasattr(ns, "halo_vprofiles") and not hasattr(ns, "halo_v12")
    assert CLI.halo_velocity_options(ns) is None
    ns = CLI.build_parser().parse_args(RUN + ["--fof", "--halo_vprofiles", "--halo_v12", "--xi_nbins", "5", "--boxsize", "600"])
    vm = CLI.halo_velocity_options(ns)
    assert np.array_equal(vm["v12"], np.linspace(1.0, 50.0, 6)) and np.array_equal(vm["vprofiles"], P.profile_edges(0.05, 5.0, 20))
    assert CLI.halo_xi_options(ns) is None and CLI.halo_profile_options(ns) is None
    with pytest.raises(SystemExit):
        CLI.halo_velocity_options(CLI.build_parser().parse_args(RUN + ["--halo_v12"]))                          # needs --fof
    with pytest.raises(SystemExit):
        CLI.halo_velocity_options(CLI.build_parser().parse_args(RUN + ["--fof", "--no-vel", "--halo_vprofiles"]))  # needs --vel
    with pytest.raises(SystemExit):
        CLI.halo_velocity_options(CLI.build_parser().parse_args(RUN + ["--fof", "--halo_v12", "--boxsize", "120"]))  # 50 >= L / 3
    with pytest.raises(SystemExit):
        CLI.halo_xi_options(CLI.build_parser().parse_args(RUN + ["--fof", "--xi_nbins", "5"]))                  # as before


@pytest.mark.gpu
def test_the_files_equal_the_api(tmp_path, capsys):
    import torch
    psi, vel = F.clustered_field(16), F.velocity_field(16, 11)
    np.save(tmp_path / "dis.npy", psi)
    np.save(tmp_path / "vel.npy", np.moveaxis(vel, 0, -1))                       # (N, N, N, 3), as the displacement may be
    args = ["--displacement_file", str(tmp_path / "dis.npy"), "--output_dir", str(tmp_path / "out"), "--boxsize", "100",
            "--nmin", "1", "--velocity_file", str(tmp_path / "vel.npy"), "--halo_vprofiles", "--profile_rmin", "0.5",
            "--profile_rmax", "20", "--profile_nbins", "6", "--halo_v12", "--xi_rmin", "0", "--xi_rmax", "30", "--xi_nbins", "6"]
    H.main(args)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["fof_catalog.npz", "halo_v12.npz", "halo_vprofiles.npz"]
    cat = H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=1, velocity=vel)
    want = H.halo_velocity_profiles(cat, psi, vel, 100.0, P.profile_edges(0.5, 20.0, 6))
    got = np.load(tmp_path / "out" / "halo_vprofiles.npz")
    assert sorted(got.files) == VPROFILE_KEYS
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want["counts"]) and got["counts"].sum() > 1000
    assert got["sums"].dtype == np.int64 and np.array_equal(got["sums"], want["sums"]) and got["sums"][:, :, 0].any()
    assert int(got["exponent"]) == want["exponent"] and int(got["count"]) == len(cat["Length"])
    assert np.array_equal(got["Length"], cat["Length"]) and np.array_equal(got["r_edges"], P.profile_edges(0.5, 20.0, 6))
    for k in ("v_r", "sigma_r", "sigma_t"):
        assert np.array_equal(got[k], want[k], equal_nan=True)
    want12 = H.halo_pairwise_velocity(cat, 100.0, np.linspace(0.0, 30.0, 7))
    got12 = np.load(tmp_path / "out" / "halo_v12.npz")
    assert sorted(got12.files) == V12_KEYS
    assert got12["npairs"].dtype == np.int64 and np.array_equal(got12["npairs"], want12["npairs"]) and got12["npairs"].sum() > 1000
    assert np.array_equal(got12["npairs"], H.halo_correlation(cat, 100.0, np.linspace(0.0, 30.0, 7))["npairs"])
    for k in ("sums", "v12", "sigma_r", "sigma_t", "r_edges"):
        assert np.array_equal(got12[k], want12[k], equal_nan=True)
    assert int(got12["exponent"]) == want12["exponent"] and int(got12["count"]) == len(cat["Length"])
    # the catalogue file is what a run without the flags writes
    H.main(args[:3] + [str(tmp_path / "plain")] + args[4:8])
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == ["fof_catalog.npz"]
    plain, moving = np.load(tmp_path / "plain" / "fof_catalog.npz"), np.load(tmp_path / "out" / "fof_catalog.npz")
    assert sorted(plain.files) == sorted(moving.files) and all(np.array_equal(plain[k], moving[k]) for k in plain.files)
    # run_emulator's step on the device fields: the same arrays; without the options, the keys as before
    fof = dict(boxsize=100.0, linking_length=0.2, nmin=1)
    vm = dict(vprofiles=P.profile_edges(0.5, 20.0, 6), v12=np.linspace(0.0, 30.0, 7))
    extra = CLI.fof_catalog(torch.from_numpy(psi).cuda(), fof, 0.3175, vel=torch.from_numpy(vel).cuda(), vmom=vm)
    assert sorted(extra) == ["fof", "halo_v12", "halo_vprofiles"]
    for k in got.files:
        assert np.array_equal(extra["halo_vprofiles"][k], got[k], equal_nan=got[k].dtype.kind == "f"), k
    for k in got12.files:
        assert np.array_equal(extra["halo_v12"][k], got12[k], equal_nan=got12[k].dtype.kind == "f"), k
    assert sorted(CLI.fof_catalog(torch.from_numpy(psi).cuda(), fof, 0.3175)) == ["fof"]
    # a catalogue without a halo: one line each, no file
    capsys.readouterr()
    H.main(args[:3] + [str(tmp_path / "none")] + args[4:6] + ["--nmin", "100000"] + args[8:])
    said = capsys.readouterr().out
    assert "no halo in the catalogue: halo_vprofiles.npz is not written" in said
    assert "no halo in the catalogue: halo_v12.npz is not written" in said
    assert sorted(p.name for p in (tmp_path / "none").iterdir()) == ["fof_catalog.npz"]
