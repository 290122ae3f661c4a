"""The drivers of the halo pair counts: `python -m ...halos --halo_xi` and `run_emulator --fof
--halo_xi`.  The parsers and their checks run on the CPU; one case on the MI355X writes halo_xi.npz."""

import numpy as np
import pytest

import fof_ref as F
from jax_nbody_emulator_with_dj_amd import halos as H, run_emulator as CLI

BASE = ["--displacement_file", "f.npy", "--output_dir", "d"]
RUN = ["--cosmo_param_files", __file__, "--displacement_files", __file__, "--output_dirs", ".", "--ndiv", "1"]


def test_halos_parser_round_trips():
    a = H.build_parser().parse_args(BASE)
    assert (a.halo_xi, a.xi_rmin, a.xi_rmax, a.xi_nbins, a.xi_log, a.xi_nmu) == (False, None, None, None, False, None)
    assert H.xi_options(a, 1000.0, pytest.fail) is None
    a = H.build_parser().parse_args(BASE + ["--halo_xi"])
    xi = H.xi_options(a, 1000.0, pytest.fail)
    assert xi["nmu"] is None and np.array_equal(xi["r_edges"], np.linspace(1.0, 50.0, 21))
    a = H.build_parser().parse_args(BASE + ["--halo_xi", "--xi_rmin", "0.5", "--xi_rmax", "40", "--xi_nbins", "8", "--xi_log",
                                            "--xi_nmu", "10"])
    xi = H.xi_options(a, 1000.0, pytest.fail)
    assert xi["nmu"] == 10 and np.allclose(xi["r_edges"], np.geomspace(0.5, 40.0, 9), rtol=1e-15)
    assert np.array_equal(H.xi_edges(0.0, 30.0, 3), [0.0, 10.0, 20.0, 30.0])

    def die(msg):
        raise SystemExit(msg)
    for extra, match in ((["--xi_rmax", "40"], "--xi_rmax needs --halo_xi"),
                         (["--xi_log"], "--xi_log needs --halo_xi"),
                         (["--xi_nmu", "4"], "--xi_nmu needs --halo_xi"),
                         (["--halo_xi", "--xi_rmax", "400"], "must stay below L / 3"),
                         (["--halo_xi", "--xi_rmin", "60"], "xi_rmin < xi_rmax"),
                         (["--halo_xi", "--xi_nbins", "0"], "xi_nbins >= 1"),
                         (["--halo_xi", "--xi_nbins", "129"], "r_edges must be 2 .. 129"),
                         (["--halo_xi", "--xi_rmin", "0", "--xi_log"], "--xi_log needs xi_rmin > 0"),
                         (["--halo_xi", "--xi_nmu", "33"], "--xi_nmu must be in 1 .. 32")):
        with pytest.raises(SystemExit, match=match):
            H.xi_options(H.build_parser().parse_args(BASE + extra), 1000.0, die)


def test_run_emulator_parser_round_trips():
    ns = CLI.build_parser().parse_args(RUN)
    for name in ("halo_xi", "xi_rmin", "xi_rmax", "xi_nbins", "xi_log", "xi_nmu"):
        assert not hasattr(ns, name)
    assert CLI.halo_xi_options(ns) is None
    ns = CLI.build_parser().parse_args(RUN + ["--fof", "--halo_xi", "--xi_nbins", "5", "--xi_nmu", "4", "--boxsize", "600"])
    xi = CLI.halo_xi_options(ns)
    assert xi["nmu"] == 4 and np.array_equal(xi["r_edges"], np.linspace(1.0, 50.0, 6))
    with pytest.raises(SystemExit):
        CLI.halo_xi_options(CLI.build_parser().parse_args(RUN + ["--halo_xi"]))                    # needs --fof
    with pytest.raises(SystemExit):
        CLI.halo_xi_options(CLI.build_parser().parse_args(RUN + ["--fof", "--xi_nbins", "5"]))      # needs --halo_xi
    with pytest.raises(SystemExit):
        CLI.halo_xi_options(CLI.build_parser().parse_args(RUN + ["--fof", "--halo_xi", "--boxsize", "120"]))   # 50 >= L / 3


@pytest.mark.gpu
def test_halo_xi_file_equals_the_api(tmp_path):
    import torch
    psi = F.clustered_field(16)
    np.save(tmp_path / "dis.npy", psi)
    args = ["--displacement_file", str(tmp_path / "dis.npy"), "--output_dir", str(tmp_path / "out"), "--boxsize", "100",
            "--nmin", "1", "--halo_xi", "--xi_rmin", "0", "--xi_rmax", "30", "--xi_nbins", "6"]
    H.main(args)
    cat = H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=1)
    want = H.halo_correlation(cat, 100.0, np.linspace(0.0, 30.0, 7))
    got = np.load(tmp_path / "out" / "halo_xi.npz")
    assert sorted(got.files) == ["count", "npairs", "r_edges", "r_mid", "rr", "xi"]
    assert got["npairs"].dtype == np.int64 and np.array_equal(got["npairs"], want["npairs"]) and got["npairs"].sum() > 1000
    assert int(got["count"]) == len(cat["Length"]) and got["count"].dtype == np.int64
    for k in ("r_edges", "r_mid", "rr", "xi"):
        assert np.array_equal(got[k], want[k])
    H.main(args + ["--xi_nmu", "4"])
    got = np.load(tmp_path / "out" / "halo_xi.npz")
    want = H.halo_correlation(cat, 100.0, np.linspace(0.0, 30.0, 7), nmu=4)
    assert sorted(got.files) == ["count", "mu_edges", "npairs", "r_edges", "r_mid", "rr", "xi", "xi0", "xi2", "xi4"]
    for k in ("npairs", "xi", "xi0", "xi2", "xi4", "mu_edges"):
        assert np.array_equal(got[k], want[k])
    # run_emulator's step on the device displacement: the same arrays
    extra = CLI.fof_catalog(torch.from_numpy(psi).cuda(), dict(boxsize=100.0, linking_length=0.2, nmin=1), 0.3,
                            xi=dict(r_edges=np.linspace(0.0, 30.0, 7), nmu=4))
    assert sorted(extra) == ["fof", "halo_xi"]
    for k in got.files:
        assert np.array_equal(extra["halo_xi"][k], got[k])
