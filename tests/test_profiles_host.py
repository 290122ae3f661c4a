"""Radial profiles and spherical-overdensity masses on the CPU: argument errors before any device
work, the SO arithmetic on hand-made count tables, stack_profiles and profile_edges, the NumPy restatement of
tests/profiles_ref.py against scipy's periodic cKDTree, the declared symbols and the drivers' parsers."""

import math
import re

import numpy as np
import pytest

import pairs_ref as R
import profiles_ref as PR
from jax_nbody_emulator_with_dj_amd import _lib, halos as H, profiles as P, run_emulator as CLI

BASE = ["--displacement_file", "f.npy", "--output_dir", "d"]
RUN = ["--cosmo_param_files", __file__, "--displacement_files", __file__, "--output_dirs", ".", "--ndiv", "1"]
NEW_OPTIONS = ("halo_profiles", "profile_rmin", "profile_rmax", "profile_nbins", "so_overdensity", "so_reference")


def test_argument_errors_come_before_device_work(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: pytest.fail("the library was reached"))
    ok = np.zeros((4, 3))
    for centres, matter, match in ((np.zeros((4, 2)), ok, r"must be \(count, 3\) positions"),
                                   (np.zeros((3, 4, 4, 4), np.float32), ok, r"centres must be \(H, 3\) positions"),
                                   (np.zeros((0, 3)), ok, "1 .. 2\\^30 rows"),
                                   (ok.astype(np.int64), ok, "float32 or float64"),
                                   (ok, np.zeros((4, 3), np.float16), "float32 or float64"),
                                   (ok, np.zeros((3, 4, 4, 4), np.float64), "float32 or float16"),
                                   (ok, np.zeros((3, 4, 4, 5), np.float32), "positions or a"),
                                   ([[0.0, 0.0, 0.0]], ok, "NumPy array or a CUDA torch tensor")):
        with pytest.raises(ValueError, match=match):
            P.radial_counts(centres, matter, 100.0, [0.0, 1.0])
    for edges, match in (([0.0, 10.0, 100.0 / 3.0], "below L / 3"), ([0.0, 40.0], "below L / 3"), ([1.0], "r_edges must be 2"),
                         ([0.0, 2.0, 2.0], "strictly increasing"), ([-1.0, 2.0], "strictly increasing"),
                         (np.linspace(0.0, 30.0, 130), "r_edges must be 2 .. 129"), ([0.0, np.nan], "finite")):
        with pytest.raises(ValueError, match=match):
            P.radial_counts(ok, ok, 100.0, edges)
    with pytest.raises(ValueError, match="cubic box"):
        P.radial_counts(ok, ok, (100.0, 100.0, 50.0), [0.0, 1.0])
    with pytest.raises(ValueError, match="_max_blocks"):
        P.radial_counts(ok, ok, 100.0, [0.0, 1.0], _max_blocks=0)
    with pytest.raises(ValueError, match="_form"):
        P.radial_counts(ok, ok, 100.0, [0.0, 1.0], _form=2)
    import torch
    with pytest.raises(ValueError, match="centres: a torch tensor must live on a CUDA"):
        P.radial_counts(torch.zeros((4, 3)), ok, 100.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="matter: a torch tensor must live on a CUDA"):
        P.radial_counts(ok, torch.zeros((4, 3)), 100.0, [0.0, 1.0])
    # the host functions
    table = np.ones((2, 3), np.int64)
    with pytest.raises(ValueError, match=r"r_edges\[0\] == 0"):
        P.spherical_overdensity(table, [0.5, 1.0, 2.0, 3.0], 100.0, 10)
    with pytest.raises(ValueError, match="'critical' needs Om"):
        P.spherical_overdensity(table, [0.0, 1.0, 2.0, 3.0], 100.0, 10, reference="critical")
    with pytest.raises(ValueError, match="'mean' or 'critical'"):
        P.spherical_overdensity(table, [0.0, 1.0, 2.0, 3.0], 100.0, 10, reference="virial")
    with pytest.raises(ValueError, match="overdensity must be a positive"):
        P.spherical_overdensity(table, [0.0, 1.0, 2.0, 3.0], 100.0, 10, overdensity=0.0)
    with pytest.raises(ValueError, match="nb \\+ 1 edges"):
        P.spherical_overdensity(table, [0.0, 1.0, 2.0], 100.0, 10)
    with pytest.raises(ValueError, match="integer table"):
        P.density_profile(table.astype(np.float64), [0.0, 1.0, 2.0, 3.0], 100.0, 10)
    # halo_profiles: the selection and the SO arguments, before radial_counts
    cat = dict(CMPosition=np.zeros((2, 3)), Length=np.array([30, 20]))
    with pytest.raises(ValueError, match="paint_halos needs fof_halos's dict"):
        H.halo_profiles([1, 2], ok, 100.0, [0.0, 1.0])
    with pytest.raises(ValueError, match="no halo is left"):
        H.halo_profiles(cat, ok, 100.0, [0.0, 1.0], min_length=50)
    with pytest.raises(ValueError, match=r"r_edges\[0\] == 0"):
        H.halo_profiles(cat, ok, 100.0, [0.5, 1.0], overdensity=200.0)
    with pytest.raises(ValueError, match="'critical' needs Om"):
        H.halo_profiles(cat, ok, 100.0, [0.0, 1.0], overdensity=200.0, reference="critical")


def _table(D, edges, nbar):
    """The count table (1, nb) whose enclosed overdensities are D (chosen so that the enclosed numbers are integers)."""
    N = np.array([d * nbar * 4.0 * math.pi / 3.0 * r ** 3 for d, r in zip(D, edges[1:])])
    Ni = np.rint(N).astype(np.int64)
    assert np.abs(N - Ni).max() < 1e-6 and (np.diff(Ni) >= 0).all()
    return np.diff(np.concatenate([[0], Ni]))[None, :]


def test_spherical_overdensity_by_hand():
    # nbar 4 pi / 3 = 1: N_j = D_j r_{j+1}^3 exactly
    L, count_b = 1.0, 3
    nbar = 3.0
    unit = 1.0 / (nbar * 4.0 * math.pi / 3.0)                                # D of one particle inside r = 1
    edges = np.array([0.0, 1.0, 2.0, 4.0])
    vol = edges[1:] ** 3
    def so(N, delta_in_units):
        c = np.diff(np.concatenate([[0], N]))[None, :]
        return P.spherical_overdensity(c, edges, L, count_b, overdensity=delta_in_units * unit), c
    # D = (64, 16, 4) units: N = (64, 128, 256).  Delta = 8 units lies in the last interval, D ~ r^-2: R = 2 sqrt(2)
    out, c = so([64, 128, 256], 8.0)
    assert out["flag"].tolist() == [0] and out["R"][0] == pytest.approx(2.0 * math.sqrt(2.0), rel=1e-14)
    assert out["N"][0] == pytest.approx(8.0 * (2.0 * math.sqrt(2.0)) ** 3, rel=1e-13) and out["M"] is None
    assert out["delta_eff"] == pytest.approx(8.0 * unit)
    # Delta = 32 units: the first interval that can hold a crossing, (r_1, r_2]: R = sqrt(2)
    out, _ = so([64, 128, 256], 32.0)
    assert out["flag"].tolist() == [0] and out["R"][0] == pytest.approx(math.sqrt(2.0), rel=1e-14)
    # D equal to Delta exactly at an edge is not below: Delta = 16 units = D_1, so j* = 2 and t = 0: R = r_2 exactly
    out, _ = so([64, 128, 256], 16.0)
    assert out["flag"].tolist() == [0] and out["R"][0] == pytest.approx(2.0, rel=1e-15)
    # ... and at the first edge: Delta = 64 units = D_0 is not flag 1
    out, _ = so([64, 128, 256], 64.0)
    assert out["flag"].tolist() == [0] and out["R"][0] == pytest.approx(1.0, rel=1e-15)
    # flag 1: below Delta at the first edge; flag 2: never below; a row of zeros is flag 1
    out, _ = so([64, 128, 256], 65.0)
    assert out["flag"].tolist() == [1] and np.isnan(out["R"][0]) and np.isnan(out["N"][0])
    out, _ = so([64, 128, 256], 4.0)                                          # D_2 = 4 units is not below 4
    assert out["flag"].tolist() == [2] and np.isnan(out["R"][0])
    out, _ = so([0, 0, 0], 1.0)
    assert out["flag"].tolist() == [1] and out["flag"].dtype == np.int8
    # several rows at once, a particle mass, and the restatement
    table = np.array([[64, 64, 128], [0, 0, 0], [64, 448, 3584], [10, 0, 0]], np.int64)
    out = P.spherical_overdensity(table, edges, L, count_b, overdensity=8.0 * unit, particle_mass=2.5)
    assert out["flag"].tolist() == [0, 1, 2, 0]
    ref = PR.spherical_overdensity(table, edges, L, count_b, overdensity=8.0 * unit)
    np.testing.assert_allclose(out["R"], ref[0], rtol=1e-13, equal_nan=True)
    np.testing.assert_allclose(out["N"], ref[1], rtol=1e-13, equal_nan=True)
    assert np.array_equal(out["flag"], ref[2])
    np.testing.assert_allclose(out["M"], 2.5 * out["N"], rtol=1e-15, equal_nan=True)
    # critical: Delta = overdensity / Omega_m(z)
    out = P.spherical_overdensity(table, edges, L, count_b, overdensity=200.0, reference="critical", Om=0.3, z=1.0)
    om = 0.3 * 8.0 / (0.3 * 8.0 + 0.7)
    assert out["delta_eff"] == pytest.approx(200.0 / om, rel=1e-15) == PR.spherical_overdensity(
        table, edges, L, count_b, 200.0, "critical", 0.3, 1.0)[3]
    assert P.spherical_overdensity(table, edges, L, count_b, reference="critical", Om=1.0)["delta_eff"] == 200.0
    del vol, c


def test_density_profile_stack_and_edges():
    edges = np.array([0.0, 1.0, 2.0, 4.0])
    counts = np.array([[1, 7, 56], [0, 0, 3]], np.int64)
    out = P.density_profile(counts, edges, 10.0, 500)
    nbar = 0.5
    np.testing.assert_allclose(out["rho"][0], np.array([1, 7, 56]) / (nbar * 4.0 * np.pi / 3.0 * np.array([1.0, 7.0, 56.0])),
                               rtol=1e-15)
    assert np.array_equal(out["enclosed"], [[1, 8, 64], [0, 0, 3]]) and out["enclosed"].dtype == np.int64
    assert np.array_equal(out["r_mid"], [0.5, 1.5, 3.0])
    lengths = np.array([20, 99, 100, 450, 1000, 5])
    table = np.arange(18, dtype=np.int64).reshape(6, 3) * (1 << 40)
    stacked, halos = P.stack_profiles(table, lengths, [20, 100, 1000])
    assert halos.tolist() == [2, 2] and stacked.dtype == np.int64
    assert np.array_equal(stacked, [table[0] + table[1], table[2] + table[3]])
    with pytest.raises(ValueError, match="lengths"):
        P.stack_profiles(table, lengths[:3], [20, 100])
    with pytest.raises(ValueError, match="increasing"):
        P.stack_profiles(table, lengths, [100, 20])
    e = P.profile_edges(0.05, 5.0, 20)
    assert e.shape == (21,) and e[0] == 0.0 and np.array_equal(e[1:], np.geomspace(0.05, 5.0, 20))
    assert np.array_equal(e, PR.profile_edges(0.05, 5.0, 20))
    for bad in ((0.0, 5.0, 20), (5.0, 5.0, 20), (0.05, 5.0, 1), (0.05, np.inf, 4)):
        with pytest.raises(ValueError):
            P.profile_edges(*bad)


def test_restatement_against_ckdtree():
    """Counts within r of 40 centres among 500 points: scipy's periodic tree on the rounded coordinates against the
    cumulative counts of the restatement (float64 distances of integers below 2^30 are far from an edge here)."""
    from scipy.spatial import cKDTree
    L, edges = 100.0, np.array([0.0, 3.0, 7.0, 12.0, 21.0, 33.0])
    pos = np.mod(R.uniform_points()[:500], L)
    XB = R.coordinates(pos, L)
    XA = XB[:, :40]
    ref = PR.radial_counts(XA, XB, R.thresholds(edges, L))
    assert ref[:, 0].min() >= 1                                              # a centre is a matter row: itself, in bin 0
    pts = XB.T.astype(np.float64) / R.U * L
    tree = cKDTree(np.mod(pts, L), boxsize=L)
    for j, r in enumerate(edges[1:]):
        within = np.array([len(v) for v in tree.query_ball_point(np.mod(pts[:40], L), r)])
        assert np.array_equal(within, ref[:, :j + 1].sum(axis=1)), r
    # r_0 > 0 leaves the centre itself out, and every other count as it was
    ref2 = PR.radial_counts(XA, XB, R.thresholds(edges[1:], L))
    assert np.array_equal(ref2, ref[:, 1:])


def test_abi_and_modules_are_declared():
    assert "nbe_profiles.hip" in _lib.SOURCES
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "nbe.h")).read()
    section = header[header.index("---- Profiles"):header.index("---- test / measurement hooks")]
    names = re.findall(r"^int (nbe_\w+)\(", section, flags=re.M)
    assert names == ["nbe_halo_profiles", "nbe_halo_profiles_form"]
    for name in names:
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["nbe_halo_profiles_form"][1][:10] == _lib.SIGNATURES["nbe_halo_profiles"][1][:10]
    for word in ("Rockstar", "AHF", "the reference does not have", "spherical-overdensity"):
        assert word in section.replace("\n * ", " ")
    pairs = header[header.index("---- Pairs"):header.index("---- Input fields")]
    assert re.findall(r"^int (nbe_\w+)\(", pairs, flags=re.M) == ["nbe_pair_coords", "nbe_pair_count", "nbe_pair_count_form"]
    assert header.index("---- Profiles") > header.index("---- Input fields")
    assert int(re.search(r"#define NBE_PROFILE_WAVE_BELOW (\d+)", section).group(1)) > 0 and P.FORMS == (0, 1)
    assert P.__all__ == ["radial_counts", "density_profile", "spherical_overdensity", "stack_profiles", "profile_edges"]
    assert "halo_profiles" in H.__all__
    import jax_nbody_emulator_with_dj_amd as pkg
    assert not hasattr(pkg, "radial_counts") and "radial_counts" not in pkg.__all__ and "profiles" not in pkg.__all__


def test_parsers_round_trip():
    a = H.build_parser().parse_args(BASE)
    assert [getattr(a, n) for n in NEW_OPTIONS] == [False, None, None, None, None, None]
    assert H.profile_options(a, 1000.0, pytest.fail) is None
    prof = H.profile_options(H.build_parser().parse_args(BASE + ["--halo_profiles"]), 1000.0, pytest.fail)
    assert np.array_equal(prof["r_edges"], P.profile_edges(0.05, 5.0, 20))
    assert (prof["overdensity"], prof["reference"]) == (200.0, "mean")
    a = H.build_parser().parse_args(BASE + ["--halo_profiles", "--profile_rmin", "0.1", "--profile_rmax", "15", "--profile_nbins",
                                            "12", "--so_overdensity", "500", "--so_reference", "critical"])
    prof = H.profile_options(a, 1000.0, pytest.fail)
    assert np.array_equal(prof["r_edges"], P.profile_edges(0.1, 15.0, 12))
    assert (prof["overdensity"], prof["reference"]) == (500.0, "critical")

    def die(msg):
        raise SystemExit(msg)
    for extra, match in ((["--profile_rmax", "4"], "--profile_rmax needs --halo_profiles"),
                         (["--so_overdensity", "500"], "--so_overdensity needs --halo_profiles"),
                         (["--so_reference", "mean"], "--so_reference needs --halo_profiles"),
                         (["--halo_profiles", "--profile_rmax", "400"], "must stay below L / 3"),
                         (["--halo_profiles", "--profile_rmin", "6"], "0 < rmin < rmax"),
                         (["--halo_profiles", "--profile_nbins", "1"], "nbins must be an int >= 2"),
                         (["--halo_profiles", "--profile_nbins", "129"], "r_edges must be 2 .. 129"),
                         (["--halo_profiles", "--so_overdensity", "-1"], "--so_overdensity must be positive")):
        with pytest.raises(SystemExit, match=match):
            H.profile_options(H.build_parser().parse_args(BASE + extra), 1000.0, die)
    with pytest.raises(SystemExit):
        H.build_parser().parse_args(BASE + ["--halo_profiles", "--so_reference", "virial"])
    # run_emulator: absent unless given, and --fof is needed
    ns = CLI.build_parser().parse_args(RUN)
    for name in NEW_OPTIONS:
        assert not hasattr(ns, name)
    assert CLI.halo_profile_options(ns) is None
    ns = CLI.build_parser().parse_args(RUN + ["--fof", "--halo_profiles", "--profile_nbins", "8", "--boxsize", "600"])
    prof = CLI.halo_profile_options(ns)
    assert np.array_equal(prof["r_edges"], P.profile_edges(0.05, 5.0, 8)) and prof["overdensity"] == 200.0
    with pytest.raises(SystemExit):
        CLI.halo_profile_options(CLI.build_parser().parse_args(RUN + ["--halo_profiles"]))                 # needs --fof
    with pytest.raises(SystemExit):
        CLI.halo_profile_options(CLI.build_parser().parse_args(RUN + ["--fof", "--profile_nbins", "5"]))    # needs --halo_profiles
    with pytest.raises(SystemExit):
        CLI.halo_profile_options(CLI.build_parser().parse_args(RUN + ["--fof", "--halo_profiles", "--boxsize", "12"]))
    # the existing options and their file lists are as they were
    assert H.xi_options(H.build_parser().parse_args(BASE), 1000.0, pytest.fail) is None
    assert H.CATALOG_FILE == "fof_catalog.npz" and H.HALO_PROFILES_FILE == "halo_profiles.npz"
