"""Radial profiles and spherical-overdensity masses on the MI355X: profiles.radial_counts against
the NumPy restatement of tests/profiles_ref.py.  Counts are integers and are compared with ==, never with a tolerance."""

import functools

import numpy as np
import pytest

import fof_ref as F
import pairs_ref as R
import profiles_ref as PR
from jax_nbody_emulator_with_dj_amd import correlation as CF, halos as H, profiles as P, run_emulator as CLI

pytestmark = pytest.mark.gpu

L, EDGES = R.UNIFORM_L, R.UNIFORM_EDGES
NPZ_KEYS = ["Length", "M_delta", "N_delta", "R_delta", "count", "counts", "flag", "overdensity", "r_edges", "r_mid", "reference",
            "rho"]


def check_dict(out, ref, edges, boxsize, count_a, count_b):
    assert isinstance(out["counts"], np.ndarray) and out["counts"].dtype == np.int64 and out["counts"].shape == ref.shape
    assert np.array_equal(out["counts"], ref)
    assert out["r_edges"].dtype == np.float64 and np.array_equal(out["r_edges"], np.asarray(edges, np.float64))
    T = R.thresholds(edges, boxsize)
    assert out["thresholds"].dtype == np.int64 and out["thresholds"].tolist() == T
    assert out["ncell"] == R.ncell_of(T) and out["count_a"] == count_a and out["count_b"] == count_b
    assert sorted(out) == ["count_a", "count_b", "counts", "ncell", "r_edges", "thresholds"]


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_uniform_points_several_boxes_away(dtype):
    centres, matter, ref = PR.uniform_case(dtype)
    out = P.radial_counts(centres, matter, L, EDGES)
    check_dict(out, ref, EDGES, L, 300, 1500)
    npairs = CF.pair_counts(centres, L, EDGES, b=matter)["npairs"]               # the existing kernel: the stacked sum
    assert np.array_equal(out["counts"].sum(axis=0), npairs)
    # a centre is a matter row: itself in bin 0 with r_0 = 0, nowhere with r_0 = 2
    assert out["counts"][:, 0].min() >= 1
    inner = P.radial_counts(centres, matter, L, EDGES[1:])
    assert np.array_equal(inner["counts"], ref[:, 1:])
    assert np.array_equal(inner["counts"].sum(axis=0), CF.pair_counts(centres, L, EDGES[1:], b=matter)["npairs"])
    alone = P.radial_counts(centres, centres[:1] + 0.0, L, EDGES)["counts"]       # matter = the first centre only
    assert alone[0].tolist() == [1, 0, 0, 0, 0] and alone.sum() == PR.counts_of(centres, centres[:1], L, EDGES).sum()


@functools.lru_cache(maxsize=None)
def clustered():
    psi = F.clustered_field(16)
    cat = H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=20)
    corners = np.array([[x, y, z] for x in (0.0, 100.0) for y in (0.0, 100.0) for z in (0.0, 100.0)])
    faces = np.array([[50.0, 50.0, 0.0], [50.0, 0.0, 50.0], [0.0, 50.0, 50.0], [50.0, 50.0, 100.0], [100.0, 50.0, 50.0],
                      [50.0, 100.0, 50.0]])
    return psi, cat, np.concatenate([cat["CMPosition"], corners, faces])


def test_clustered_lattice_halo_centres_corners_and_faces():
    psi, cat, centres = clustered()
    assert len(cat["Length"]) >= 3
    edges = PR.profile_edges(0.5, 20.0, 12)
    ref = PR.counts_of(centres, psi, 100.0, edges)
    out = P.radial_counts(centres, psi, 100.0, edges)
    check_dict(out, ref, edges, 100.0, len(centres), 4096)
    assert ref.sum(axis=1).min() > 0                                             # every corner and face sees matter
    assert np.array_equal(P.radial_counts(centres, psi.astype(np.float16).astype(np.float32), 100.0, edges)["counts"],
                          P.radial_counts(centres, psi.astype(np.float16), 100.0, edges)["counts"])
    # halos.halo_profiles with a selection: the rows of the halos kept, Length and count
    big = int(np.sort(cat["Length"])[-2])
    hp = H.halo_profiles(cat, psi, 100.0, edges, min_length=big)
    keep = cat["Length"] >= big
    assert hp["count"] == int(keep.sum()) < len(keep) and np.array_equal(hp["Length"], cat["Length"][keep])
    assert np.array_equal(hp["counts"], ref[:len(keep)][keep]) and "R" not in hp
    so = H.halo_profiles(cat, psi, 100.0, edges, overdensity=50.0, particle_mass=2.0)
    want = PR.spherical_overdensity(ref[:len(keep)], edges, 100.0, 4096, 50.0)
    np.testing.assert_allclose(so["R"], want[0], rtol=1e-12, equal_nan=True)
    assert np.array_equal(so["flag"], want[2]) and so["delta_eff"] == 50.0 and (so["flag"] == 0).any()
    np.testing.assert_allclose(so["M"], 2.0 * so["N"], rtol=1e-15, equal_nan=True)


def test_three_cells_every_range_wraps():
    rng = np.random.default_rng(31)
    centres, matter = rng.uniform(0.0, 100.0, size=(40, 3)), rng.uniform(0.0, 100.0, size=(200, 3))
    edges = (0.0, 10.0, 33.3)
    out = P.radial_counts(centres, matter, 100.0, edges)
    assert out["ncell"] == 3
    check_dict(out, PR.counts_of(centres, matter, 100.0, edges), edges, 100.0, 40, 200)


def test_finest_cell_grid():
    ten = np.random.default_rng(32).uniform(0.0, 100.0, size=(10, 3))
    out = P.radial_counts(ten, ten, 100.0, (0.0, 0.01, 0.02))
    assert out["ncell"] == 4096
    assert np.array_equal(out["counts"], np.repeat([[1, 0]], 10, axis=0))
    check_dict(out, PR.counts_of(ten, ten, 100.0, (0.0, 0.01, 0.02)), (0.0, 0.01, 0.02), 100.0, 10, 10)


@pytest.mark.parametrize("count", [255, 256, 257, 1000])
def test_one_full_cell_at_the_tile_boundaries(count):
    """One cell holds all the matter: the stream's steps of 256 (and of 64) records end exactly at, before and after it."""
    centre, matter, box, edges = PR.one_cell_case(count)
    ref = PR.counts_of(centre, matter, box, edges)
    assert ref.sum() == count
    for form in (None, 0, 1):
        assert np.array_equal(P.radial_counts(centre, matter, box, edges, _form=form)["counts"], ref), form


def test_separations_that_equal_a_threshold():
    pts = R.edge_points()
    ref = PR.counts_of(pts, pts, R.EDGE_L, R.EDGE_EDGES)
    assert ref.sum() - len(pts) >= 480                                           # each of the 240 pairs from both ends
    for form in (0, 1):
        assert np.array_equal(P.radial_counts(pts, pts, R.EDGE_L, R.EDGE_EDGES, _form=form)["counts"], ref)


def test_bin_numbers_and_smallest_catalogues():
    pos = R.uniform_points()
    for edges in ((0.0, 25.0), np.linspace(0.0, 30.0, 129)):
        ref = PR.counts_of(pos[:50], pos, L, edges)
        for form in (0, 1):
            assert np.array_equal(P.radial_counts(pos[:50], pos, L, edges, _form=form)["counts"], ref)
    one = P.radial_counts(pos[:1], pos[:1], L, EDGES)
    check_dict(one, np.array([[1, 0, 0, 0, 0]], np.int64), EDGES, L, 1, 1)
    assert P.radial_counts(pos[:1], pos[1:2], L, EDGES[1:])["counts"].shape == (1, 4)


def test_launch_geometry_forms_and_order():
    centres, matter, ref = PR.uniform_case("float64")
    for blocks in (1, 3):
        for form in (0, 1):
            assert np.array_equal(P.radial_counts(centres, matter, L, EDGES, _max_blocks=blocks, _form=form)["counts"], ref)
    rng = np.random.default_rng(33)
    pc, pm = rng.permutation(300), rng.permutation(1500)
    assert np.array_equal(P.radial_counts(centres[pc], matter[pm], L, EDGES)["counts"], ref[pc])


def test_the_library_takes_both_forms():
    """nbe_halo_profiles runs a wave per centre from 4096 centres on where the cells are sparse (NBE_PROFILE_WAVE_CENTRES,
    NBE_PROFILE_WAVE_BELOW), else a workgroup: 4095, 4096 and 5000 centres with sparse cells, and 5000 with dense ones."""
    centres = R.uniform_points(5000, L, 6)
    matter = R.uniform_points()
    for edges in ((0.0, 2.0, 5.0), EDGES):                                      # 27 * 1500 / ncell^3: 0.004, and 1500
        ref = PR.counts_of(centres, matter, L, edges)
        assert ref.sum() > 0
        for rows in (4095, 4096, 5000):
            assert np.array_equal(P.radial_counts(centres[:rows], matter, L, edges)["counts"], ref[:rows]), (edges, rows)
        for form in (0, 1):
            assert np.array_equal(P.radial_counts(centres, matter, L, edges, _form=form)["counts"], ref)


def test_residency_and_streams():
    import torch
    centres, matter, ref = PR.uniform_case("float64")
    tc, tm = torch.from_numpy(centres.copy()).cuda(), torch.from_numpy(matter.copy()).cuda()
    out = P.radial_counts(tc, tm, L, EDGES)
    for k in ("counts", "r_edges", "thresholds"):
        assert isinstance(out[k], torch.Tensor) and out[k].device == tc.device
    assert out["counts"].dtype == torch.int64 and np.array_equal(out["counts"].cpu().numpy(), ref)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = P.radial_counts(tc, tm, L, EDGES)["counts"]
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), ref)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        P.radial_counts(tc, matter, L, EDGES)
    assert isinstance(P.radial_counts(centres, matter, L, EDGES)["counts"], np.ndarray)


def test_a_nan_centre_is_refused():
    centres, matter, _ = PR.uniform_case("float64")
    bad = centres.copy()
    bad[17, 1] = np.nan
    with pytest.raises(ValueError, match="1 row\\(s\\) have a non-finite position"):
        P.radial_counts(bad, matter, L, EDGES)
    far = matter.copy()
    far[3, 0] = 2.0 ** 21 * L
    with pytest.raises(ValueError, match="non-finite position or one 2\\^20 boxes"):
        P.radial_counts(centres, far, L, EDGES)


def test_spherical_overdensity_of_an_isothermal_halo():
    """N0 = 1500 points at radii R0 (i + 1/2) / N0 about (99, 0.5, 50) and no other matter: N(< r) is within 1/2 of
    N0 r / R0 and D ~ r^-2, for which the log-log interpolation is exact, so R_Delta = 0.8 R0 to 0.25 / N(<= r_j*)."""
    pos = PR.isothermal_halo()
    centre = np.array([PR.ISO_CENTRE])
    out = P.radial_counts(centre, pos, PR.ISO_L, PR.ISO_EDGES)
    ref = PR.counts_of(centre, pos, PR.ISO_L, PR.ISO_EDGES)
    assert np.array_equal(out["counts"], ref) and ref.sum() == PR.ISO_N
    delta = PR.isothermal_overdensity(0.8 * PR.ISO_R0)
    so = P.spherical_overdensity(out["counts"], out["r_edges"], PR.ISO_L, out["count_b"], overdensity=delta)
    want = PR.spherical_overdensity(ref, PR.ISO_EDGES, PR.ISO_L, PR.ISO_N, delta)
    assert so["flag"].tolist() == [0] == want[2].tolist()
    assert abs(so["R"][0] / want[0][0] - 1.0) <= 1e-12 and abs(so["N"][0] / want[1][0] - 1.0) <= 1e-11
    enclosed = np.cumsum(ref[0])
    D = enclosed / (PR.ISO_N / PR.ISO_L ** 3 * 4.0 * np.pi / 3.0 * PR.ISO_EDGES[1:] ** 3)
    jstar = int(np.argmax(D < delta))
    assert jstar >= 1 and PR.ISO_EDGES[jstar] < 0.8 * PR.ISO_R0 <= PR.ISO_EDGES[jstar + 1]
    bound = 0.25 / enclosed[jstar - 1]
    print("R_delta / (0.8 R0) - 1 = %.3e, bound %.3e, j* = %d" % (so["R"][0] / (0.8 * PR.ISO_R0) - 1.0, bound, jstar))
    assert abs(so["R"][0] / (0.8 * PR.ISO_R0) - 1.0) <= bound


def test_halo_profiles_file_equals_the_api(tmp_path, capsys):
    import torch
    psi, cat, _ = clustered()
    np.save(tmp_path / "dis.npy", psi)
    args = ["--displacement_file", str(tmp_path / "dis.npy"), "--output_dir", str(tmp_path / "out"), "--boxsize", "100",
            "--halo_profiles", "--profile_rmin", "0.5", "--profile_rmax", "20", "--profile_nbins", "12", "--so_overdensity", "50"]
    H.main(args)
    assert sorted(p.name for p in (tmp_path / "out").iterdir()) == ["fof_catalog.npz", "halo_profiles.npz"]
    got = np.load(tmp_path / "out" / "halo_profiles.npz")
    assert sorted(got.files) == NPZ_KEYS
    edges = P.profile_edges(0.5, 20.0, 12)
    want = P.radial_counts(cat["CMPosition"], psi, 100.0, edges)
    assert got["counts"].dtype == np.int64 and np.array_equal(got["counts"], want["counts"])
    assert np.array_equal(got["counts"], PR.counts_of(cat["CMPosition"], psi, 100.0, edges)) and got["counts"].min(axis=1).max() > 0
    assert np.array_equal(got["r_edges"], edges) and np.array_equal(got["Length"], cat["Length"])
    assert int(got["count"]) == len(cat["Length"]) and str(got["reference"]) == "mean" and float(got["overdensity"]) == 50.0
    prof = P.density_profile(want["counts"], edges, 100.0, 4096)
    assert np.array_equal(got["rho"], prof["rho"]) and np.array_equal(got["r_mid"], prof["r_mid"])
    so = P.spherical_overdensity(want["counts"], edges, 100.0, 4096, overdensity=50.0,
                                 particle_mass=H.particle_mass(0.3175, 100.0, 16))
    for key, name in (("R_delta", "R"), ("N_delta", "N"), ("M_delta", "M"), ("flag", "flag")):
        assert np.array_equal(got[key], so[name], equal_nan=key != "flag")
    # run_emulator's step on the device displacement: the same arrays; without the option, the keys as before
    fof = dict(boxsize=100.0, linking_length=0.2, nmin=20)
    extra = CLI.fof_catalog(torch.from_numpy(psi).cuda(), fof, 0.3175,
                            profiles=dict(r_edges=edges, overdensity=50.0, reference="mean"))
    assert sorted(extra) == ["fof", "halo_profiles"]
    for k in got.files:
        assert np.array_equal(extra["halo_profiles"][k], got[k], equal_nan=got[k].dtype.kind == "f")
    assert sorted(CLI.fof_catalog(torch.from_numpy(psi).cuda(), fof, 0.3175)) == ["fof"]
    # a catalogue without a halo: one line, no file
    capsys.readouterr()
    H.main(args[:3] + [str(tmp_path / "none")] + args[4:] + ["--nmin", "100000"])
    assert "no halo in the catalogue: halo_profiles.npz is not written" in capsys.readouterr().out
    assert sorted(p.name for p in (tmp_path / "none").iterdir()) == ["fof_catalog.npz"]
