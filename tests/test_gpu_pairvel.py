"""Pairwise velocity moments on the MI355X: correlation.pairwise_velocity, profiles.radial_velocity_moments
and the halo functions above them against the Python-int restatement of tests/pairvel_ref.py.  Every sum is an integer fixed by
the pair alone and is compared with ==, never with a tolerance; the float64 moments are formed from those integers by the same
expressions and are compared with == too."""

import functools

import numpy as np
import pytest

import fof_ref as F
import pairs_ref as R
import pairvel_ref as V
from jax_nbody_emulator_with_dj_amd import correlation as CF, halos as H, profiles as P

pytestmark = pytest.mark.gpu

L, EDGES = R.UNIFORM_L, R.UNIFORM_EDGES
PAIR_KEYS = ["count_a", "count_b", "exponent", "ncell", "npairs", "r_edges", "sigma_r", "sigma_t", "sums", "thresholds", "v12",
             "vr2", "vt2"]
PROFILE_KEYS = ["count_a", "count_b", "counts", "exponent", "ncell", "r_edges", "sums", "thresholds"]
MOMENTS = ("v12", "vr2", "sigma_r", "vt2", "sigma_t")


@functools.lru_cache(maxsize=None)
def reference(name):
    """(case, pair table (nb, 6) or None, exponent, per-centre tables (H, nb, 6) or None) of a shared case, once per process."""
    a, va, b, vb, box, edges = case = V.case(name)
    pairs = None if va is None else V.moments_of(a, va, box, edges, b, vb)[0]
    tables = None if b is None else V.profiles_of(a, va, b, vb, box, edges)[0]
    for t in (pairs, tables):
        if t is not None:
            t.setflags(write=False)
    return case, pairs, V.exponent(va, vb), tables


def check_pairs(out, ref, e, edges, box, count_a, count_b):
    assert sorted(out) == PAIR_KEYS
    assert isinstance(out["npairs"], np.ndarray) and out["npairs"].dtype == np.int64 and out["sums"].dtype == np.int64
    assert np.array_equal(out["npairs"], ref[:, 0]) and np.array_equal(out["sums"], ref[:, 1:]) and out["exponent"] == e
    want = V.derived(ref, e)
    for k in MOMENTS:
        assert out[k].dtype == np.float64 and np.array_equal(out[k], want[k], equal_nan=True), k
    T = R.thresholds(edges, box)
    assert np.array_equal(out["r_edges"], np.asarray(edges, np.float64)) and out["thresholds"].tolist() == T
    assert out["ncell"] == R.ncell_of(T) and out["count_a"] == count_a and out["count_b"] == count_b


def check_tables(out, ref, e, edges, box, count_a, count_b):
    assert sorted(out) == PROFILE_KEYS
    assert isinstance(out["counts"], np.ndarray) and out["counts"].dtype == np.int64 and out["sums"].dtype == np.int64
    assert np.array_equal(out["counts"], ref[:, :, 0]) and np.array_equal(out["sums"], ref[:, :, 1:]) and out["exponent"] == e
    T = R.thresholds(edges, box)
    assert np.array_equal(out["r_edges"], np.asarray(edges, np.float64)) and out["thresholds"].tolist() == T
    assert out["ncell"] == R.ncell_of(T) and out["count_a"] == count_a and out["count_b"] == count_b


def rows_of(x):
    x = np.asarray(x)
    return x.shape[0] if x.ndim == 2 else x.shape[1] ** 3


@pytest.mark.parametrize("name", V.CASE_NAMES)
def test_every_shared_case_in_every_form(name):
    """The list of tests/pairvel_ref.py: uniform points several boxes away in float64 and float32, the clustered lattice in
    float32 and float16 about its centres, the box corners and face centres, ncell = 3 and 4096, one full cell of 255, 256,
    257 and 1000 rows, separations on a threshold, 1 and 128 bins, one row against one, coincident rows, zero velocities,
    words of +-2^20, centres at rest."""
    (a, va, b, vb, box, edges), pairs, e, tables = reference(name)
    nb = len(edges) - 1
    if pairs is not None:
        assert pairs[:, 0].sum() > 0
        for form in (None,) + CF.VELOCITY_FORMS:
            out = CF.pairwise_velocity(a, va, box, edges, b=b, vel_b=vb, _form=form)
            check_pairs(out, pairs, e, edges, box, rows_of(a), None if b is None else rows_of(b))
        assert np.array_equal(out["npairs"], CF.pair_counts(a, box, edges, b=b)["npairs"])      # the count kernel's bits
    if tables is not None:
        for form in (None,) + P.FORMS:
            out = P.radial_velocity_moments(a, va, b, vb, box, edges, _form=form)
            check_tables(out, tables, e, edges, box, rows_of(a), rows_of(b))
        assert np.array_equal(out["counts"], P.radial_counts(a, b, box, edges)["counts"])       # the count kernel's bits
        if pairs is not None:                                                                   # the stacked sum
            assert np.array_equal(tables.sum(axis=0), pairs)
        prof = P.velocity_profile(out["counts"], out["sums"], out["exponent"])
        want = V.derived(tables, e)
        assert prof["v_r"].shape == (rows_of(a), nb) and np.array_equal(prof["v_r"], want["v12"], equal_nan=True)
        assert np.array_equal(prof["sigma_r"], want["sigma_r"], equal_nan=True)
        assert np.array_equal(prof["sigma_t"], want["sigma_t"], equal_nan=True)


def test_what_the_edge_cases_are_about():
    """The shared cases do hold what their names say."""
    (_, _, _, _, box, edges), pairs, e, tables = reference("zero velocities")
    assert e == 0 and not pairs[:, 1:].any() and not tables[:, :, 1:].any() and pairs[:, 0].sum() > 1000
    for dt in ("float64", "float32"):
        (a, va, b, vb, _, _), pairs, e, _ = reference("one component at +-max %s" % dt)
        assert e == 8 and np.abs(V.words(vb, e)).max() == 1 << 20 == -V.words(vb, e).min() and pairs[:, 3].sum() > 0
    (a, va, b, vb, _, _), pairs, e, tables = reference("coincident rows, r_0 = 0")
    # a row of b on a row of a: q = 0, counted in bin 0 with vr = 0 and its own |dW|^2; each of the 40 points four times
    d = V.words(vb, e)[:, :, None] - V.words(va, e)[:, None, :]
    same = (np.arange(80)[:, None] % 40 == np.arange(80)[None, :] % 40)
    near = V.moments_of(a, va, L, (0.0, 1e-6), b, vb)[0]
    assert near[0, 0] == 160 == same.sum() and near[0, 1:4].tolist() == [0, 0, 0]
    assert near[0, 4] + (near[0, 5] << 24) == int((d * d).sum(axis=0)[same].sum()) > 0 and pairs[0, 0] >= 160
    (_, _, _, _, _, edges2), inner, _, _ = reference("coincident rows, r_0 = 2")
    assert edges2[0] == 2.0 and inner[:, 0].sum() > 0                        # with r_0 = 2 the coincident rows are in no bin
    (_, _, _, _, _, _), edge, _, _ = reference("edges hit exactly")
    assert edge[:, 0].sum() - 300 >= 480                                      # each of the 240 pairs on a threshold from both ends
    (_, va, _, _, _, _), _, _, tables = reference("centres at rest")
    assert va is None and tables[:, :, 1].any()
    (_, _, _, _, _, _), one, _, one_t = reference("H = 1, count_b = 1")
    assert one[:, 0].tolist() == [1, 0, 0, 0, 0] and one[0, 1:4].tolist() == [0, 0, 0] and one[0, 4] + (one[0, 5] << 24) > 0


@functools.lru_cache(maxsize=None)
def clustered(dtype):
    psi, vel = F.clustered_field(16).astype(dtype), F.velocity_field(16, 11).astype(dtype)
    return psi, vel, H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=20, velocity=vel)


@pytest.mark.parametrize("dtype", ["float32", "float16"])
def test_clustered_lattice_about_its_fof_halos(dtype):
    psi, vel, cat = clustered(dtype)
    assert len(cat["Length"]) >= 3
    edges = P.profile_edges(0.5, 20.0, 12)
    pos, cv = cat["CMPosition"], cat["CMVelocity"]
    ref, e = V.profiles_of(pos, cv, psi, vel, 100.0, edges)
    out = H.halo_velocity_profiles(cat, psi, vel, 100.0, edges)
    assert sorted(out) == sorted(PROFILE_KEYS + ["Length", "count", "v_r", "sigma_r", "sigma_t", "vr2", "vt2"])
    check_tables({k: out[k] for k in PROFILE_KEYS}, ref, e, edges, 100.0, len(pos), 4096)
    assert out["count"] == len(pos) and np.array_equal(out["Length"], cat["Length"])
    want = V.derived(ref, e)
    assert np.array_equal(out["v_r"], want["v12"], equal_nan=True) and np.array_equal(out["sigma_t"], want["sigma_t"], equal_nan=True)
    # the column sums of the per-centre sums: the cross moments of the centres with the matter
    cross = CF.pairwise_velocity(pos, cv, 100.0, edges, b=psi, vel_b=vel)
    assert np.array_equal(out["counts"].sum(axis=0), cross["npairs"]) and np.array_equal(out["sums"].sum(axis=0), cross["sums"])
    assert cross["exponent"] == e
    # a selection: the rows of the halos kept; the exponent is the call's own
    big = int(np.sort(cat["Length"])[-2])
    keep = cat["Length"] >= big
    sel = H.halo_velocity_profiles(cat, psi, vel, 100.0, edges, min_length=big)
    ref_sel, e_sel = V.profiles_of(pos[keep], cv[keep], psi, vel, 100.0, edges)
    assert sel["count"] == int(keep.sum()) < len(keep) and np.array_equal(sel["Length"], cat["Length"][keep])
    assert sel["exponent"] == e_sel and np.array_equal(sel["counts"], ref_sel[:, :, 0]) and np.array_equal(sel["sums"], ref_sel[:, :, 1:])
    # the groups of every size among themselves
    every = H.fof_halos(psi, boxsize=100.0, linking_length=0.2, nmin=1, velocity=vel)
    hedges = (0.0, 7.0, 9.5)                                                     # the lattice's first two shells
    hh = H.halo_pairwise_velocity(every, 100.0, hedges, max_length=19)
    few = every["Length"] <= 19
    ref_hh, e_hh = V.moments_of(every["CMPosition"][few], every["CMVelocity"][few], 100.0, hedges)
    assert hh["count"] == int(few.sum()) > 1000 and ref_hh[:, 0].min() > 1000
    check_pairs({k: hh[k] for k in PAIR_KEYS}, ref_hh, e_hh, hedges, 100.0, int(few.sum()), None)
    # stacked: the sum of the rows, then the same host arithmetic
    sc, ss, halos = P.stack_velocity_profiles(out["counts"], out["sums"], cat["Length"], (20, 10 ** 6))
    assert halos.tolist() == [len(pos)] and np.array_equal(sc[0], ref[:, :, 0].sum(axis=0)) and np.array_equal(ss[0], ref[:, :, 1:].sum(axis=0))
    assert np.array_equal(P.velocity_profile(sc, ss, e)["v_r"][0], V.derived(ref.sum(axis=0), e)["v12"], equal_nan=True)


def test_launch_geometry_forms_and_order():
    (a, va, b, vb, _, _), pairs, e, tables = reference("uniform cross float64")
    (p, v, _, _, _, _), auto, _, _ = reference("uniform auto float64")
    for blocks in (1, 3, None):
        for form in CF.VELOCITY_FORMS:
            out = CF.pairwise_velocity(p, v, L, EDGES, _max_blocks=blocks, _form=form)
            assert np.array_equal(out["npairs"], auto[:, 0]) and np.array_equal(out["sums"], auto[:, 1:])
            out = CF.pairwise_velocity(a, va, L, EDGES, b=b, vel_b=vb, _max_blocks=blocks, _form=form)
            assert np.array_equal(out["npairs"], pairs[:, 0]) and np.array_equal(out["sums"], pairs[:, 1:])
        for form in P.FORMS:
            out = P.radial_velocity_moments(a, va, b, vb, L, EDGES, _max_blocks=blocks, _form=form)
            assert np.array_equal(out["counts"], tables[:, :, 0]) and np.array_equal(out["sums"], tables[:, :, 1:])
    rng = np.random.default_rng(33)
    pa, pb = rng.permutation(300), rng.permutation(1500)
    out = CF.pairwise_velocity(p[pb], v[pb], L, EDGES)
    assert np.array_equal(out["npairs"], auto[:, 0]) and np.array_equal(out["sums"], auto[:, 1:])
    out = P.radial_velocity_moments(a[pa], va[pa], b[pb], vb[pb], L, EDGES)
    assert np.array_equal(out["counts"], tables[pa][:, :, 0]) and np.array_equal(out["sums"], tables[pa][:, :, 1:])
    swapped = CF.pairwise_velocity(b, vb, L, EDGES, b=a, vel_b=va)                # a <-> o: the terms of a pair are symmetric
    assert np.array_equal(swapped["npairs"], pairs[:, 0]) and np.array_equal(swapped["sums"], pairs[:, 1:])


def test_the_library_takes_both_profile_forms():
    """nbe_halo_velocity_profiles chooses as nbe_halo_profiles does: a wave per centre from 4096 centres on where the cells
    are sparse, else a workgroup.  4095, 4096 and 5000 centres with sparse cells against the restatement; 5000 with dense
    ones against both forms and, stacked, against the pair kernel."""
    centres, cv = R.uniform_points(5000, L, 6), V.gaussian_velocity((5000, 3), 51, scale=100.0)    # the matter sets the exponent
    matter, mv = R.uniform_points(), V.gaussian_velocity((1500, 3), 41)
    edges = (0.0, 2.0, 5.0)
    ref, e = V.profiles_of(centres, cv, matter, mv, L, edges)
    assert ref[:, :, 0].sum() > 1000
    for rows in (4095, 4096, 5000):
        out = P.radial_velocity_moments(centres[:rows], cv[:rows], matter, mv, L, edges)
        assert out["exponent"] == e == V.exponent(mv)
        assert np.array_equal(out["counts"], ref[:rows, :, 0]) and np.array_equal(out["sums"], ref[:rows, :, 1:]), rows
    for form in P.FORMS:
        out = P.radial_velocity_moments(centres, cv, matter, mv, L, edges, _form=form)
        assert np.array_equal(out["counts"], ref[:, :, 0]) and np.array_equal(out["sums"], ref[:, :, 1:])
    dense = [P.radial_velocity_moments(centres, cv, matter, mv, L, EDGES, _form=form) for form in (None,) + P.FORMS]
    for out in dense[1:]:
        assert np.array_equal(out["counts"], dense[0]["counts"]) and np.array_equal(out["sums"], dense[0]["sums"])
    cross = CF.pairwise_velocity(centres, cv, L, EDGES, b=matter, vel_b=mv)
    assert np.array_equal(dense[0]["counts"].sum(axis=0), cross["npairs"]) and np.array_equal(dense[0]["sums"].sum(axis=0), cross["sums"])
    assert np.array_equal(dense[0]["counts"], P.radial_counts(centres, matter, L, EDGES)["counts"])


def test_residency_and_streams():
    import torch
    (a, va, b, vb, _, _), pairs, e, tables = reference("uniform cross float64")
    ta, tva, tb, tvb = (torch.from_numpy(x.copy()).cuda() for x in (a, va, b, vb))
    out = CF.pairwise_velocity(ta, tva, L, EDGES, b=tb, vel_b=tvb)
    for k in ("npairs", "sums", "r_edges", "thresholds") + MOMENTS:
        assert isinstance(out[k], torch.Tensor) and out[k].device == ta.device, k
    assert out["npairs"].dtype == torch.int64 and np.array_equal(out["npairs"].cpu().numpy(), pairs[:, 0])
    assert np.array_equal(out["sums"].cpu().numpy(), pairs[:, 1:]) and out["exponent"] == e
    assert np.array_equal(out["v12"].cpu().numpy(), V.derived(pairs, e)["v12"])
    prof = P.radial_velocity_moments(ta, tva, tb, tvb, L, EDGES)
    for k in ("counts", "sums", "r_edges", "thresholds"):
        assert isinstance(prof[k], torch.Tensor) and prof[k].device == ta.device, k
    assert np.array_equal(prof["counts"].cpu().numpy(), tables[:, :, 0]) and np.array_equal(prof["sums"].cpu().numpy(), tables[:, :, 1:])
    assert np.array_equal(P.velocity_profile(prof["counts"], prof["sums"], prof["exponent"])["v_r"], V.derived(tables, e)["v12"],
                          equal_nan=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = CF.pairwise_velocity(ta, tva, L, EDGES, b=tb, vel_b=tvb)["sums"]
        rest = P.radial_velocity_moments(ta, None, tb, tvb, L, EDGES)["sums"]
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), pairs[:, 1:])
    assert np.array_equal(rest.cpu().numpy(), reference("centres at rest")[3][:, :, 1:])
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        CF.pairwise_velocity(ta, va, L, EDGES)
    with pytest.raises(ValueError, match="both be NumPy arrays or both tensors"):
        P.radial_velocity_moments(a, va, b, tvb, L, EDGES)


def test_a_velocity_that_is_not_finite_is_refused():
    (a, va, b, vb, _, _), _, _, _ = reference("uniform cross float64")
    for dt in (np.float64, np.float32):
        bad = vb.astype(dt)
        bad[17, 1] = np.nan
        bad[40, 2] = np.inf
        with pytest.raises(ValueError, match="pairwise_velocity: 2 value\\(s\\) of the velocity are not finite"):
            CF.pairwise_velocity(a, va, L, EDGES, b=b, vel_b=bad)
        with pytest.raises(ValueError, match="radial_velocity_moments: 2 value\\(s\\) of the velocity are not finite"):
            P.radial_velocity_moments(a, None, b, bad, L, EDGES)
    worse = va.copy()
    worse[0, 0] = -np.inf
    with pytest.raises(ValueError, match="1 value\\(s\\) of the velocity are not finite"):
        P.radial_velocity_moments(a, worse, b, vb, L, EDGES)
    far = a.copy()
    far[3, 0] = np.nan
    with pytest.raises(ValueError, match="1 row\\(s\\) have a non-finite position"):
        CF.pairwise_velocity(far, va, L, EDGES)
