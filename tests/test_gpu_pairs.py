"""Pair counts on the MI355X: correlation.pair_counts against the NumPy restatement of
tests/pairs_ref.py.  Counts are integers and are compared with ==, never with a tolerance."""

import functools

import numpy as np
import pytest

import fof_ref as F
import pairs_ref as R
from jax_nbody_emulator_with_dj_amd import correlation as CF, halos as H

pytestmark = pytest.mark.gpu

L, EDGES = R.UNIFORM_L, R.UNIFORM_EDGES


def ref_counts(a, b, boxsize, edges, nmu=None, los=2):
    T = R.thresholds(edges, boxsize)
    return R.pair_counts(R.catalogue(a, boxsize), T, None if b is None else R.catalogue(b, boxsize), nmu=nmu, los=los)


def check_dict(out, ref, edges, boxsize, count_a, count_b, nmu=None):
    assert out["npairs"].dtype == np.int64 and out["npairs"].shape == ref.shape and np.array_equal(out["npairs"], ref)
    assert out["r_edges"].dtype == np.float64 and np.array_equal(out["r_edges"], np.asarray(edges, np.float64))
    T = R.thresholds(edges, boxsize)
    assert out["thresholds"].dtype == np.int64 and out["thresholds"].tolist() == T
    assert out["ncell"] == R.ncell_of(T) and out["count_a"] == count_a and out["count_b"] == count_b
    if nmu is None:
        assert "mu_edges" not in out
    else:
        assert np.array_equal(out["mu_edges"], np.arange(nmu + 1) / nmu)


def test_lattice_shells_from_both_kinds_of_input():
    """Spacing a = L / 16: 3 N pairs at a, 6 N at sqrt(2) a, 4 N at sqrt(3) a, from positions and from a zero displacement."""
    N = R.LATTICE_N ** 3
    want = np.array([3 * N, 6 * N, 4 * N], np.int64)
    from_pos = CF.pair_counts(R.lattice_positions(), R.LATTICE_L, R.LATTICE_EDGES)
    check_dict(from_pos, want, R.LATTICE_EDGES, R.LATTICE_L, N, None)
    for dt in (np.float32, np.float16):
        from_disp = CF.pair_counts(np.zeros((3, 16, 16, 16), dt), R.LATTICE_L, R.LATTICE_EDGES)
        check_dict(from_disp, want, R.LATTICE_EDGES, R.LATTICE_L, N, None)
    cross = CF.pair_counts(R.lattice_positions().astype(np.float32), R.LATTICE_L, R.LATTICE_EDGES,
                           b=np.zeros((3, 16, 16, 16), np.float32))
    check_dict(cross, 2 * want, R.LATTICE_EDGES, R.LATTICE_L, N, N)


@pytest.mark.parametrize("dtype", ["float64", "float32"])
def test_uniform_points_several_boxes_away(dtype):
    """ncell = 3: every offset wraps.  Auto, cross, cross(A, A) = 2 auto(A) for r_0 > 0 and the partition identity."""
    pos, X, T, auto = R.uniform_case(dtype)
    assert R.ncell_of(T) == 3
    out = CF.pair_counts(pos, L, EDGES)
    check_dict(out, auto, EDGES, L, 1500, None)
    a1, a2 = pos[:600], pos[600:]
    cross = CF.pair_counts(a1, L, EDGES, b=a2)
    check_dict(cross, R.pair_counts(X[:, :600], T, X[:, 600:]), EDGES, L, 600, 900)
    parts = CF.pair_counts(a1, L, EDGES)["npairs"] + CF.pair_counts(a2, L, EDGES)["npairs"] + cross["npairs"]
    assert np.array_equal(parts, auto)
    assert np.array_equal(CF.pair_counts(a2, L, EDGES, b=a1)["npairs"], cross["npairs"])
    inner = EDGES[1:]
    assert np.array_equal(CF.pair_counts(pos, L, inner, b=pos)["npairs"], 2 * CF.pair_counts(pos, L, inner)["npairs"])
    assert np.array_equal(CF.pair_counts(pos, L, inner)["npairs"], auto[1:])
    with_self = CF.pair_counts(pos, L, EDGES, b=pos)["npairs"]                 # r_0 = 0: every row meets itself
    assert with_self[0] == 2 * auto[0] + 1500 and np.array_equal(with_self[1:], 2 * auto[1:])


def test_mixed_precision_and_kinds_of_catalogue():
    pos = R.uniform_points()
    a, b = pos[:500].astype(np.float32), pos[500:1100]
    assert np.array_equal(CF.pair_counts(a, L, EDGES, b=b)["npairs"], ref_counts(a, b, L, EDGES))
    psi = F.clustered_field(16, L)
    edges = (0.0, 1.25, 4.0, 9.0)
    got = CF.pair_counts(psi, L, edges, b=b, nmu=2)
    check_dict(got, ref_counts(psi, b, L, edges, nmu=2), edges, L, 4096, 600, nmu=2)
    assert np.array_equal(CF.pair_counts(b, L, edges, b=psi, nmu=2)["npairs"], got["npairs"])


@functools.lru_cache(maxsize=None)
def mu_reference(nmu, los):
    pos = R.uniform_points()[:700]
    ref = ref_counts(pos, None, L, EDGES, nmu=nmu, los=los)
    ref.setflags(write=False)
    return pos, ref


@pytest.mark.parametrize("nmu", [5, 32])
@pytest.mark.parametrize("los", [0, 1, 2])
def test_mu_bins_equal_the_reference(nmu, los):
    pos, ref = mu_reference(nmu, los)
    out = CF.pair_counts(pos, L, EDGES, nmu=nmu, los=los)
    check_dict(out, ref, EDGES, L, 700, None, nmu=nmu)
    plain = CF.pair_counts(pos, L, EDGES)["npairs"]
    assert np.array_equal(out["npairs"].sum(axis=1), plain)
    one = CF.pair_counts(pos, L, EDGES, nmu=1, los=los)
    assert one["npairs"].shape == (5, 1) and np.array_equal(one["npairs"][:, 0], plain)
    cross = CF.pair_counts(pos[:300], L, EDGES, b=pos[300:], nmu=nmu, los=los)["npairs"]
    assert np.array_equal(cross, ref_counts(pos[:300], pos[300:], L, EDGES, nmu=nmu, los=los))


@pytest.mark.parametrize("los", [0, 1, 2])
def test_mu_of_pairs_along_and_across_the_line_of_sight(los):
    """Four rows: 0 and 1 are 3 apart along `los` (mu = 1: the last bin), 0 and 2 are 7 apart across it (mu = 0: the first),
    2 and 3 coincide (d^2 = 0: bin 0), and 1 and 2 lie at mu = 3 / sqrt(58)."""
    other = (los + 1) % 3
    pos = np.full((4, 3), 50.0)
    pos[1, los] += 3.0
    pos[2, other] += 7.0
    pos[3] = pos[2]
    edges, nmu = (0.0, 1.0, 4.0, 7.5, 9.0), 8
    got = CF.pair_counts(pos, 100.0, edges, nmu=nmu, los=los)["npairs"]
    want = np.zeros((4, nmu), np.int64)
    want[0, 0] += 1                                      # the coincident rows
    want[1, nmu - 1] += 1                                # along
    want[2, 0] += 2                                      # across, from both coincident rows
    want[3, int(nmu * 3.0 / np.sqrt(58.0))] += 2         # |d| = sqrt(58) = 7.6
    assert np.array_equal(got, want)
    assert np.array_equal(got, ref_counts(pos, None, 100.0, edges, nmu=nmu, los=los))
    cross = CF.pair_counts(pos, 100.0, edges, b=pos, nmu=nmu, los=los)["npairs"]
    assert cross[0, 0] == 4 + 2 and cross.sum() == 4 + 2 * want.sum()       # every row with itself, then both orders


def test_pairs_on_a_threshold_fall_in_the_lower_bin():
    pos = R.edge_points()
    X, T = R.coordinates(pos, R.EDGE_L), R.thresholds(R.EDGE_EDGES, R.EDGE_L)
    d2 = (F.min_image(X[:, :, None] - X[:, None, :]) ** 2).sum(axis=0)
    on = [int((d2 == t).sum()) // 2 for t in T[1:]]
    assert min(on) >= 60
    ref = R.pair_counts(X, T)
    for dt in (np.float64, np.float32):                                       # multiples of L 2^-10 are exact in both
        assert np.array_equal(CF.pair_counts(pos.astype(dt), R.EDGE_L, R.EDGE_EDGES)["npairs"], ref)
    # with every edge a hair shorter the thresholds fall by at least one and exactly the pairs on them move up a bin
    short = [0.0] + [r * (1.0 - 2.0 ** -40) for r in R.EDGE_EDGES[1:]]
    moved = CF.pair_counts(pos, R.EDGE_L, short)["npairs"]
    assert np.array_equal(moved, R.pair_counts(X, R.thresholds(short, R.EDGE_L)))
    assert (ref - moved).tolist() == [on[0], on[1] - on[0], on[2] - on[1], on[3] - on[2]]
    binned = CF.pair_counts(pos, R.EDGE_L, R.EDGE_EDGES, nmu=4, los=0)["npairs"]
    assert np.array_equal(binned, R.pair_counts(X, T, nmu=4, los=0))


@functools.lru_cache(maxsize=None)
def one_cell_case():
    """1000 points inside one of 499 cells per axis (several LDS tiles, a run longer than a workgroup), and 300 more in
    the cell beside it along the last axis."""
    rng = np.random.default_rng(21)
    width = 100.0 / 499
    lo = np.array([50, 50, 50]) * width
    pos = np.concatenate([lo + rng.uniform(0.02, 0.98, size=(1000, 3)) * width,
                          lo + np.array([0.0, 0.0, width]) + rng.uniform(0.02, 0.98, size=(300, 3)) * width])
    edges = (0.0, 0.05, 0.1, 0.2)
    X = R.coordinates(pos, 100.0)
    assert R.ncell_of(R.thresholds(edges, 100.0)) == 499
    assert len(set(map(tuple, ((X[:, :1000] * 499) >> 30).T.tolist()))) == 1
    return pos, edges, ref_counts(pos, None, 100.0, edges), ref_counts(pos[:1000], None, 100.0, edges)


def test_degenerate_occupancies():
    pos, edges, ref_all, ref_cell = one_cell_case()
    assert np.array_equal(CF.pair_counts(pos[:1000], 100.0, edges)["npairs"], ref_cell)
    assert np.array_equal(CF.pair_counts(pos, 100.0, edges)["npairs"], ref_all)
    assert np.array_equal(CF.pair_counts(pos[:1000], 100.0, edges, b=pos[1000:])["npairs"],
                          ref_counts(pos[:1000], pos[1000:], 100.0, edges))
    rng = np.random.default_rng(22)
    few = rng.uniform(0.0, 100.0, size=(10, 3))
    few[1] = few[0] + [0.004, 0.0, 0.0]
    few[3] = few[2] - [0.0, 0.011, 0.009]
    out = CF.pair_counts(few, 100.0, (0.0, 0.01, 0.02))
    assert out["ncell"] == 4096 and out["npairs"].tolist() == [1, 1]
    one = CF.pair_counts(np.array([[1.0, 2.0, 3.0]]), 100.0, (0.0, 1.0), nmu=3)
    assert one["npairs"].tolist() == [[0, 0, 0]] and one["count_a"] == 1
    assert CF.pair_counts(np.array([[1.0, 2.0, 3.0]]), 100.0, (0.0, 1.0), b=few)["npairs"].tolist() == [0]
    assert CF.pair_counts(np.array([[1.0, 2.0, 3.0]]), 100.0, (0.0, 1.0), b=np.array([[1.0, 2.0, 3.5]]))["npairs"].tolist() == [1]


def test_one_bin_and_the_largest_image():
    pos = R.uniform_points()[:500]
    X = R.coordinates(pos, L)
    assert CF.pair_counts(pos, L, (3.0, 17.0))["npairs"].tolist() == R.pair_counts(X, R.thresholds((3.0, 17.0), L)).tolist()
    edges = np.linspace(0.0, 30.0, 129)
    T = R.thresholds(edges, L)
    out = CF.pair_counts(pos, L, edges)
    assert out["npairs"].shape == (128,) and np.array_equal(out["npairs"], R.pair_counts(X, T))
    full = CF.pair_counts(pos, L, edges, nmu=32, los=1)                       # 4096 counters: the whole 32 KiB image
    assert full["npairs"].shape == (128, 32) and np.array_equal(full["npairs"], R.pair_counts(X, T, nmu=32, los=1))


def test_same_bits_for_every_order_geometry_kind_and_stream():
    import torch
    pos, X, T, auto = R.uniform_case()
    perm = np.random.default_rng(4).permutation(1500)
    assert np.array_equal(CF.pair_counts(np.ascontiguousarray(pos[perm]), L, EDGES)["npairs"], auto)
    cell_pos, cell_edges, cell_ref, _ = one_cell_case()
    for blocks in (1, 3, None):
        assert np.array_equal(CF.pair_counts(pos, L, EDGES, _max_blocks=blocks)["npairs"], auto)
        assert np.array_equal(CF.pair_counts(cell_pos, 100.0, cell_edges, _max_blocks=blocks)["npairs"], cell_ref)
    mu_pos, mu_ref = mu_reference(5, 2)
    t = torch.from_numpy(pos).cuda()
    out = CF.pair_counts(t, L, EDGES)
    assert all(torch.is_tensor(out[k]) and out[k].is_cuda for k in ("npairs", "r_edges", "thresholds"))
    assert out["npairs"].dtype == torch.int64 and np.array_equal(out["npairs"].cpu().numpy(), auto)
    stream = torch.cuda.Stream()
    with torch.cuda.stream(stream):
        tm = torch.from_numpy(np.array(mu_pos)).cuda()
        on_stream = CF.pair_counts(tm, L, EDGES, nmu=5)
    stream.synchronize()
    assert np.array_equal(on_stream["npairs"].cpu().numpy(), mu_ref) and on_stream["mu_edges"].is_cuda


@pytest.mark.parametrize("form", [0, 1, 2, 3])
def test_every_form_of_the_kernel_counts_the_same(form):
    """Both histogram forms and both decompositions (nbe_pair_count_form), on the dense cell and on the sparse catalogue."""
    cell_pos, cell_edges, cell_ref, _ = one_cell_case()
    mu_pos, mu_ref = mu_reference(5, 2)
    pos, X, T, auto = R.uniform_case()
    for a, b, box, edges, nmu, ref in ((cell_pos, None, 100.0, cell_edges, None, cell_ref), (mu_pos, None, L, EDGES, 5, mu_ref),
                                       (pos[:600], pos[600:], L, EDGES, None, R.pair_counts(X[:, :600], T, X[:, 600:]))):
        A, B, box, e, T_, ncell, nm, los, blocks = CF._validate(a, box, edges, b, nmu, 2, None)
        got = CF._count(A, B, box, T_, ncell, nm or 1, los, blocks, form=form).cpu().numpy()
        assert np.array_equal(got if nmu else got[:, 0], ref)


def test_auto_count_to_the_linking_length_is_the_number_of_fof_links():
    psi = F.clustered_field(16)
    ell = 0.2 * 100.0 / 16
    links = F.linked_pairs(F.coordinates(psi, 100.0), F.r2_of(ell, 100.0)).shape[1]
    out = CF.pair_counts(psi, 100.0, [0.0, ell])
    assert links > 1000 and out["npairs"].tolist() == [links] and out["count_a"] == 4096


def test_bad_positions_raise():
    pos = np.array(R.uniform_points()[:100])
    for bad in (float("nan"), float("inf"), 100.0 * 2.0 ** 20, -100.0 * 2.0 ** 20):
        p = pos.copy()
        p[17, 1] = bad
        with pytest.raises(ValueError, match="1 row\\(s\\) have a non-finite position"):
            CF.pair_counts(p, L, EDGES)
        with pytest.raises(ValueError, match="non-finite position"):
            CF.pair_counts(pos, L, EDGES, b=p.astype(np.float32))
    p = pos.copy()
    p[3, 0] = 100.0 * (2.0 ** 20 - 1.0)                                        # the last box that is taken
    assert np.array_equal(CF.pair_counts(p, L, EDGES)["npairs"], ref_counts(p, None, L, EDGES))
    psi = np.zeros((3, 4, 4, 4), np.float32)
    psi[1, 2, 2, 2] = np.nan
    with pytest.raises(ValueError, match="non-finite position"):
        CF.pair_counts(psi, L, (0.0, 30.0))


def test_correlation_function_and_halo_correlation():
    psi, box, v, kw, ref = F.case("clustered16")
    cat = H.fof_halos(psi, boxsize=box, velocity=v, linking_length=0.2, nmin=1)      # every group, the single particles included
    edges = np.array([0.0, 10.0, 20.0, 30.0])
    sel = np.asarray(cat["Length"]) <= 1
    centres = cat["CMPosition"][sel]
    assert 1000 <= sel.sum() < len(sel)
    dd = CF.pair_counts(centres, box, edges)
    hh = H.halo_correlation(cat, box, edges, max_length=1)
    assert hh["count"] == int(sel.sum()) and np.array_equal(hh["npairs"], dd["npairs"])
    want = R.estimator(dd["npairs"], edges, box, int(sel.sum()))
    for k in ("rr", "xi", "r_mid"):
        np.testing.assert_allclose(hh[k], want[k], rtol=1e-13, atol=0)
    hm = H.halo_correlation(cat, box, edges, matter=psi, max_length=1, nmu=4, los=0)
    dm = CF.pair_counts(centres, box, edges, b=psi, nmu=4, los=0)
    assert np.array_equal(hm["npairs"], dm["npairs"]) and hm["count_b"] == 4096
    assert np.array_equal(dm["npairs"], ref_counts(centres, psi, box, edges, nmu=4, los=0))
    want = R.estimator(dm["npairs"], edges, box, int(sel.sum()), 4096, nmu=4)
    for k in ("rr", "xi", "xi0", "xi2", "xi4"):
        np.testing.assert_allclose(hm[k], want[k], rtol=1e-13, atol=1e-13 * np.abs(want["xi"]).max() if k[2:] else 0)
    shifted = np.array(centres)
    shifted[:, 1] += 0.01 * cat["CMVelocity"][sel][:, 1]
    rs = H.halo_correlation(cat, box, edges, max_length=1, redshift_space=True, los=1, velocity_to_length=0.01)
    assert np.array_equal(rs["npairs"], CF.pair_counts(shifted, box, edges)["npairs"])
