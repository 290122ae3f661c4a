"""CPU: the definition of the pairwise velocity moments as tests/pairvel_ref.py restates it, held to
direct float64 computations, to its own exact rule and to analytic cases; the host arithmetic of correlation.velocity_moments
and profiles.velocity_profile; and the validation of the public functions, which runs before any device work."""

import math

import numpy as np
import pytest

import fof_ref as F
import pairs_ref as R
import pairvel_ref as V
from jax_nbody_emulator_with_dj_amd import _lib, correlation as CF, halos as H, profiles as P

SQRT3 = math.sqrt(3.0)


def dyadic_points(count, seed, L=64.0, span=1 << 10):
    """count distinct points on multiples of L / 1024: their coordinates are exact, and two of them are 2^20 units or more
    apart."""
    rng = np.random.default_rng(seed)
    cells = rng.choice(span ** 3, size=count, replace=False)
    return np.stack([cells // span ** 2, cells // span % span, cells % span], axis=1).astype(np.float64) * (L / span)


def grid_cube(count, seed, lo, hi, L=100.0):
    """count distinct points on multiples of L / 1024 with every coordinate in [lo, hi) cells: exact coordinates, exact
    differences, and for hi - lo < 512 no pair that wraps."""
    rng = np.random.default_rng(seed)
    span = hi - lo
    cells = rng.choice(span ** 3, size=count, replace=False)
    return (lo + np.stack([cells // span ** 2, cells // span % span, cells % span], axis=1)).astype(np.float64) * (L / 1024.0)


def random_words(pairs, seed):
    """(d, dW) (3, pairs) int64: separations up to 2^28 a component, word differences up to 2^21."""
    rng = np.random.default_rng(seed)
    return rng.integers(-(1 << 28), (1 << 28) + 1, size=(3, pairs)), rng.integers(-(1 << 21), (1 << 21) + 1, size=(3, pairs))


def test_radial_word_against_float64_on_separated_points():
    """vr 2^(e - 20) against dv . d_hat in float64: the words are off by at most 1/2 a component of each row, so dW . d_hat is
    off by at most |eps| <= sqrt(3), and the radial word adds its own 1/2."""
    L = 64.0
    pos, vel = dyadic_points(300, 1), V.gaussian_velocity((300, 3), 2)
    e = V.exponent(vel)
    X, W = R.coordinates(pos, L), V.words(vel, e)
    ii, jj = np.triu_indices(300, 1)
    d = F.min_image(X[:, jj] - X[:, ii])
    vr, vr2, dw2 = V.terms(d, W[:, jj] - W[:, ii])
    dhat = d / np.sqrt((d * d).sum(axis=0).astype(np.float64))
    direct = ((vel[jj] - vel[ii]).T * dhat).sum(axis=0)
    unit = math.ldexp(1.0, e - V.BITS)
    err = np.abs(vr * unit - direct).max()
    print("max |vr 2^(e - 20) - dv . d_hat| = %.3e, bound %.3e" % (err, (0.5 + SQRT3) * unit))
    assert err <= (0.5 + SQRT3) * unit
    assert np.array_equal(vr2, vr * vr) and np.array_equal(dw2, ((W[:, jj] - W[:, ii]) ** 2).sum(axis=0))
    dv2 = ((vel[jj] - vel[ii]) ** 2).sum(axis=1)
    assert np.abs(dw2 * unit * unit - dv2).max() <= (2.0 * SQRT3 * np.sqrt(dv2).max() + 3.0 * unit) * unit


def test_exact_rule_equals_float64_rint_and_has_no_tie():
    d, dW = random_words(200000, 3)
    q, u = (d * d).sum(axis=0), (dW * d).sum(axis=0)
    assert int(np.abs(u).max()) < 1 << 52 and int(q.max()) < 1 << 60
    vr = np.rint(u.astype(np.float64) / np.sqrt(q.astype(np.float64))).astype(np.int64)
    for uu, qq, vv in zip(u.tolist(), q.tolist(), vr.tolist()):
        k = abs(V.vr_exact(uu, qq))
        assert V.vr_exact(uu, qq) == vv and not V.is_tie(uu, qq)
        assert (2 * k - 1) ** 2 * qq <= 4 * uu * uu < (2 * k + 1) ** 2 * qq or (k == 0 and 4 * uu * uu < qq)
    assert int(np.abs(vr).max()) < 1 << 23 and int((vr * vr).max()) < 1 << 44 and int((dW * dW).sum(axis=0).max()) < 1 << 44


def test_no_tie_for_small_integers_exhaustively():
    """4 u^2 = (2 k + 1)^2 q with u != 0 needs sqrt(q) = 2 |u| / (2 k + 1) rational, hence an integer, and even (its odd
    multiple is even), so q = 0 mod 4 and every d_c is even (squares are 0 or 1 mod 4); halving d halves u and sqrt(q) and
    keeps the tie, and the descent ends at d = 0.  Every d in -4 .. 4 and dW in -3 .. 3 per component: no tie; and the
    detector does find the ties of pairs (u, q) that no integer d yields."""
    assert V.is_tie(1, 4) and V.is_tie(3, 4) and V.is_tie(5, 100) and not V.is_tie(2, 4) and not V.is_tie(1, 3)
    g = np.arange(-4, 5)
    d = np.stack(np.meshgrid(g, g, g, indexing="ij")).reshape(3, -1)
    w = np.stack(np.meshgrid(g[1:-1], g[1:-1], g[1:-1], indexing="ij")).reshape(3, -1)
    q = (d * d).sum(axis=0)[:, None]
    u = (d[:, :, None] * w[:, None, :]).sum(axis=0)
    ok = (q > 0) & (u != 0)
    m = np.where(ok, 4 * u * u // np.maximum(q, 1), 0)
    root = np.rint(np.sqrt(m.astype(np.float64))).astype(np.int64)
    tie = ok & (4 * u * u % np.maximum(q, 1) == 0) & (root * root == m) & (root % 2 == 1)
    assert ok.sum() > 200000 and not tie.any()


def test_terms_are_symmetric_under_swapping_the_rows():
    d, dW = random_words(2000, 4)
    for x, y in zip(V.terms(d, dW), V.terms(-d, -dW)):
        assert np.array_equal(x, y)
    pos, vel = R.uniform_points()[:400], V.gaussian_velocity((400, 3), 5)
    e = V.exponent(vel)
    X, W, T = R.coordinates(pos, R.UNIFORM_L), V.words(vel, e), R.thresholds(R.UNIFORM_EDGES, R.UNIFORM_L)
    ab = V.pair_velocity(X[:, :150], W[:, :150], T, X[:, 150:], W[:, 150:])
    assert np.array_equal(ab, V.pair_velocity(X[:, 150:], W[:, 150:], T, X[:, :150], W[:, :150]))
    auto = V.pair_velocity(X, W, T)
    rows = np.zeros((5, 6), np.int64)
    rows[0, 0] = 400                                                             # a row with itself: q = 0, in bin 0, all terms 0
    assert np.array_equal(V.pair_velocity(X, W, T, X, W), 2 * auto + rows)       # every pair from both ends
    assert np.array_equal(auto[:, 0], R.pair_counts(X, T))
    perm = np.random.default_rng(6).permutation(400)
    assert np.array_equal(V.pair_velocity(X[:, perm], W[:, perm], T), auto)


def test_overflow_bound_and_host_arithmetic():
    top = 3 * (1 << 21) ** 2                                                     # |dW|^2 at its largest; k <= |dW| + 1/2
    assert top < 1 << 44 and (math.isqrt(top) + 1) ** 2 < 1 << 44 and math.isqrt(top) + 1 < 1 << 23
    n = CF.MAX_PAIRS_PER_BIN
    assert n == 1 << 39 == V.MAX_PAIRS
    assert n * (top >> V.SPLIT) < 1 << 63 and n * V.MASK < 1 << 63 and n * (math.isqrt(top) + 1) < 1 << 63
    CF.check_pairs_per_bin(np.array([0, n]), "x")
    with pytest.raises(_lib.NBEError, match="exceed 2\\^39"):
        CF.check_pairs_per_bin(np.array([3, n + 1]), "x")
    # the largest table the split allows: float64 from the exact integers
    sums = np.array([[n, -n * 1000, n * 5, n * 7, n * 11, n * 13], [0, 0, 0, 0, 0, 0]], np.int64)
    got = CF.velocity_moments(sums[:, 0], sums[:, 1:], 10)
    want = V.derived(sums, 10)
    for k in want:
        assert np.array_equal(got[k], want[k], equal_nan=True), k
    assert got["v12"][0] == -1000.0 * 2.0 ** -10 and np.isnan(got["v12"][1]) and np.isnan(got["sigma_t"][1])
    assert got["vr2"][0] == (7 * 2.0 ** 24 + 5) * 4.0 ** -10
    prof = P.velocity_profile(sums[None, :, 0], sums[None, :, 1:], 10)
    assert prof["v_r"].shape == (1, 2) and np.array_equal(prof["v_r"][0], got["v12"], equal_nan=True)
    assert sorted(prof) == ["sigma_r", "sigma_t", "v_r", "vr2", "vt2"]
    assert V.exponent(np.zeros((4, 3))) == 0 and V.exponent(np.array([[0.5, 0, 0]])) == 0 and V.exponent(np.array([[1.0, 0, -3]])) == 2
    with pytest.raises(ValueError):
        V.exponent(np.array([[np.inf, 0, 0]]))


def test_stacked_profiles_are_sums_of_rows():
    rng = np.random.default_rng(7)
    counts, sums = rng.integers(0, 50, size=(9, 4)), rng.integers(-1000, 1000, size=(9, 4, 5))
    lengths = np.array([5, 9, 20, 21, 40, 41, 99, 100, 7])
    sc, ss, halos = P.stack_velocity_profiles(counts, sums, lengths, (10, 41, 100))
    assert halos.tolist() == [3, 2] and np.array_equal(sc[0], counts[2:5].sum(axis=0)) and np.array_equal(ss[1], sums[5:7].sum(axis=0))
    one = P.velocity_profile(sc, ss, 3)
    assert one["v_r"].shape == (2, 4)
    with pytest.raises(ValueError, match="stack_velocity_profiles"):
        P.stack_velocity_profiles(counts, sums[:, :, :4], lengths, (10, 41))


def test_hubble_flow_streams_at_H_r_with_no_transverse_dispersion():
    """v = H x on grid points inside a cube of side below L / 2 (no pair wraps; positions, differences and velocities are
    exact): dv . d_hat = H r for every pair, so v12 = H <r> per bin and the transverse moment vanishes, both to the rounding
    of the words: |v12 - H <r>| <= B = (1/2 + sqrt(3)) 2^(e - 20); and with |dW| off by at most sqrt(3) and vr by at most
    B / unit, |vt2| <= (2 sqrt(3) unit H r + 3 unit^2 + 2 B H r + B^2) / 2."""
    L, Hub = 100.0, 10.0
    pos = grid_cube(400, 9, 52, 460)
    vel = Hub * pos
    edges = np.array([0.0, 4.0, 9.0, 15.0, 22.0, 30.0])
    sums, e = V.moments_of(pos, vel, L, edges)
    out = V.derived(sums, e)
    X, T = R.coordinates(pos, L), R.thresholds(edges, L)
    ii, jj = np.triu_indices(400, 1)
    d = X[:, jj] - X[:, ii]                                                      # nothing wraps
    assert np.array_equal(d, F.min_image(d))
    q = (d * d).sum(axis=0)
    b = np.searchsorted(np.array(T), q, side="left") - 1
    r = np.sqrt(q.astype(np.float64)) * (L / R.U)
    unit = math.ldexp(1.0, e - V.BITS)
    bound = (0.5 + SQRT3) * unit
    for k in range(5):
        sel = b == k
        assert sel.sum() == sums[k, 0] > 100
        assert abs(out["v12"][k] - Hub * r[sel].mean()) <= bound
        rmax = r[sel].max()
        vt_bound = 0.5 * (2.0 * SQRT3 * unit * Hub * rmax + 3.0 * unit * unit + 2.0 * bound * Hub * rmax + bound * bound)
        assert abs(out["vt2"][k]) <= vt_bound and out["sigma_t"][k] <= math.sqrt(vt_bound)
        assert out["sigma_r"][k] > 0.0 and out["v12"][k] > 0.0
    print("v12 - H <r> =", out["v12"] - np.array([Hub * r[b == k].mean() for k in range(5)]), "bound", bound)


def test_rigid_rotation_has_no_radial_motion():
    """v = omega x (x - c) on grid points (exact differences): dv . d = 0 for every pair, so every radial word is within the
    rounding of the words of 0 and all the motion is transverse."""
    L = 100.0
    pos = grid_cube(200, 10, 300, 620)
    vel = np.cross(np.array([0.25, -1.0, 2.0]), pos - 45.0)
    sums, e = V.moments_of(pos, vel, L, (0.0, 10.0, 25.0))
    out = V.derived(sums, e)
    unit = math.ldexp(1.0, e - V.BITS)
    assert np.abs(out["v12"]).max() <= (0.5 + SQRT3) * unit and out["vr2"].max() <= ((0.5 + SQRT3) * unit) ** 2
    assert (out["sigma_t"] > 100.0 * unit).all()


def test_validation_comes_before_any_device_work():
    pos, vel = R.uniform_points()[:20], V.gaussian_velocity((20, 3), 11)
    psi = np.zeros((3, 4, 4, 4), np.float32)
    E = R.UNIFORM_EDGES
    for call, match in (
            (lambda: CF.pairwise_velocity(pos, vel[:19], 100.0, E), "vel_a must have its catalogue's shape"),
            (lambda: CF.pairwise_velocity(pos, vel.astype(np.float16), 100.0, E), "vel_a must be float32 or float64"),
            (lambda: CF.pairwise_velocity(psi, psi.astype(np.float64), 100.0, E), "vel_a must be float32 or float16"),
            (lambda: CF.pairwise_velocity(pos, vel.tolist(), 100.0, E), "vel_a must be a NumPy array or a CUDA torch tensor"),
            (lambda: CF.pairwise_velocity(pos, vel, 100.0, E, b=pos), "b and vel_b go together"),
            (lambda: CF.pairwise_velocity(pos, vel, 100.0, E, vel_b=vel), "b and vel_b go together"),
            (lambda: CF.pairwise_velocity(pos, vel, 100.0, E, b=psi, vel_b=vel), "vel_b must have its catalogue's shape"),
            (lambda: CF.pairwise_velocity(pos, vel, 100.0, E, _form=2), "_form must be None or one of"),
            (lambda: CF.pairwise_velocity(pos, vel, 100.0, E, _max_blocks=0), "_max_blocks must be an int >= 1"),
            (lambda: CF.pairwise_velocity(pos, vel, 100.0, (0.0, 40.0)), "must stay below L / 3"),
            (lambda: CF.pairwise_velocity(pos[:, :2], vel, 100.0, E), "must be \\(count, 3\\) positions"),
            (lambda: P.radial_velocity_moments(psi, None, pos, vel, 100.0, E), "centres must be \\(H, 3\\) positions"),
            (lambda: P.radial_velocity_moments(pos, vel[:3], pos, vel, 100.0, E), "centre_velocity must have its catalogue's shape"),
            (lambda: P.radial_velocity_moments(pos, vel, pos, None, 100.0, E), "matter_velocity must be a NumPy array"),
            (lambda: P.radial_velocity_moments(pos, None, psi, psi.astype(np.float64), 100.0, E), "matter_velocity must be float32 or float16"),
            (lambda: P.radial_velocity_moments(pos, None, pos, vel, 100.0, E, _form=2), "_form must be None, 0 or 1"),
            (lambda: CF.velocity_moments(np.zeros(3, np.int64), np.zeros((3, 4), np.int64), 1), "sums its \\(\\.\\.\\., 5\\) sums"),
            (lambda: CF.velocity_moments(np.zeros(3), np.zeros((3, 5), np.int64), 1), "integer table"),
            (lambda: CF.velocity_moments(np.zeros(3, np.int64), np.zeros((3, 5), np.int64), 1.5), "exponent must be an int")):
        with pytest.raises(ValueError, match=match):
            call()
    cat = {"CMPosition": pos, "Length": np.arange(20) + 5}
    with pytest.raises(ValueError, match="halo_velocity_profiles needs a catalogue with CMVelocity"):
        H.halo_velocity_profiles(cat, pos, vel, 100.0, E)
    with pytest.raises(ValueError, match="halo_pairwise_velocity needs a catalogue with CMVelocity"):
        H.halo_pairwise_velocity(cat, 100.0, E)
    cat["CMVelocity"] = vel
    with pytest.raises(ValueError, match="no halo is left by the selection"):
        H.halo_pairwise_velocity(cat, 100.0, E, min_length=1000)


def test_the_entry_points_are_declared_and_bound():
    assert "nbe_pairvel.hip" in _lib.SOURCES
    header = open(_lib.os.path.join(_lib._HERE, "..", "include", "nbe.h")).read()
    for name in ("nbe_velocity_words", "nbe_pair_velocity", "nbe_pair_velocity_form", "nbe_halo_velocity_profiles",
                 "nbe_halo_velocity_profiles_form"):
        assert "int %s(" % name in header
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["nbe_pair_velocity_form"][1][:12] == _lib.SIGNATURES["nbe_pair_velocity"][1][:12]
    assert _lib.SIGNATURES["nbe_halo_velocity_profiles_form"][1][:12] == _lib.SIGNATURES["nbe_halo_velocity_profiles"][1][:12]
    assert "#define NBE_VELOCITY_BITS %d" % CF.VELOCITY_BITS in header and V.BITS == CF.VELOCITY_BITS and V.SPLIT == CF.VELOCITY_SPLIT
