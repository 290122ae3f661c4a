"""NumPy restatement of jax_nbody_emulator_with_dj_amd.profiles: brute-force (H, count) int64 d^2
between centres and matter with the coordinates and thresholds of tests/pairs_ref.py, the bin searchsorted(T, q, "left") - 1,
and the spherical-overdensity definition written out one halo at a time.  The GPU tests compare the counts with it exactly;
tests/test_profiles_host.py compares it with scipy's periodic cKDTree.

Everything that decides a bin is an integer, so this file and the kernel must agree bit for bit."""

import functools
import math

import numpy as np

import fof_ref as F
import pairs_ref as R


def radial_counts(XA, XB, T, chunk=128):
    """int64 (H, nb): the rows of XB (3, count) in each bin about every column of XA (3, H)."""
    nb = len(T) - 1
    Tarr = np.array(T, dtype=np.int64)
    out = np.zeros((XA.shape[1], nb), np.int64)
    for lo in range(0, XA.shape[1], chunk):
        hi = min(XA.shape[1], lo + chunk)
        d = F.min_image(XA[:, lo:hi, None] - XB[:, None, :])
        q = (d * d).sum(axis=0)
        b = np.searchsorted(Tarr, q, side="left") - 1                       # T[b] < q <= T[b + 1]; -1 or nb: in no bin
        for h in range(lo, hi):
            row = b[h - lo]
            out[h] = np.bincount(row[(row >= 0) & (row < nb)], minlength=nb)
    return out


def counts_of(centres, matter, L, edges):
    """radial_counts of two catalogues of either kind."""
    return radial_counts(R.catalogue(centres, L), R.catalogue(matter, L), R.thresholds(edges, L))


def omega_m(Om, z):
    return Om * (1.0 + z) ** 3 / (Om * (1.0 + z) ** 3 + 1.0 - Om)


def spherical_overdensity(counts, r_edges, L, count_b, overdensity=200.0, reference="mean", Om=None, z=0.0):
    """(R, N, flag, delta) of every row, with Python floats and one loop per halo."""
    e = [float(r) for r in r_edges]
    assert e[0] == 0.0
    nbar = count_b / float(L) ** 3
    delta = float(overdensity) if reference == "mean" else float(overdensity) / omega_m(Om, z)
    Rs, Ns, flags = [], [], []
    for row in np.asarray(counts).tolist():
        D, n = [], 0
        for j, c in enumerate(row):
            n += c
            D.append(n / (nbar * 4.0 * math.pi / 3.0 * e[j + 1] ** 3))
        js = [j for j in range(len(D)) if D[j] < delta]
        if not js:
            Rs.append(math.nan); Ns.append(math.nan); flags.append(2)
        elif js[0] == 0:
            Rs.append(math.nan); Ns.append(math.nan); flags.append(1)
        else:
            j = js[0]
            x0, x1, y0, y1 = math.log(e[j]), math.log(e[j + 1]), math.log(D[j - 1]), math.log(D[j])
            lnR = x0 + (x1 - x0) * (y0 - math.log(delta)) / (y0 - y1)
            Rs.append(math.exp(lnR)); Ns.append(delta * nbar * 4.0 * math.pi / 3.0 * math.exp(lnR) ** 3); flags.append(0)
    return np.array(Rs), np.array(Ns), np.array(flags, np.int8), delta


def profile_edges(rmin, rmax, nbins):
    return np.concatenate([[0.0], np.geomspace(rmin, rmax, nbins)])


# ---- the shared cases ------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def uniform_case(dtype="float64"):
    """(centres: the first 300 uniform points, matter: all 1500, reference counts (300, 5)) in dtype, once per process."""
    pos = R.uniform_points().astype(dtype)
    ref = counts_of(pos[:300], pos, R.UNIFORM_L, R.UNIFORM_EDGES)
    ref.setflags(write=False)
    return pos[:300], pos, ref


ISO_N, ISO_R0, ISO_L, ISO_CENTRE = 1500, 8.0, 100.0, (99.0, 0.5, 50.0)
ISO_EDGES = profile_edges(0.5, 12.0, 24)


@functools.lru_cache(maxsize=None)
def isothermal_halo(seed=21):
    """N0 points at radii R0 (i + 1/2) / N0 about ISO_CENTRE in seeded directions: N(< r) = N0 r / R0 to within 1/2, an
    enclosed overdensity D(r) = (L^3 / (4 pi / 3)) / (R0 r^2) against nbar = N0 / L^3.  The halo wraps two faces."""
    rng = np.random.default_rng(seed)
    u = rng.standard_normal((ISO_N, 3))
    u /= np.linalg.norm(u, axis=1)[:, None]
    r = ISO_R0 * (np.arange(ISO_N) + 0.5) / ISO_N
    pos = np.asarray(ISO_CENTRE)[None, :] + r[:, None] * u
    pos.setflags(write=False)
    return pos


def isothermal_overdensity(r):
    """The analytic enclosed overdensity of isothermal_halo at radius r <= R0."""
    return ISO_L ** 3 / (4.0 * math.pi / 3.0) / (ISO_R0 * r * r)


def one_cell_case(count, seed=3):
    """(centre (1, 3), matter (count, 3), L, edges): `count` points inside cell (50, 50, 50) of the grid that the edges give
    (cells of about 0.2 at L = 100), a centre in its middle, every other cell empty."""
    L, edges = 100.0, (0.0, 0.03, 0.07, 0.12, 0.199)
    w = L / R.ncell_of(R.thresholds(edges, L))
    rng = np.random.default_rng(seed + count)
    matter = (50.0 + rng.uniform(0.05, 0.95, size=(count, 3))) * w
    return np.full((1, 3), 50.5 * w), matter, L, edges
