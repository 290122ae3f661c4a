"""NumPy restatement of jax_nbody_emulator_with_dj_amd.correlation: the integer coordinates, the
thresholds, a brute-force pair count in int64 over all pairs with Python ints for the mu comparison, the analytic RR and the
Legendre bin integrals.  The GPU tests compare the counts with it exactly; tests/test_pairs_host.py compares it with scipy's
periodic cKDTree.

Everything that decides a bin is an integer, so this file and the kernels must agree bit for bit."""

import functools
import math

import numpy as np

import fof_ref as F

U = F.U


def coordinates(pos, L):
    """X (3, count) int64 of (count, 3) positions: rint((x / L) 2^30) mod 2^30, formed in float64."""
    r = np.asarray(pos).astype(np.float64) / float(L)
    if not np.isfinite(r).all() or (np.abs(r) >= 2.0 ** 20).any():
        raise ValueError("non-finite or out-of-range coordinate")
    return (np.rint(r * float(U)).astype(np.int64) & (U - 1)).T.copy()


def catalogue(x, L):
    """X (3, count) int64 of either kind of catalogue."""
    x = np.asarray(x)
    return F.coordinates(x, L) if x.ndim == 4 else coordinates(x, L)


def thresholds(r_edges, L):
    T = [int(math.floor((float(r) / float(L)) ** 2 * 2.0 ** 60)) for r in r_edges]
    if float(r_edges[0]) == 0.0:
        T[0] = -1
    return T


def ncell_of(T):
    return min(4096, U // (math.isqrt(T[-1]) + 1))


def mu_bin(dl2, d2, nmu):
    """#{ j in 1 .. nmu - 1 : dl2 nmu^2 >= j^2 d2 } in Python ints; 0 for d2 = 0.  j^2 d2 <= P iff j^2 <= P // d2 iff
    j <= isqrt(P // d2), so the count is min(nmu - 1, isqrt(dl2 nmu^2 // d2)) (mu_bin_counted spells the set out)."""
    if d2 == 0:
        return 0
    return min(nmu - 1, math.isqrt(dl2 * nmu * nmu // d2))


def mu_bin_counted(dl2, d2, nmu):
    return 0 if d2 == 0 else sum(1 for j in range(1, nmu) if dl2 * nmu * nmu >= j * j * d2)


def pair_counts(XA, T, XB=None, nmu=None, los=2, chunk=256):
    """int64 (nb,) or (nb, nmu): brute force over all pairs of XA (each unordered pair once), or over all (i in XA, j in
    XB)."""
    nb = len(T) - 1
    Tarr = np.array(T, dtype=np.int64)
    out = np.zeros((nb, nmu or 1), np.int64)
    Y = XA if XB is None else XB
    for lo in range(0, XA.shape[1], chunk):
        hi = min(XA.shape[1], lo + chunk)
        d = F.min_image(XA[:, lo:hi, None] - Y[:, None, :])
        d2 = (d * d).sum(axis=0)
        keep = (d2 > Tarr[0]) & (d2 <= Tarr[-1])
        if XB is None:
            keep &= (np.arange(lo, hi)[:, None] < np.arange(Y.shape[1])[None, :])
        ii, jj = np.nonzero(keep)
        q = d2[ii, jj]
        b = np.searchsorted(Tarr, q, side="left") - 1                       # T[b] < q <= T[b + 1]
        if nmu is None:
            np.add.at(out[:, 0], b, 1)
        else:
            dl = d[los, ii, jj]
            for bb, qq, ll in zip(b.tolist(), q.tolist(), dl.tolist()):
                out[bb, mu_bin(ll * ll, qq, nmu)] += 1
    return out[:, 0] if nmu is None else out


def rr(r_edges, L, count_a, count_b=None, nmu=None):
    e = [float(r) for r in r_edges]
    norm = count_a * (count_a - 1) / 2.0 if count_b is None else float(count_a) * float(count_b)
    out = np.array([norm * (4.0 * math.pi / 3.0 * (e[b + 1] ** 3 - e[b] ** 3)) / float(L) ** 3 for b in range(len(e) - 1)])
    return out if nmu is None else np.repeat(out[:, None] / nmu, nmu, axis=1)


def legendre_integrals(nmu):
    """(3, nmu): the integrals of L_0, L_2 = (3 mu^2 - 1) / 2 and L_4 = (35 mu^4 - 30 mu^2 + 3) / 8 over the mu bins."""
    anti = (lambda m: m, lambda m: (m ** 3 - m) / 2.0, lambda m: (7.0 * m ** 5 - 10.0 * m ** 3 + 3.0 * m) / 8.0)
    return np.array([[f((m + 1) / nmu) - f(m / nmu) for m in range(nmu)] for f in anti])


def estimator(npairs, r_edges, L, count_a, count_b=None, nmu=None):
    """dict rr, xi, r_mid and, with nmu, xi0, xi2, xi4."""
    R = rr(r_edges, L, count_a, count_b, nmu)
    xi = np.asarray(npairs, dtype=np.float64) / R - 1.0
    e = np.asarray(r_edges, dtype=np.float64)
    out = {"rr": R, "xi": xi, "r_mid": 0.5 * (e[1:] + e[:-1])}
    if nmu is not None:
        w = legendre_integrals(nmu)
        for i, ell in enumerate((0, 2, 4)):
            out["xi%d" % ell] = (2 * ell + 1) * (xi * w[i][None, :]).sum(axis=1)
    return out


# ---- the shared cases ------------------------------------------------------------------------------------------------------

LATTICE_N, LATTICE_L = 16, 128.0
LATTICE_EDGES = tuple(f * LATTICE_L / LATTICE_N for f in (0.5, 1.2, 1.6, 1.9))      # shells at a, sqrt(2) a, sqrt(3) a
UNIFORM_L, UNIFORM_EDGES = 100.0, (0.0, 2.0, 5.0, 11.0, 20.0, 31.0)


def lattice_positions(n=LATTICE_N, L=LATTICE_L):
    q = np.stack(np.meshgrid(*([np.arange(n) * (L / n)] * 3), indexing="ij"))
    return np.ascontiguousarray(q.reshape(3, -1).T)


@functools.lru_cache(maxsize=None)
def uniform_points(count=1500, L=UNIFORM_L, seed=5):
    """count points uniform in [-3 L, 4 L): several boxes away on both sides."""
    pos = np.random.default_rng(seed).uniform(-3.0 * L, 4.0 * L, size=(count, 3))
    pos.setflags(write=False)
    return pos


@functools.lru_cache(maxsize=None)
def uniform_case(dtype="float64", nmu=None, los=2):
    """(positions in dtype, X, T, counts of the auto count of the 1500 uniform points), computed once per process."""
    pos = uniform_points().astype(dtype)
    X = coordinates(pos, UNIFORM_L)
    T = thresholds(UNIFORM_EDGES, UNIFORM_L)
    ref = pair_counts(X, T, nmu=nmu, los=los)
    ref.setflags(write=False)
    return pos, X, T, ref


EDGE_L, EDGE_EDGES = 64.0, (0.0, 3.0, 5.0, 9.0, 13.0)


@functools.lru_cache(maxsize=None)
def edge_points(seed=8):
    """Points on multiples of L 2^-10 (one step is 1/16 of a length unit, 2^20 coordinate units): 60 random ones, and
    beside each of them partners at exactly 3, 5, 9 and 13 length units -- (48, 0, 0), (48, 64, 0), (0, 0, 144) and
    (80, 0, 192) steps with random signs and axes --, so that d^2 equals a threshold for at least 240 pairs."""
    rng = np.random.default_rng(seed)
    base = rng.integers(0, 1 << 10, size=(60, 3))
    pts = [base]
    for off in ((48, 0, 0), (48, 64, 0), (0, 0, 144), (80, 0, 192)):
        o = np.array([rng.permutation(off) * rng.choice((-1, 1), 3) for _ in range(len(base))])
        pts.append(base + o)
    pos = np.concatenate(pts).astype(np.float64) * (EDGE_L / 1024.0)
    pos.setflags(write=False)
    return pos
