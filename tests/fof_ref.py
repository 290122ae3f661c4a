"""NumPy restatement of jax_nbody_emulator_with_dj_amd.halos.fof_halos: the integer
coordinates, a brute-force pair test in int64, union-find on the host and the catalogue.  The GPU tests compare with it
exactly; tests/test_fof_host.py compares it with scipy's periodic cKDTree.  It also holds the clustered test field.

Everything that decides a link is an integer, so this file and the kernels must agree bit for bit."""

import functools
import math

import numpy as np

U = 1 << 30
CENTRES = np.array([(0.0, 0.0, 0.0), (0.5, 0.0, 0.5), (0.0, 0.5, 0.25), (0.5, 0.5, 0.0), (0.3, 0.7, 0.6)])
VELOCITY_SCALES = np.array([1.0, 300.0, 1e-3])


def clustered_field(n=16, L=100.0, seed=1, dtype=np.float32):
    """(3, n, n, n) displacement: noise of 0.05 lattice steps, and around each of five centres a pull
    -0.9 d exp(-(|d|^2 / (0.2 L)^2)^4) with d the minimum-image offset from the centre: the particles within about 0.2 L
    of a centre collapse to a tenth of their distance, the rest stay on the lattice.  The first centre is the box corner,
    so its halo straddles the periodic edge on all three axes; the next three straddle it on one axis each."""
    rng = np.random.default_rng(seed)
    a = L / n
    psi = 0.05 * a * rng.standard_normal((3, n, n, n))
    q = np.stack(np.meshgrid(*([np.arange(n) * a] * 3), indexing="ij"))
    for ctr in CENTRES:
        d = q - (L * ctr)[:, None, None, None]
        d -= L * np.rint(d / L)
        r2 = (d * d).sum(axis=0)
        psi -= 0.9 * d * np.exp(-(r2 / (0.2 * L) ** 2) ** 4)
    return psi.astype(dtype)


def velocity_field(n, seed):
    """(3, n, n, n) float32 with channel scales 1, 300 and 1e-3."""
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((3, n, n, n)) * VELOCITY_SCALES[:, None, None, None]).astype(np.float32)


def threshold_field():
    """n = 4, L = 16, absolute linking length 1, so R2 = 2^52 and a coordinate unit is 2^-26: four pairs along axis 0, in
    four rows (i1, i2) that are 8 apart.  Row (0, 0): i0 = 1 stays, i0 = 2 moves by -3: d = 2^26 exactly, linked.  Row (2, 0):
    the same with i0 = 1 moved by -2^-26: d = 2^26 + 1, not linked.  Rows (0, 2) and (2, 2): the same two distances through
    the periodic face, between i0 = 0 (moved by 0 or +2^-26) and i0 = 3 moved by +3.  Every value is exact in float32.
    Returns (psi, L, ell, linked pairs, unlinked pairs) with the pairs as particle indices."""
    n, L = 4, 16.0
    psi = np.zeros((3, n, n, n), np.float32)
    eps = np.float32(2.0 ** -26)
    psi[0, 2, 0, 0] = -3.0
    psi[0, 2, 2, 0] = -3.0
    psi[0, 1, 2, 0] = -eps
    psi[0, 3, 0, 2] = 3.0
    psi[0, 3, 2, 2] = 3.0
    psi[0, 0, 2, 2] = eps
    idx = lambda i0, i1, i2: (i0 * n + i1) * n + i2
    linked = [(idx(1, 0, 0), idx(2, 0, 0)), (idx(0, 0, 2), idx(3, 0, 2))]
    unlinked = [(idx(1, 2, 0), idx(2, 2, 0)), (idx(0, 2, 2), idx(3, 2, 2))]
    return psi, L, 1.0, linked, unlinked


def chain_field(n=8, L=100.0, ell=0.25, y0=37.3, z0=51.0):
    """Particle p at (0.9 ell p mod L, y0, z0): one chain of n^3 particles, each linked to the next only (and, where the
    chain laps the box, to the particles it passes).  Returns (psi, L, ell)."""
    a = L / n
    p = np.arange(n ** 3, dtype=np.float64).reshape(n, n, n)
    q = np.stack(np.meshgrid(*([np.arange(n) * a] * 3), indexing="ij"))
    pos = np.stack([np.mod(0.9 * ell * p, L), np.full_like(p, y0), np.full_like(p, z0)])
    return (pos - q).astype(np.float32), L, ell


def coordinates(psi, L):
    """X (3, n^3) int64: rint((i_c / n + psi_c / L) 2^30) mod 2^30, formed in float64."""
    psi = np.asarray(psi)
    n = psi.shape[1]
    q = np.stack(np.meshgrid(*([np.arange(n, dtype=np.float64) / n] * 3), indexing="ij"))
    t = q + psi.astype(np.float64) / float(L)
    if not np.isfinite(t).all() or (np.abs(psi.astype(np.float64) / float(L)) >= 2.0 ** 20).any():
        raise ValueError("non-finite or out-of-range coordinate")
    return (np.rint(t * float(U)).astype(np.int64) & (U - 1)).reshape(3, -1)


def r2_of(ell, L):
    return int(math.floor((ell / L) ** 2 * 2.0 ** 60))


def ncell_of(R2):
    return min(4096, U // (math.isqrt(R2) + 1))


def min_image(d):
    """(X - Y) mod U mapped to [-U/2, U/2)."""
    return ((d + U // 2) & (U - 1)) - U // 2


def linked_pairs(X, R2, chunk=512):
    """(p, q) with p < q of every linked pair: d0^2 + d1^2 + d2^2 <= R2 in int64, brute force over all pairs (the first
    axis is tested on its own first so that only its survivors cost the other two)."""
    N = X.shape[1]
    s = math.isqrt(R2)
    out = []
    for lo in range(0, N, chunk):
        hi = min(N, lo + chunk)
        d0 = min_image(X[0, lo:hi, None] - X[0, None, :])
        ii, jj = np.nonzero(np.abs(d0) <= s)
        keep = (ii + lo) < jj
        ii, jj = ii[keep], jj[keep]
        d = min_image(X[:, ii + lo] - X[:, jj])
        ok = (d * d).sum(axis=0) <= R2
        out.append(np.stack([ii[ok] + lo, jj[ok]]))
    return np.concatenate(out, axis=1)


def components(N, pairs):
    """root (N,) int64: the smallest particle index of each connected component (union-find, smaller root wins)."""
    parent = list(range(N))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    for p, q in zip(pairs[0].tolist(), pairs[1].tolist()):
        a, b = find(p), find(q)
        if a != b:
            parent[max(a, b)] = min(a, b)
    return np.array([find(x) for x in range(N)], dtype=np.int64)


def velocity_exponents(v):
    """e_c with max |v_c| < 2^e_c (frexp), as nbe_quantity_range / nbe_paint_fields."""
    amax = np.abs(np.asarray(v, np.float32).reshape(3, -1)).max(axis=1).astype(np.float64)
    return np.frexp(amax)[1].astype(np.int64)


def fof(psi, L, linking_length=0.2, nmin=20, absolute=False, velocity=None):
    """The dict of fof_halos (with labels), all NumPy."""
    psi = np.asarray(psi)
    n = psi.shape[1]
    N = n ** 3
    ell = float(linking_length) if absolute else float(linking_length) * float(L) / n
    R2 = r2_of(ell, L)
    X = coordinates(psi, L)
    root = components(N, linked_pairs(X, R2))
    size = np.bincount(root, minlength=N).astype(np.int64)
    label = np.nonzero(size >= nmin)[0]
    length = size[label]
    order = np.lexsort((label, -length))
    label, length = label[order], length[order]
    row = np.full(N, -1, np.int64)
    row[label] = np.arange(len(label))
    labels = row[root]
    member = labels >= 0
    d = min_image(X[:, member] - X[:, root[member]])
    S = np.zeros((len(label), 3), np.int64)
    for c in range(3):
        np.add.at(S[:, c], labels[member], d[c])
    cm = np.mod(X[:, label].T + S.astype(np.float64) / length[:, None].astype(np.float64), float(U)) / float(U) * float(L)
    out = {"CMPosition": cm, "Length": length, "label": label, "ngroups": int((size > 0).sum()),
           "linking_length": ell, "labels": labels.reshape(n, n, n).astype(np.int32), "R2": R2, "X": X, "root": root}
    if velocity is not None:
        v = np.asarray(velocity).astype(np.float32).reshape(3, -1)
        e = velocity_exponents(v)
        V = np.rint(np.ldexp(v.astype(np.float64), (24 - e)[:, None].astype(np.int32))).astype(np.int64)
        SV = np.zeros((len(label), 3), np.int64)
        for c in range(3):
            np.add.at(SV[:, c], labels[member], V[c, member])
        out["CMVelocity"] = np.ldexp(SV.astype(np.float64), (e - 24)[None, :].astype(np.int32)) \
            / length[:, None].astype(np.float64)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """The shared cases of the tests, computed once per process: (psi, L, velocity, kwargs, reference dict)."""
    if name == "clustered16":
        psi, L, v = clustered_field(16, 100.0, 1), 100.0, velocity_field(16, 11)
    elif name == "clustered16_half":
        psi, L, v = clustered_field(16, 100.0, 1).astype(np.float16), 100.0, velocity_field(16, 11)
    elif name == "clustered24":
        psi, L, v = clustered_field(24, 100.0, 2), 100.0, velocity_field(24, 12)
    else:
        raise KeyError(name)
    kw = dict(linking_length=0.2, nmin=8)
    return psi, L, v, kw, fof(psi, L, velocity=v, **kw)
