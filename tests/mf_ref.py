"""NumPy restatement of the Minkowski-functional counts of density.minkowski_functionals, threshold by threshold, straight
from the definition (include/nbe.h, "Minkowski functionals").  One boolean mask and a handful of periodic shifts per
threshold: meant for meshes up to 128^3."""

import itertools

import numpy as np

E = ((1, 0, 0), (0, 1, 0), (0, 0, 1))


def _any_shifted(m, shifts):
    """#{v : m[v - s] for some s in shifts} (indices mod n)."""
    out = np.zeros_like(m)
    for s in shifts:
        out |= np.roll(m, s, axis=(0, 1, 2))
    return int(np.count_nonzero(out))


def element_counts(mask):
    """(n0, n1, n2, n3) of the periodic cubical complex of a cubic boolean mask."""
    m = np.asarray(mask, dtype=bool)
    assert m.ndim == 3 and len(set(m.shape)) == 1
    zero = (0, 0, 0)
    add = lambda a, b: tuple(x + y for x, y in zip(a, b))
    n3 = int(np.count_nonzero(m))
    n2 = sum(_any_shifted(m, [zero, E[a]]) for a in range(3))
    n1 = 0
    for a in range(3):
        b, c = [E[x] for x in range(3) if x != a]
        n1 += _any_shifted(m, [zero, b, c, add(b, c)])
    n0 = _any_shifted(m, list(itertools.product((0, 1), repeat=3)))
    return n0, n1, n2, n3


def standardized(x, mean, std):
    """float32 w = (x - float32(mean)) / float32(std), 0 where float32(std) is 0; numpy rounds each operation."""
    x = np.asarray(x, dtype=np.float32)
    mf, sf = np.float32(mean), np.float32(std)
    if sf == 0:
        return np.zeros_like(x)
    return (x - mf) / sf


def counts(field, thresholds, standardize=True, mean=None, std=None):
    """(T, 4) int64 counts (n0, n1, n2, n3) of {w >= t} for every threshold, in the given order.  With standardize, mean
    and std are those to standardize with (the device's, as returned); by default float64 NumPy's."""
    x = np.asarray(field, dtype=np.float32)
    if standardize:
        if mean is None:
            mean, std = float(x.astype(np.float64).mean()), float(x.astype(np.float64).std())
        w = standardized(x, mean, std)
    else:
        w = x
    t = np.asarray(thresholds, dtype=np.float32).ravel()
    return np.array([element_counts(w >= v) for v in t], dtype=np.int64).reshape(-1, 4)


def functionals(c, n, boxsize):
    """(v0, v1, v2, v3) from (T, 4) counts of an n^3 mesh in a box of side boxsize."""
    c = np.asarray(c, dtype=np.float64)
    n0, n1, n2, n3 = c.T
    h, vol = boxsize / n, float(boxsize) ** 3
    return (h ** 3 * n3 / vol, h ** 2 * (-2.0 / 3.0 * n3 + 2.0 / 9.0 * n2) / vol,
            h * (2.0 / 3.0 * n3 - 4.0 / 9.0 * n2 + 2.0 / 9.0 * n1) / vol, (n0 - n1 + n2 - n3) / vol)


def block_counts(a, b, c):
    """Closed form of an a x b x c block of voxels that does not wrap onto itself."""
    return ((a + 1) * (b + 1) * (c + 1),
            a * (b + 1) * (c + 1) + (a + 1) * b * (c + 1) + (a + 1) * (b + 1) * c,
            (a + 1) * b * c + a * (b + 1) * c + a * b * (c + 1),
            a * b * c)


def slab_counts(s, n):
    """Closed form of s whole planes (0 < s < n) of an n^3 periodic mesh."""
    return ((s + 1) * n * n, (3 * s + 2) * n * n, (3 * s + 1) * n * n, s * n * n)
