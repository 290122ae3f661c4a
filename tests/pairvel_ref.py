"""NumPy / Python-int restatement of the pairwise velocity moments: correlation.pairwise_velocity
and profiles.radial_velocity_moments.  Coordinates, thresholds and bins are those of tests/pairs_ref.py, tests/profiles_ref.py
and tests/fof_ref.py; what is new here is the velocity word, the radial word of a pair with its exact rounding in Python
ints, the five sums per bin by brute force over all pairs, and the float64 quantities derived from them.

Every sum is a sum of integers fixed by the pair alone, so this file and the kernels must agree bit for bit."""

import math

import numpy as np

import fof_ref as F
import pairs_ref as R

BITS, SPLIT = 20, 24
MASK = (1 << SPLIT) - 1
MAX_PAIRS = 1 << 39


def exponent(*velocities):
    """The one exponent of a call: the e of frexp with max |v_c| < 2^e over every component of every array (None is
    skipped); 0 for all-zero velocities.  ValueError for a non-finite value."""
    top = 0.0
    for v in velocities:
        if v is None:
            continue
        v = np.asarray(v).astype(np.float64)
        if not np.isfinite(v).all():
            raise ValueError("non-finite velocity")
        top = max(top, float(np.abs(v).max()))
    return int(math.frexp(top)[1])


def words(v, e):
    """W (3, count) int64 = rint(v 2^(20 - e)) of a (count, 3) table or a (3, n, n, n) field, formed in float64."""
    v = np.asarray(v)
    v = v.reshape(3, -1) if v.ndim == 4 else v.T
    return np.rint(np.ldexp(v.astype(np.float64), BITS - e)).astype(np.int64)


def vr_exact(u, q):
    """sign(u) k with k = floor(|u| / sqrt(q) + 1/2) in Python ints: the k >= 0 with (2 k - 1)^2 q <= 4 u^2 < (2 k + 1)^2 q;
    0 for q = 0.  2 |u| / sqrt(q) = sqrt(4 u^2 / q), and floor((x + 1) / 2) of x = floor(sqrt(4 u^2 / q)) is that k: the
    candidates around it are tested as the definition reads."""
    u, q = int(u), int(q)
    if q == 0 or u == 0:
        return 0
    k = (math.isqrt(4 * u * u // q) + 1) // 2
    while k > 0 and (2 * k - 1) ** 2 * q > 4 * u * u:
        k -= 1
    while (2 * k + 1) ** 2 * q <= 4 * u * u:
        k += 1
    return k if u > 0 else -k


def is_tie(u, q):
    """4 u^2 = (2 k + 1)^2 q for some k >= 0: the radial word would sit on a rounding boundary."""
    u, q = int(u), int(q)
    if q == 0:
        return False
    m, r = divmod(4 * u * u, q)
    s = math.isqrt(m)
    return r == 0 and s * s == m and s % 2 == 1


def terms(d, dW, verify=True):
    """(vr, vr^2, |dW|^2) int64 of pairs with the differences d, dW (3, pairs) int64 (both taken o - a).  The radial word is
    formed as rint(u / sqrt(q)) in float64 and, with verify, held to vr_exact pair by pair."""
    q = (d * d).sum(axis=0)
    u = (dW * d).sum(axis=0)
    with np.errstate(divide="ignore", invalid="ignore"):
        vr = np.where(q > 0, np.rint(u.astype(np.float64) / np.sqrt(q.astype(np.float64))), 0.0).astype(np.int64)
    if verify:
        for uu, qq, vv in zip(u.tolist(), q.tolist(), vr.tolist()):
            assert vr_exact(uu, qq) == vv, (uu, qq, vv)
    return vr, vr * vr, (dW * dW).sum(axis=0)


def accumulate(out, b, vr, vr2, dw2):
    """out (nb, 6) += (1, vr, vr^2 lo, vr^2 hi, |dW|^2 lo, |dW|^2 hi) of the pairs in the bins b."""
    for col, val in enumerate((np.ones_like(vr), vr, vr2 & MASK, vr2 >> SPLIT, dw2 & MASK, dw2 >> SPLIT)):
        np.add.at(out[:, col], b, val)


def pair_velocity(XA, WA, T, XB=None, WB=None, chunk=256, verify=True):
    """int64 (nb, 6): N and the five sums per bin, brute force over all pairs of XA (each unordered pair once) or over all
    (i in XA, j in XB).  X, W are (3, count) int64."""
    nb = len(T) - 1
    Tarr = np.array(T, dtype=np.int64)
    out = np.zeros((nb, 6), np.int64)
    Y, WY = (XA, WA) if XB is None else (XB, WB)
    for lo in range(0, XA.shape[1], chunk):
        hi = min(XA.shape[1], lo + chunk)
        d = F.min_image(Y[:, None, :] - XA[:, lo:hi, None])                   # o - a
        d2 = (d * d).sum(axis=0)
        keep = (d2 > Tarr[0]) & (d2 <= Tarr[-1])
        if XB is None:
            keep &= (np.arange(lo, hi)[:, None] < np.arange(Y.shape[1])[None, :])
        ii, jj = np.nonzero(keep)
        b = np.searchsorted(Tarr, d2[ii, jj], side="left") - 1                  # T[b] < q <= T[b + 1]
        accumulate(out, b, *terms(d[:, ii, jj], WY[:, jj] - WA[:, lo + ii], verify))
    return out


def radial_velocity(XA, WA, XB, WB, T, verify=True):
    """int64 (H, nb, 6): pair_velocity of every centre on its own against the matter; WA None: centres at rest."""
    if WA is None:
        WA = np.zeros_like(XA)
    return np.stack([pair_velocity(XA[:, h:h + 1], WA[:, h:h + 1], T, XB, WB, verify=verify) for h in range(XA.shape[1])])


def moments_of(a, va, L, edges, b=None, vb=None, verify=True):
    """(sums (nb, 6), e) of two catalogues of either kind with their velocities."""
    e = exponent(va, vb)
    XB = None if b is None else R.catalogue(b, L)
    WB = None if b is None else words(vb, e)
    return pair_velocity(R.catalogue(a, L), words(va, e), R.thresholds(edges, L), XB, WB, verify=verify), e


def profiles_of(centres, vc, matter, vm, L, edges, verify=True):
    """(sums (H, nb, 6), e) of centres (velocities vc or None) against matter."""
    e = exponent(vc, vm)
    WA = None if vc is None else words(vc, e)
    return radial_velocity(R.catalogue(centres, L), WA, R.catalogue(matter, L), words(vm, e), R.thresholds(edges, L), verify), e


def derived(sums, e):
    """dict v12, vr2, sigma_r, vt2, sigma_t in float64 from the table (..., 6) and the exponent, as the module states them;
    NaN where N = 0."""
    s = np.asarray(sums)
    n = s[..., 0].astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        v12 = math.ldexp(1.0, e - BITS) * s[..., 1].astype(np.float64) / n
        vr2 = math.ldexp(1.0, 2 * (e - BITS)) * (2.0 ** SPLIT * s[..., 3].astype(np.float64) + s[..., 2].astype(np.float64)) / n
        dv2 = math.ldexp(1.0, 2 * (e - BITS)) * (2.0 ** SPLIT * s[..., 5].astype(np.float64) + s[..., 4].astype(np.float64)) / n
        vt2 = 0.5 * (dv2 - vr2)
        return {"v12": v12, "vr2": vr2, "sigma_r": np.sqrt(np.maximum(vr2 - v12 * v12, 0.0)), "vt2": vt2,
                "sigma_t": np.sqrt(np.maximum(vt2, 0.0))}


def gaussian_velocity(shape, seed, scale=250.0, dtype=np.float64):
    """Seeded Gaussian velocities of a shape, km/s-like."""
    return (scale * np.random.default_rng(seed).standard_normal(shape)).astype(dtype)


# ---- the shared cases ------------------------------------------------------------------------------------------------------

def clustered_centres():
    """The five centres of F.clustered_field, the eight box corners and six face centres of the L = 100 box."""
    corners = np.array([[x, y, z] for x in (0.0, 100.0) for y in (0.0, 100.0) for z in (0.0, 100.0)])
    faces = np.array([[50.0, 50.0, 0.0], [50.0, 0.0, 50.0], [0.0, 50.0, 50.0], [50.0, 50.0, 100.0], [100.0, 50.0, 50.0],
                      [50.0, 100.0, 50.0]])
    return np.concatenate([F.CENTRES * 100.0, corners, faces])


def cases():
    """(name, a, va, b, vb, L, edges) of every case that the host walk and the GPU tests run: a with its velocity va (None:
    centres at rest) alone (b None: the auto moments) or against b with vb (the cross moments and, a being positions, the
    per-centre tables).  The smallest at which a kernel can go wrong, as tools/catalog_host_walk.py lists them for the counts."""
    import profiles_ref as PR
    pos = R.uniform_points()
    vel = gaussian_velocity((1500, 3), 41)
    for dt in ("float64", "float32"):
        p, v = pos.astype(dt), vel.astype(dt)
        yield "uniform auto %s" % dt, p, v, None, None, R.UNIFORM_L, R.UNIFORM_EDGES
        yield "uniform cross %s" % dt, p[:300], v[:300], p, v, R.UNIFORM_L, R.UNIFORM_EDGES
    yield "uniform r_0 = 2", pos[:300], vel[:300], pos, vel, R.UNIFORM_L, R.UNIFORM_EDGES[1:]
    centres, vc = clustered_centres(), gaussian_velocity((19, 3), 42)
    for dt in (np.float32, np.float16):
        yield ("clustered displacement %s" % np.dtype(dt).name, centres, vc, F.clustered_field(16).astype(dt),
               F.velocity_field(16, 11).astype(dt), 100.0, PR.profile_edges(0.5, 20.0, 12))
    rng = np.random.default_rng(8)
    yield ("ncell 3", rng.uniform(0.0, 100.0, size=(40, 3)), gaussian_velocity((40, 3), 43), rng.uniform(0.0, 100.0, size=(200, 3)),
           gaussian_velocity((200, 3), 44), 100.0, (0.0, 10.0, 33.0))
    ten = rng.uniform(0.0, 100.0, size=(10, 3))
    yield "ncell 4096", ten, vel[:10], ten, vel[:10], 100.0, (0.0, 0.01, 0.02)
    for count in (255, 256, 257, 1000):
        c, m, L, e = PR.one_cell_case(count)
        yield "one cell of %d" % count, c, vel[:1], m, vel[:count], L, e
    yield "one cell of 1000, auto", PR.one_cell_case(1000)[1], vel[:1000], None, None, 100.0, PR.one_cell_case(1000)[3]
    edge = R.edge_points()
    yield "edges hit exactly", edge, vel[:len(edge)], edge, vel[:len(edge)], R.EDGE_L, R.EDGE_EDGES
    yield "edges hit exactly, auto", edge, vel[:len(edge)], None, None, R.EDGE_L, R.EDGE_EDGES
    yield "1 bin", pos[:50], vel[:50], pos, vel, R.UNIFORM_L, (0.0, 25.0)
    yield "128 bins", pos[:50], vel[:50], pos, vel, R.UNIFORM_L, np.linspace(0.0, 30.0, 129)
    yield "H = 1, count_b = 1", pos[:1], vel[:1], pos[:1], vel[1:2], R.UNIFORM_L, R.UNIFORM_EDGES
    twice = np.concatenate([pos[:40], pos[:40]])
    yield "coincident rows, r_0 = 0", twice, vel[:80], twice, vel[80:160], R.UNIFORM_L, R.UNIFORM_EDGES
    yield "coincident rows, r_0 = 2", twice, vel[:80], None, None, R.UNIFORM_L, R.UNIFORM_EDGES[1:]
    yield "zero velocities", pos[:200], np.zeros((200, 3)), pos, np.zeros((1500, 3)), R.UNIFORM_L, R.UNIFORM_EDGES
    axis, sign = rng.integers(0, 3, 1500), rng.choice((-1.0, 1.0), 1500)
    for dt in (np.float64, np.float32):                     # the largest value below 256 = 2^e of the dtype: words of +-2^20
        top = np.zeros((1500, 3), dt)
        top[np.arange(1500), axis] = sign.astype(dt) * np.nextafter(dt(256.0), dt(0.0))
        yield "one component at +-max %s" % np.dtype(dt).name, pos[:300].astype(dt), top[:300], pos.astype(dt), top, \
            R.UNIFORM_L, R.UNIFORM_EDGES
    yield "centres at rest", pos[:300], None, pos, vel, R.UNIFORM_L, R.UNIFORM_EDGES


def case(name):
    for c in cases():
        if c[0] == name:
            return c[1:]
    raise KeyError(name)


CASE_NAMES = tuple(c[0] for c in cases())
