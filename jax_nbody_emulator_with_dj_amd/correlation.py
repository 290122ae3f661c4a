"""Pair counts of periodic catalogues on the GPU: xi(r), xi(s, mu) and its multipoles (Corrfunc's theory.DD / theory.DDsmu,
nbodykit's SimulationBox2PCF).

    from jax_nbody_emulator_with_dj_amd.correlation import pair_counts, correlation_function

    dd = pair_counts(positions, 1000.0, np.linspace(0.0, 50.0, 26))                 # npairs (25,) int64
    xi = correlation_function(halo_positions, 1000.0, edges, b=displacement)        # xi_hm against the displaced lattice
    xs = correlation_function(positions, 1000.0, edges, nmu=10, los=2)              # xi (nb, 10), xi0, xi2, xi4

Definition (tests/pairs_ref.py restates it in NumPy).  The box is cubic and periodic with side L and
U = 2^30 coordinate units.  A catalogue is a (count, 3) float32 / float64 array of positions, any number of boxes away, with
X_c = rint((x_c / L) U) mod U formed in float64, or a displaced lattice (3, n, n, n) float32 / float16 with the coordinates
of halos.fof_halos, bit for bit.  The minimum-image difference d_c is (X_c(p) - X_c(q)) mod U mapped to [-U/2, U/2) and
d^2 = d_0^2 + d_1^2 + d_2^2 in 64-bit integers.  The nb + 1 edges r_b become the thresholds T_b = floor((r_b / L)^2 2^60),
with T_0 = -1 for r_0 = 0, and a pair is in bin b iff T_b < d^2 <= T_{b+1}: (r_b, r_{b+1}] on the rounded coordinates, "<= T"
being the FoF link rule, so that the auto count for the edges [0, l] is the number of FoF links at linking length l.  With
nmu, mu = |d_los| / |d| is binned uniformly over [0, 1]: for d^2 > 0, m = #{ j in 1 .. nmu - 1 : d_los^2 nmu^2 >= j^2 d^2 },
compared exactly, and m = 0 for d^2 = 0.  An auto count (b=None) takes each unordered pair of distinct rows once; a cross
count takes every (i in a, j in b), coincident rows included.  Counts are sums of ones: the same bits for every launch
geometry, order of the rows and stream.

xi = DD / RR - 1 on the host in float64 with the analytic RR = N (N - 1) / 2 V_b / L^3 dmu (auto) or N_a N_b V_b / L^3 dmu
(cross), V_b = 4 pi / 3 (r_{b+1}^3 - r_b^3), dmu = 1 / nmu (1 without mu bins), and xi_l(s_b) = (2 l + 1) sum_m xi(s_b, mu_m)
int_{m / nmu}^{(m + 1) / nmu} L_l(mu) dmu for l = 0, 2, 4 with the exact polynomial integrals.

Not built: weights, non-uniform mu bins, r_max >= L / 3, and the mesh-based xi(r) (an inverse FFT of |delta_k|^2).

Residency as in density.py: NumPy in gives NumPy out, CUDA tensors in give CUDA tensors on their device, on torch's current
stream.  There is no CPU fallback.  Arguments are validated before any device work.
"""

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib
from .density import (_check_array, _check_free_memory, _check_los, _check_max_blocks, _device_of, _dtype_name, _is_torch,
                      _ptr, _same_kind, _stream, _triple)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["pair_counts", "correlation_function", "pair_geometry", "analytic_rr", "legendre_bin_integrals", "multipoles"]

_U = 1 << 30                    # include/nbe.h, "Halos": coordinate units per box side
_MIN_N, _MAX_N = 2, 1024        # NBE_FOF_MIN_N, NBE_FOF_MAX_N
_MAX_CELLS = 4096               # NBE_FOF_MAX_CELLS
MAX_BINS, MAX_MU, MAX_IMAGE = 128, 32, 4096     # NBE_PAIR_MAX_BINS, NBE_PAIR_MAX_MU, NBE_PAIR_MAX_IMAGE
MAX_COUNT = 1 << 30
# Peak device memory per row of a catalogue beside a tensor input: coordinates 12, keys 8, torch.sort's sorted keys, order
# and scratch 8 + 8 + 16, FoF's parent 4 (lattice input), the sorted records 16; a NumPy input adds
# its device copy, at most 24
BYTES_PER_PARTICLE = 96


def pair_geometry(boxsize, r_edges):
    """(edges float64 (nb + 1,), thresholds as a list of Python ints, ncell) of a call: T_b = floor((r_b / L)^2 2^60), -1 for
    r_0 = 0, and ncell = min(4096, U // (isqrt(T_nb) + 1)).  ValueError for edges that are not 2 .. 129 finite, strictly
    increasing lengths from 0 or more, that reach L / 3, or whose thresholds do not increase strictly."""
    L = float(boxsize)
    e = np.asarray(r_edges)
    if e.ndim != 1 or e.dtype.kind not in "fiu" or not 2 <= e.size <= MAX_BINS + 1:
        raise ValueError("pair_counts: r_edges must be 2 .. %d real numbers (1 .. %d bins), got %s"
                         % (MAX_BINS + 1, MAX_BINS, "shape %s" % (e.shape,) if e.dtype.kind in "fiu" else e.dtype))
    e = e.astype(np.float64)
    if not np.isfinite(e).all() or e[0] < 0.0 or not (np.diff(e) > 0.0).all():
        raise ValueError("pair_counts: r_edges must be finite and strictly increasing from 0 or more, got %s" % (e,))
    if not e[-1] < L / 3.0:
        raise ValueError("pair_counts: the largest edge %g must stay below L / 3 = %g (at least 3 cells per axis)"
                         % (e[-1], L / 3.0))
    T = [int(math.floor((float(r) / L) ** 2 * 2.0 ** 60)) for r in e]
    if e[0] == 0.0:
        T[0] = -1
    if any(b <= a for a, b in zip(T, T[1:])):
        raise ValueError("pair_counts: two edges of %s give the same threshold floor((r / L)^2 2^60)" % (e,))
    ncell = min(_MAX_CELLS, _U // (math.isqrt(T[-1]) + 1))
    if ncell < 3:
        raise ValueError("pair_counts: the largest edge %g must stay below L / 3 = %g (at least 3 cells per axis)"
                         % (e[-1], L / 3.0))
    return e, T, ncell


def _catalogue(x, name):
    """(array, kind, rows) of one catalogue, validated: kind 'positions' for (count, 3), 'lattice' for (3, n, n, n)."""
    x = _check_array(x, name)
    dt = _dtype_name(x)
    if x.ndim == 2 and x.shape[1] == 3:
        if dt not in ("float32", "float64"):
            raise ValueError("pair_counts: positions %s must be float32 or float64, got %s" % (name, dt))
        if not 1 <= x.shape[0] <= MAX_COUNT:
            raise ValueError("pair_counts: %s must have 1 .. 2^30 rows, got %d" % (name, x.shape[0]))
        return x, "positions", int(x.shape[0])
    if x.ndim == 4 and x.shape[0] == 3 and len(set(x.shape[1:])) == 1:
        if dt not in ("float32", "float16"):
            raise ValueError("pair_counts: displacement %s must be float32 or float16, got %s" % (name, dt))
        n = int(x.shape[1])
        if not _MIN_N <= n <= _MAX_N:
            raise ValueError("pair_counts: lattice size %d unsupported (%d .. %d)" % (n, _MIN_N, _MAX_N))
        return x, "lattice", n ** 3
    raise ValueError("pair_counts: %s must be (count, 3) positions or a (3, n, n, n) displacement, got shape %s"
                     % (name, tuple(x.shape)))


def _validate(a, boxsize, r_edges, b, nmu, los, max_blocks):
    A = _catalogue(a, "a")
    B = None if b is None else _catalogue(b, "b")
    if B is not None:
        _same_kind(A[0], B[0], "pair_counts: a", "b")
    L = _triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("pair_counts needs a cubic box, got boxsize %s" % (L,))
    edges, T, ncell = pair_geometry(L[0], r_edges)
    if nmu is not None:
        if isinstance(nmu, (bool, np.bool_)) or not isinstance(nmu, numbers.Integral) or not 1 <= int(nmu) <= MAX_MU:
            raise ValueError("pair_counts: nmu must be None or an int in 1 .. %d, got %r" % (MAX_MU, nmu))
        nmu = int(nmu)
        if (len(T) - 1) * nmu > MAX_IMAGE:
            raise ValueError("pair_counts: %d x %d bins exceed %d" % (len(T) - 1, nmu, MAX_IMAGE))
    los = _check_los(los)
    return A, B, L[0], edges, T, ncell, nmu, los, _check_max_blocks(max_blocks, "pair_counts")


def _on_device(x, dev):
    if _is_torch(x):
        return x.contiguous()
    x = np.ascontiguousarray(x)
    return torch.from_numpy(x if x.flags.writeable else x.copy()).to(dev)


def _sorted_records(l, x, kind, rows, L, ncell, blocks, dev, s, tick):
    """(records (rows, 4) int32 in cell order, sorted keys int64) of one catalogue on the device."""
    tick("coords")
    X = torch.empty((3, rows), dtype=torch.int32, device=dev)
    keys = torch.empty(rows, dtype=torch.int64, device=dev)
    stats = torch.zeros(1, dtype=torch.int32, device=dev)
    xd = _on_device(x, dev)
    if kind == "lattice":
        scratch = torch.empty(rows, dtype=torch.int32, device=dev)                  # FoF's parent: not used here
        _lib.check(l.nbe_fof_cells(_ptr(xd), 1 if xd.dtype == torch.float16 else 0, int(x.shape[1]), L, ncell, blocks,
                                   _ptr(X), _ptr(keys), _ptr(scratch), _ptr(stats), s))
        del scratch
    else:
        _lib.check(l.nbe_pair_coords(_ptr(xd), 2 if xd.dtype == torch.float64 else 0, rows, L, ncell, blocks, _ptr(X),
                                     _ptr(keys), _ptr(stats), s))
    tick("sort")
    sk, order = torch.sort(keys)
    del keys
    tick("gather")
    bad = int(stats.item())
    if bad:
        raise ValueError("pair_counts: %d row(s) have a non-finite position or one 2^20 boxes or more away" % bad)
    P = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    _lib.check(l.nbe_fof_gather(_ptr(X), _ptr(order), rows, blocks, _ptr(P), s))
    return P, sk


def _count(A, B, L, T, ncell, nmu, los, blocks, form=None, timer=None):
    """Device work of pair_counts: the (nb, nmu) int64 count tensor.  `form` as nbe_pair_count_form (None: the library's
    choice); `timer(name)` is called before every stage (coords, sort, gather per catalogue, then count) and timer(None) at
    the end (tools/time_pairs.py)."""
    l = _lib.lib()
    dev = _device_of(A[0])
    tick = timer or (lambda name: None)
    nb = len(T) - 1
    thresholds = (C.c_int64 * (nb + 1))(*T)
    with torch.cuda.device(dev):
        s = _stream(dev)
        PA, skA = _sorted_records(l, A[0], A[1], A[2], L, ncell, blocks, dev, s, tick)
        PB = skB = None
        if B is not None:
            PB, skB = _sorted_records(l, B[0], B[1], B[2], L, ncell, blocks, dev, s, tick)
        tick("count")
        counts = torch.zeros((nb, nmu), dtype=torch.int64, device=dev)
        args = (_ptr(PA), _ptr(skA), A[2], _ptr(PB) if B is not None else None, _ptr(skB) if B is not None else None,
                B[2] if B is not None else 0, ncell, thresholds, nb, nmu, los, blocks)
        if form is None:
            _lib.check(l.nbe_pair_count(*args, _ptr(counts), s))
        else:
            _lib.check(l.nbe_pair_count_form(*args, int(form), _ptr(counts), s))
        tick(None)
    return counts


def pair_counts(a, boxsize, r_edges, b=None, nmu=None, los=2, _max_blocks=None):
    """Pairs per bin of separation of one catalogue (b=None: each unordered pair of distinct rows once) or between two
    (every row of a with every row of b): Corrfunc's theory.DD / DDsmu, nbodykit's SimulationBox2PCF pair counts.  The
    module docstring has the definition.

    a, b: each a (count, 3) float32 / float64 array of positions or a (3, n, n, n) float32 / float16 displacement of the
    lattice, NumPy arrays or CUDA tensors on one device.  boxsize: L (scalar, or a 3-tuple of equal values).  r_edges:
    nb + 1 strictly increasing lengths, 0 <= r_0, r_nb < L / 3, 1 <= nb <= 128.  nmu: None, or 1 .. 32 uniform bins of
    mu = |d_los| / |d| about array axis los, with nb nmu <= 4096.  `_max_blocks` caps the grid of every launch (tests): the
    counts do not depend on it.

    Returns a dict: npairs int64 of shape (nb,), or (nb, nmu) with nmu; r_edges float64; thresholds int64; with nmu mu_edges
    float64 -- NumPy arrays for NumPy input, tensors on the input's device for tensors --, ncell, count_a and count_b (ints;
    count_b is None for an auto count).

    Raises ValueError, before any device work, for bad shapes, kinds or edges; ValueError for a non-finite position or
    |x_c / L| >= 2^20 (no partial result is returned); NBEError when the device's free memory cannot take 96 bytes per row."""
    A, B, L, edges, T, ncell, nmu, los, blocks = _validate(a, boxsize, r_edges, b, nmu, los, _max_blocks)
    dev = _device_of(A[0])
    rows = A[2] + (B[2] if B is not None else 0)
    _check_free_memory(dev, BYTES_PER_PARTICLE * rows, "pair_counts: %d rows" % rows, "%d bytes each" % BYTES_PER_PARTICLE)
    counts = _count(A, B, L, T, ncell, 1 if nmu is None else nmu, los, blocks)
    if nmu is None:
        counts = counts.reshape(-1)
    kind = (lambda v: torch.from_numpy(v).to(dev)) if _is_torch(A[0]) else (lambda v: v)
    out = {"npairs": counts if _is_torch(A[0]) else counts.cpu().numpy(), "r_edges": kind(edges),
           "thresholds": kind(np.array(T, dtype=np.int64))}
    if nmu is not None:
        out["mu_edges"] = kind(np.arange(nmu + 1, dtype=np.float64) / nmu)
    out.update(ncell=ncell, count_a=A[2], count_b=None if B is None else B[2])
    return out


def analytic_rr(r_edges, boxsize, count_a, count_b=None, nmu=None):
    """Expected pairs of unclustered catalogues, float64 (nb,) or (nb, nmu): N (N - 1) / 2 V_b / L^3 dmu for an auto count
    (count_b None), N_a N_b V_b / L^3 dmu for a cross count, with V_b = 4 pi / 3 (r_{b+1}^3 - r_b^3) and dmu = 1 / nmu."""
    e = np.asarray(r_edges, dtype=np.float64)
    vol = 4.0 * np.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
    norm = 0.5 * float(count_a) * (float(count_a) - 1.0) if count_b is None else float(count_a) * float(count_b)
    rr = norm * vol / float(boxsize) ** 3
    return rr if nmu is None else np.repeat(rr[:, None] / float(nmu), nmu, axis=1)


def legendre_bin_integrals(nmu):
    """(3, nmu) float64: the integrals of L_0, L_2, L_4 over the bins [m / nmu, (m + 1) / nmu], from the antiderivatives mu,
    (mu^3 - mu) / 2 and (7 mu^5 - 10 mu^3 + 3 mu) / 8.  Over all bins they sum to 1, 0, 0."""
    mu = np.arange(nmu + 1, dtype=np.float64) / nmu
    anti = np.stack([mu, 0.5 * (mu ** 3 - mu), (7.0 * mu ** 5 - 10.0 * mu ** 3 + 3.0 * mu) / 8.0])
    return anti[:, 1:] - anti[:, :-1]


def multipoles(xi):
    """(xi0, xi2, xi4) of xi (nb, nmu): (2 l + 1) sum_m xi[:, m] int_bin L_l."""
    w = legendre_bin_integrals(xi.shape[1])
    return tuple((2 * ell + 1) * (xi * w[i][None, :]).sum(axis=1) for i, ell in enumerate((0, 2, 4)))


def correlation_function(a, boxsize, r_edges, b=None, nmu=None, los=2):
    """xi = DD / RR - 1 with the analytic RR of a periodic box: pair_counts's dict with rr, xi (float64, the shape of npairs)
    and r_mid (the arithmetic bin centres) added, and with nmu the multipoles xi0, xi2, xi4 (nb,) of xi(s, mu) by the exact
    Legendre integrals over the mu bins.  Arguments and errors as pair_counts."""
    out = pair_counts(a, boxsize, r_edges, b=b, nmu=nmu, los=los)
    tens = _is_torch(out["npairs"])
    dev = out["npairs"].device if tens else None
    host = (lambda v: v.cpu().numpy()) if tens else (lambda v: v)
    edges = host(out["r_edges"])
    L = float(np.asarray(boxsize, dtype=np.float64).ravel()[0])
    rr = analytic_rr(edges, L, out["count_a"], out["count_b"], nmu)
    with np.errstate(divide="ignore", invalid="ignore"):                    # one row against itself has RR = 0
        xi = host(out["npairs"]).astype(np.float64) / rr - 1.0
    new = {"rr": rr, "xi": xi, "r_mid": 0.5 * (edges[1:] + edges[:-1])}
    if nmu is not None:
        new["xi0"], new["xi2"], new["xi4"] = multipoles(xi)
    for k, v in new.items():
        out[k] = torch.from_numpy(v).to(dev) if tens else v
    return out
