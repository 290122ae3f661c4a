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

Pairwise velocities (tests/pairvel_ref.py restates them): pairwise_velocity gives, per radial bin of
the same pairs, the mean streaming velocity v12(r) and the dispersions sigma_r(r), sigma_t(r) of the streaming model.  One
exponent e per call with max |v_c| < 2^e over all components of both catalogues; W_c = rint(v_c 2^(20 - e)).  For a pair (a, o):
d_c the minimum-image X_c(o) - X_c(a), dW_c = W_c(o) - W_c(a), u = sum dW_c d_c in int64 and the radial word vr = sign(u)
floor(|u| / |d| + 1/2), decided by 128-bit integer comparisons (0 for d = 0; vr < 0 is approach).  A bin holds N and five
int64 sums: S1 = sum vr, sum (vr^2 & (2^24 - 1)), sum (vr^2 >> 24) and the same two of |dW|^2, all fixed by the pair alone,
hence the same bits for every launch geometry, form, row order and stream.  On the host in float64: v12 = 2^(e - 20) S1 / N,
<v_r^2> = 4^(e - 20) (2^24 hi + lo) / N, sigma_r^2 = <v_r^2> - v12^2, <v_t^2> = (<|dv|^2> - <v_r^2>) / 2 per transverse
direction, NaN where N = 0.

Not built: weights, non-uniform mu bins, r_max >= L / 3, the mesh-based xi(r) (an inverse FFT of |delta_k|^2), and for the
velocities mu bins, pair weights and line-of-sight moments in (r, mu).

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

__all__ = ["pair_counts", "correlation_function", "pair_geometry", "analytic_rr", "legendre_bin_integrals", "multipoles",
           "pairwise_velocity", "velocity_moments"]

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


# ---- pairwise velocities ------------------------------------------------------------------------

VELOCITY_BITS, VELOCITY_SPLIT = 20, 24          # NBE_VELOCITY_BITS; a square below 2^44 is summed as its low 24 bits and the rest
MAX_PAIRS_PER_BIN = 1 << 39                     # beyond it a sum of squares' high parts could leave int64
VELOCITY_BYTES = 16                             # a velocity record per row, beside BYTES_PER_PARTICLE
VELOCITY_FORMS = (0, 1)                         # nbe_pair_velocity_form: the LDS image, global atomics


def _velocity(v, cat, name, what):
    """The velocity array of the catalogue `cat` (_catalogue's triple), validated: its shape, and float32 / float64 for
    positions, float32 / float16 for a lattice."""
    v = _check_array(v, name)
    if tuple(v.shape) != tuple(cat[0].shape):
        raise ValueError("%s: %s must have its catalogue's shape %s, got %s" % (what, name, tuple(cat[0].shape), tuple(v.shape)))
    ok = ("float32", "float64") if cat[1] == "positions" else ("float32", "float16")
    if _dtype_name(v) not in ok:
        raise ValueError("%s: %s must be %s or %s, got %s" % (what, name, ok[0], ok[1], _dtype_name(v)))
    _same_kind(cat[0], v, "%s: the catalogue" % what, name)
    return v


def _velocity_exponent(l, tensors, s, dev, what):
    """The exponent e of a call, max |v| < 2^e over every device tensor given (0 for all zeros): nbe_quantity_range on the
    values as one channel, the float64 maximum for float64.  ValueError for a non-finite value."""
    top, bad = 0.0, 0
    for vd in tensors:
        if vd.dtype == torch.float64:
            bad += int((~torch.isfinite(vd)).sum().item())
            top = max(top, float(torch.nan_to_num(vd, nan=0.0, posinf=0.0, neginf=0.0).abs().max().item()))
            continue
        rng = torch.zeros(2, dtype=torch.int32, device=dev)
        _lib.check(l.nbe_quantity_range(_ptr(vd), 1 if vd.dtype == torch.float16 else 0, 1, vd.numel(), _ptr(rng), s))
        r = rng.cpu().numpy()
        bad += int(r[1:].view(np.uint32)[0])
        top = max(top, float(r[:1].view(np.float32)[0]))
    if bad:
        raise ValueError("%s: %d value(s) of the velocity are not finite" % (what, bad))
    return int(math.frexp(top)[1])


def _velocity_words(l, vd, kind, rows, e, P, blocks, dev, s):
    """The velocity records (rows, 4) int32 parallel to the sorted records P."""
    W = torch.empty((rows, 4), dtype=torch.int32, device=dev)
    dtype = {torch.float32: 0, torch.float16: 1, torch.float64: 2}[vd.dtype]
    _lib.check(l.nbe_velocity_words(_ptr(vd), dtype, 1 if kind == "lattice" else 0, rows, e, _ptr(P), blocks, _ptr(W), s))
    return W


def _moments(A, VA, B, VB, L, T, ncell, blocks, form=None, timer=None, records=None):
    """Device work of pairwise_velocity: ((nb, 6) int64 tensor of N and the five sums, the exponent).  `form` as
    nbe_pair_velocity_form (None: the library's choice); `timer` and `records` as profiles._count (tools/time_pairvel.py)."""
    l = _lib.lib()
    dev = _device_of(A[0])
    tick = timer or (lambda name: None)
    nb = len(T) - 1
    thresholds = (C.c_int64 * (nb + 1))(*T)
    with torch.cuda.device(dev):
        s = _stream(dev)
        tick("range")
        va = _on_device(VA, dev)
        vb = None if B is None else _on_device(VB, dev)
        e = _velocity_exponent(l, [va] if vb is None else [va, vb], s, dev, "pairwise_velocity")
        PA, skA = _sorted_records(l, A[0], A[1], A[2], L, ncell, blocks, dev, s, tick)
        PB = skB = WB = None
        if B is not None:
            PB, skB = _sorted_records(l, B[0], B[1], B[2], L, ncell, blocks, dev, s, tick)
        tick("words")
        WA = _velocity_words(l, va, A[1], A[2], e, PA, blocks, dev, s)
        if B is not None:
            WB = _velocity_words(l, vb, B[1], B[2], e, PB, blocks, dev, s)
        tick("moments")
        sums = torch.zeros((nb, 6), dtype=torch.int64, device=dev)
        opt = lambda t: _ptr(t) if t is not None else None
        args = (_ptr(PA), _ptr(skA), _ptr(WA), A[2], opt(PB), opt(skB), opt(WB), B[2] if B is not None else 0, ncell,
                thresholds, nb, blocks)
        if form is None:
            _lib.check(l.nbe_pair_velocity(*args, _ptr(sums), s))
        else:
            _lib.check(l.nbe_pair_velocity_form(*args, int(form), _ptr(sums), s))
        tick(None)
        if records is not None:
            records.update(PA=PA, skA=skA, WA=WA, PB=PB, skB=skB, WB=WB)
    return sums, e


def check_pairs_per_bin(npairs, what):
    """NBEError where a bin holds more than 2^39 pairs: vr^2, |dW|^2 < 2^44 keep the low sums below 2^63 for any count, the
    high sums (below 2^20 a pair) only up to 2^43 pairs, and S1 (|vr| < 2^23) up to 2^40; 2^39 leaves a factor of two."""
    top = int(np.max(npairs)) if np.size(npairs) else 0
    if top > MAX_PAIRS_PER_BIN:
        raise _lib.NBEError("%s: %d pairs in one bin exceed 2^39: the velocity sums could leave int64" % (what, top))


def velocity_moments(npairs, sums, exponent):
    """The float64 moments of the exact integers, on the host: a dict v12, vr2, sigma_r, vt2, sigma_t of the shape of npairs.
    npairs (...,) and sums (..., 5) are pairwise_velocity's (or radial_velocity_moments's counts and sums, or sums of them
    over halos); exponent its e.  v12 = 2^(e - 20) S1 / N; vr2 = <v_r^2> = 4^(e - 20) (2^24 hi + lo) / N; sigma_r =
    sqrt(max(vr2 - v12^2, 0)); vt2 = (<|dv|^2> - vr2) / 2, per transverse direction; sigma_t = sqrt(max(vt2, 0)) -- the
    rounding of a radial word can carry vr2 past <|dv|^2> by a unit of 4^(e - 20) where the motion is radial.  NaN where
    N = 0."""
    host = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    n, s = host(npairs), host(sums)
    if n.dtype.kind not in "iu" or s.dtype.kind not in "iu" or s.shape != n.shape + (5,):
        raise ValueError("velocity_moments: npairs must be an integer table and sums its (..., 5) sums, got %s %s and %s %s"
                         % (n.dtype, n.shape, s.dtype, s.shape))
    if isinstance(exponent, (bool, np.bool_)) or not isinstance(exponent, numbers.Integral):
        raise ValueError("velocity_moments: exponent must be an int, got %r" % (exponent,))
    nf, f = n.astype(np.float64), s.astype(np.float64)
    unit, split = math.ldexp(1.0, int(exponent) - VELOCITY_BITS), float(1 << VELOCITY_SPLIT)
    with np.errstate(divide="ignore", invalid="ignore"):
        v12 = unit * f[..., 0] / nf
        vr2 = unit * unit * (split * f[..., 2] + f[..., 1]) / nf
        dv2 = unit * unit * (split * f[..., 4] + f[..., 3]) / nf
        vt2 = 0.5 * (dv2 - vr2)
        return {"v12": v12, "vr2": vr2, "sigma_r": np.sqrt(np.maximum(vr2 - v12 * v12, 0.0)), "vt2": vt2,
                "sigma_t": np.sqrt(np.maximum(vt2, 0.0))}


def _check_form(form, forms, what):
    if form is not None and (isinstance(form, (bool, np.bool_)) or form not in forms):
        raise ValueError("%s: _form must be None or one of %s, got %r" % (what, forms, form))
    return form


def pairwise_velocity(a, vel_a, boxsize, r_edges, b=None, vel_b=None, _max_blocks=None, _form=None):
    """The mean pairwise (streaming) velocity v12(r) and the pairwise dispersions sigma_r(r), sigma_t(r) of one catalogue
    (b=None: each unordered pair of distinct rows once) or between two: the ingredients of the streaming model of
    xi(s, mu).  The module docstring has the definition.

    a, b: catalogues as pair_counts takes them.  vel_a, vel_b: their velocities, of the catalogue's shape -- (count, 3)
    float32 / float64 beside positions, (3, n, n, n) float32 / float16 beside a displacement --, finite, of the catalogue's
    kind and device; vel_b goes with b.  boxsize, r_edges: as pair_counts.  `_max_blocks` caps the grid of every launch and
    `_form` picks the kernel's form (0 the LDS image, 1 global atomics) for the tests: the sums depend on neither.

    Returns a dict: npairs int64 (nb,), the bits of pair_counts's; sums int64 (nb, 5): S1, vr^2 low and high, |dW|^2 low and
    high; v12, vr2, sigma_r, vt2, sigma_t float64 (nb,) as velocity_moments forms them (v12 < 0: approach); r_edges float64;
    thresholds int64 -- NumPy arrays for NumPy input, tensors on the input's device for tensors --, exponent, ncell, count_a
    and count_b (ints; count_b is None for an auto count).

    Raises ValueError, before any device work, for bad shapes, kinds or edges; ValueError for a non-finite velocity or
    position or |x_c / L| >= 2^20 (no partial result is returned); NBEError when the device's free memory cannot take 112
    bytes per row, or when a bin holds more than 2^39 pairs."""
    A, B, L, edges, T, ncell, _, _, blocks = _validate(a, boxsize, r_edges, b, None, 2, _max_blocks)
    if (B is None) != (vel_b is None):
        raise ValueError("pairwise_velocity: b and vel_b go together")
    VA = _velocity(vel_a, A, "vel_a", "pairwise_velocity")
    VB = None if B is None else _velocity(vel_b, B, "vel_b", "pairwise_velocity")
    form = _check_form(_form, VELOCITY_FORMS, "pairwise_velocity")
    dev = _device_of(A[0])
    rows, each = A[2] + (B[2] if B is not None else 0), BYTES_PER_PARTICLE + VELOCITY_BYTES
    _check_free_memory(dev, each * rows, "pairwise_velocity: %d rows" % rows, "%d bytes each" % each)
    table, e = _moments(A, VA, B, VB, L, T, ncell, blocks, form)
    host = table.cpu().numpy()
    check_pairs_per_bin(host[:, 0], "pairwise_velocity")
    tens = _is_torch(A[0])
    kind = (lambda v: torch.from_numpy(v).to(dev)) if tens else (lambda v: v)
    out = {"npairs": table[:, 0].contiguous() if tens else host[:, 0].copy(),
           "sums": table[:, 1:].contiguous() if tens else host[:, 1:].copy()}
    out.update({k: kind(v) for k, v in velocity_moments(host[:, 0], host[:, 1:], e).items()})
    out.update(r_edges=kind(edges), thresholds=kind(np.array(T, dtype=np.int64)), exponent=e, ncell=ncell, count_a=A[2],
               count_b=None if B is None else B[2])
    return out
