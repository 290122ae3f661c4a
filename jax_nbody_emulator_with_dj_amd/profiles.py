"""Radial profiles and spherical-overdensity masses around centres, on the GPU: the profile and SO step of a halo finder
such as Rockstar or AHF.  The reference has no such step; its scripts/halos.py gives a halo its FoF Length only.

    from jax_nbody_emulator_with_dj_amd.profiles import radial_counts, density_profile, spherical_overdensity, profile_edges

    edges = profile_edges(0.05, 5.0, 20)                                            # [0, geomspace(0.05, 5, 20)]
    rc = radial_counts(cat["CMPosition"], displacement, 1000.0, edges)              # counts (H, 20) int64
    prof = density_profile(rc["counts"], rc["r_edges"], 1000.0, rc["count_b"])      # rho / rho_mean, enclosed, r_mid
    so = spherical_overdensity(rc["counts"], rc["r_edges"], 1000.0, rc["count_b"], overdensity=200.0)   # R, N, flag

Definition (tests/profiles_ref.py restates it in NumPy).  Coordinates, the minimum-image d^2 in
64-bit integers, the thresholds T_b = floor((r_b / L)^2 2^60) (T_0 = -1 for r_0 = 0) and the rule T_b < d^2 <= T_{b+1} are
those of correlation.pair_counts, whose code decides every bin: counts[h, b] is the number of rows of `matter` in the shell
(r_b, r_{b+1}] about centre h, a row that coincides with the centre included (in bin 0 iff r_0 = 0).  Counts are sums of
ones: the same bits for every launch geometry, form of the kernel, order of the matter rows and stream; permuting the
centres permutes the rows.  The column sums are pair_counts(a=centres, b=matter)["npairs"].

Spherical overdensity, on the host in float64 from the exact integers, with nbar = count_b / L^3 and r_0 = 0:
N_j = sum_{b <= j} counts[h, b], D_j = N_j / (nbar 4 pi / 3 r_{j+1}^3), Delta = overdensity ("mean") or overdensity /
Omega_m(z) ("critical").  j* is the smallest j with D_j < Delta; j* = 0 gives flag 1 (below Delta already at the first
edge), no such j flag 2 (r_max too small), both with NaN radius and mass; otherwise ln R is the linear interpolation in
(ln r, ln D) between (r_{j*}, D_{j*-1}) and (r_{j*+1}, D_{j*}), and N = Delta nbar 4 pi / 3 R^3.

Velocity profiles: radial_velocity_moments adds, beside every count, the five integer sums of
correlation.pairwise_velocity for the pairs (centre, row of matter), and velocity_profile forms the infall v_r and the
dispersions sigma_r, sigma_t per shell from them.

    vm = radial_velocity_moments(cat["CMPosition"], cat["CMVelocity"], displacement, velocity, 1000.0, edges)
    vp = velocity_profile(vm["counts"], vm["sums"], vm["exponent"])                 # v_r, sigma_r, sigma_t (H, 20)

Not built: unbinding, an exact sort-based R_Delta, most-bound centres, weights, r_max >= L / 3.

Residency as in correlation.py: NumPy in gives NumPy out, CUDA tensors in give CUDA tensors on their device, on torch's
current stream.  There is no CPU fallback.  Arguments are validated before any device work.
"""

import ctypes as C
import math
import numbers

import numpy as np

from . import _lib
from . import correlation as CF
from .density import _check_free_memory, _check_max_blocks, _device_of, _is_torch, _ptr, _same_kind, _stream, _triple

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["radial_counts", "density_profile", "spherical_overdensity", "stack_profiles", "profile_edges"]
# the velocity functions (radial_velocity_moments, velocity_profile, stack_velocity_profiles) are imported by name: the
# star-import surface stays what tests/test_profiles_host.py pins

FORMS = (0, 1)                  # nbe_halo_profiles_form: a workgroup per centre, a wave per centre


def profile_edges(rmin, rmax, nbins):
    """The nbins + 1 edges [0, geomspace(rmin, rmax, nbins)]: a first bin (0, rmin] and nbins - 1 logarithmic ones up to
    rmax.  ValueError unless 0 < rmin < rmax, both finite, and nbins >= 2."""
    if isinstance(nbins, (bool, np.bool_)) or not isinstance(nbins, numbers.Integral) or nbins < 2:
        raise ValueError("profile_edges: nbins must be an int >= 2, got %r" % (nbins,))
    if not (np.isfinite(rmin) and np.isfinite(rmax)) or not 0.0 < rmin < rmax:
        raise ValueError("profile_edges needs 0 < rmin < rmax, got %r, %r" % (rmin, rmax))
    return np.concatenate([[0.0], np.geomspace(float(rmin), float(rmax), int(nbins))])


def _validate(centres, matter, boxsize, r_edges, max_blocks, form):
    A = CF._catalogue(centres, "centres")
    if A[1] != "positions":
        raise ValueError("radial_counts: centres must be (H, 3) positions, got shape %s" % (tuple(A[0].shape),))
    B = CF._catalogue(matter, "matter")
    _same_kind(A[0], B[0], "radial_counts: centres", "matter")
    L = _triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("radial_counts needs a cubic box, got boxsize %s" % (L,))
    edges, T, ncell = CF.pair_geometry(L[0], r_edges)
    blocks = _check_max_blocks(max_blocks, "radial_counts")
    if form is not None and (isinstance(form, (bool, np.bool_)) or form not in FORMS):
        raise ValueError("radial_counts: _form must be None, 0 or 1, got %r" % (form,))
    return A, B, L[0], edges, T, ncell, blocks, form


def _count(A, B, L, T, ncell, blocks, form=None, timer=None, records=None):
    """Device work of radial_counts: the (H, nb) int64 count tensor.  `form` as nbe_halo_profiles_form (None: the library's
    choice); `timer(name)` is called before every stage (coords, sort, gather per catalogue, then count) and timer(None) at
    the end; `records` receives the sorted records and keys of both catalogues (tools/time_profiles.py)."""
    l = _lib.lib()
    dev = _device_of(A[0])
    tick = timer or (lambda name: None)
    nb = len(T) - 1
    thresholds = (C.c_int64 * (nb + 1))(*T)
    with torch.cuda.device(dev):
        s = _stream(dev)
        PA, skA = CF._sorted_records(l, A[0], A[1], A[2], L, ncell, blocks, dev, s, tick)
        PB, skB = CF._sorted_records(l, B[0], B[1], B[2], L, ncell, blocks, dev, s, tick)
        tick("count")
        counts = torch.empty((A[2], nb), dtype=torch.int64, device=dev)             # every row is written whole
        args = (_ptr(PA), _ptr(skA), A[2], _ptr(PB), _ptr(skB), B[2], ncell, thresholds, nb, blocks)
        if form is None:
            _lib.check(l.nbe_halo_profiles(*args, _ptr(counts), s))
        else:
            _lib.check(l.nbe_halo_profiles_form(*args, int(form), _ptr(counts), s))
        tick(None)
        if records is not None:
            records.update(PA=PA, skA=skA, PB=PB, skB=skB)
    return counts


def radial_counts(centres, matter, boxsize, r_edges, _max_blocks=None, _form=None):
    """Rows of `matter` per shell of separation about every centre.  The module docstring has the definition.

    centres: (H, 3) float32 / float64 positions, any number of boxes away.  matter: (count, 3) float32 / float64 positions or
    a (3, n, n, n) float32 / float16 displacement of the lattice.  Both NumPy arrays, or CUDA tensors on one device.
    boxsize: L (scalar, or a 3-tuple of equal values).  r_edges: nb + 1 strictly increasing lengths, 0 <= r_0,
    r_nb < L / 3, 1 <= nb <= 128.  `_max_blocks` caps the grid of every launch and `_form` picks the kernel's form (0 a
    workgroup per centre, 1 a wave per centre) for the tests: the counts depend on neither.

    Returns a dict: counts int64 (H, nb), r_edges float64, thresholds int64 -- NumPy arrays for NumPy input, tensors on the
    input's device for tensors --, ncell, count_a (H) and count_b (ints).

    Raises ValueError, before any device work, for bad shapes, kinds or edges; ValueError for a non-finite position or
    |x_c / L| >= 2^20 (no partial result is returned); NBEError when the device's free memory cannot take 96 bytes per row
    of both catalogues plus 8 H nb for the counts."""
    A, B, L, edges, T, ncell, blocks, form = _validate(centres, matter, boxsize, r_edges, _max_blocks, _form)
    dev = _device_of(A[0])
    rows, H, nb = A[2] + B[2], A[2], len(T) - 1
    _check_free_memory(dev, CF.BYTES_PER_PARTICLE * rows + 8 * H * nb, "radial_counts: %d rows and %d x %d counts" % (rows, H, nb),
                       "%d bytes a row, 8 a count" % CF.BYTES_PER_PARTICLE)
    counts = _count(A, B, L, T, ncell, blocks, form)
    tens = _is_torch(A[0])
    kind = (lambda v: torch.from_numpy(v).to(dev)) if tens else (lambda v: v)
    return {"counts": counts if tens else counts.cpu().numpy(), "r_edges": kind(edges),
            "thresholds": kind(np.array(T, dtype=np.int64)), "ncell": ncell, "count_a": A[2], "count_b": B[2]}


def _host(a):
    return a.cpu().numpy() if _is_torch(a) else np.asarray(a)


def _count_table(counts, r_edges, what):
    c = _host(counts)
    e = np.asarray(_host(r_edges), dtype=np.float64)
    if c.ndim != 2 or c.dtype.kind not in "iu" or e.ndim != 1 or e.size != c.shape[1] + 1:
        raise ValueError("%s: counts must be an (H, nb) integer table and r_edges its nb + 1 edges, got %s %s and %s"
                         % (what, c.dtype, c.shape, e.shape))
    if not np.isfinite(e).all() or e[0] < 0.0 or not (np.diff(e) > 0.0).all():
        raise ValueError("%s: r_edges must be finite and strictly increasing from 0 or more, got %s" % (what, e))
    return c.astype(np.int64), e


def _mean_density(boxsize, count_b, what):
    L = float(boxsize)
    if isinstance(count_b, (bool, np.bool_)) or not isinstance(count_b, numbers.Integral) or count_b < 1 or not L > 0.0:
        raise ValueError("%s needs a positive boxsize and count_b >= 1, got %r, %r" % (what, boxsize, count_b))
    return float(count_b) / L ** 3


def density_profile(counts, r_edges, boxsize, count_b):
    """The profile of radial_counts's table, on the host in float64: a dict with rho (H, nb), the shell density in units of
    the mean, counts / (nbar V_shell) with nbar = count_b / L^3 and V_shell = 4 pi / 3 (r_{b+1}^3 - r_b^3); enclosed (H, nb)
    int64, the cumulative counts (the rows within r_{b+1} when r_0 = 0); r_mid (nb,), the arithmetic bin centres."""
    c, e = _count_table(counts, r_edges, "density_profile")
    nbar = _mean_density(boxsize, count_b, "density_profile")
    shell = 4.0 * np.pi / 3.0 * (e[1:] ** 3 - e[:-1] ** 3)
    return {"rho": c.astype(np.float64) / (nbar * shell)[None, :], "enclosed": np.cumsum(c, axis=1),
            "r_mid": 0.5 * (e[1:] + e[:-1])}


def omega_m_of_z(Om, z):
    """Omega_m(z) = Om (1 + z)^3 / (Om (1 + z)^3 + 1 - Om) of a flat LCDM model."""
    a3 = float(Om) * (1.0 + float(z)) ** 3
    return a3 / (a3 + 1.0 - float(Om))


def spherical_overdensity(counts, r_edges, boxsize, count_b, overdensity=200.0, reference="mean", Om=None, z=0.0,
                          particle_mass=None):
    """Spherical-overdensity radius and mass of every row of radial_counts's table, on the host in float64 from the exact
    integers (the module docstring has the definition).  r_edges[0] must be 0.  reference: "mean" (Delta = overdensity
    times the mean matter density) or "critical" (Delta = overdensity / Omega_m(z); Om is required).

    Returns a dict: R (H,) the radius, N (H,) the particle number Delta nbar 4 pi / 3 R^3, M = N particle_mass or None, flag
    (H,) int8 -- 0 found, 1 below Delta already at the first edge, 2 never below Delta (r_max too small); R, N and M are NaN
    where flag != 0 --, and delta_eff, the Delta used."""
    c, e = _count_table(counts, r_edges, "spherical_overdensity")
    if e[0] != 0.0:
        raise ValueError("spherical_overdensity needs r_edges[0] == 0 (enclosed counts), got %g" % e[0])
    nbar = _mean_density(boxsize, count_b, "spherical_overdensity")
    if isinstance(overdensity, (bool, np.bool_)) or not isinstance(overdensity, numbers.Real) or \
            not np.isfinite(float(overdensity)) or float(overdensity) <= 0.0:
        raise ValueError("spherical_overdensity: overdensity must be a positive number, got %r" % (overdensity,))
    if reference not in ("mean", "critical"):
        raise ValueError("spherical_overdensity: reference must be 'mean' or 'critical', got %r" % (reference,))
    delta = float(overdensity)
    if reference == "critical":
        if Om is None:
            raise ValueError("spherical_overdensity: reference='critical' needs Om")
        if not 0.0 < float(Om) <= 1.0 or not float(z) > -1.0:
            raise ValueError("spherical_overdensity: needs 0 < Om <= 1 and z > -1, got %r, %r" % (Om, z))
        delta = delta / omega_m_of_z(Om, z)
    H, nb = c.shape
    sphere = nbar * (4.0 * np.pi / 3.0) * e[1:] ** 3
    D = np.cumsum(c, axis=1).astype(np.float64) / sphere[None, :]
    below = D < delta
    jstar = np.where(below.any(axis=1), below.argmax(axis=1), nb)
    flag = np.where(jstar == 0, 1, np.where(jstar == nb, 2, 0)).astype(np.int8)
    R = np.full(H, np.nan)
    ok = np.nonzero(flag == 0)[0]
    if ok.size:
        j = jstar[ok]
        x0, x1 = np.log(e[j]), np.log(e[j + 1])
        y0, y1 = np.log(D[ok, j - 1]), np.log(D[ok, j])                             # D_{j-1} >= Delta > D_j > 0: N_j >= N_{j-1} > 0
        t = (y0 - math.log(delta)) / (y0 - y1)
        R[ok] = np.exp(x0 + t * (x1 - x0))
    N = delta * nbar * (4.0 * np.pi / 3.0) * R ** 3
    return {"R": R, "N": N, "M": None if particle_mass is None else N * float(particle_mass), "flag": flag,
            "delta_eff": delta}


def stack_profiles(counts, lengths, length_edges):
    """Integer sums of the rows of a count table per bin of Length: (stacked (nl, nb) int64, halos (nl,) int64) for the
    nl + 1 increasing length_edges; a halo is in bin i iff length_edges[i] <= Length < length_edges[i + 1]."""
    c = _host(counts)
    n = _host(lengths)
    le = np.asarray(length_edges)
    if c.ndim != 2 or c.dtype.kind not in "iu" or n.shape != (c.shape[0],):
        raise ValueError("stack_profiles: counts must be an (H, nb) integer table and lengths (H,), got %s and %s"
                         % (c.shape, n.shape))
    if le.ndim != 1 or le.size < 2 or not (np.diff(le) > 0).all():
        raise ValueError("stack_profiles: length_edges must be 2 or more increasing numbers, got %r" % (length_edges,))
    which = np.searchsorted(le, n, side="right") - 1
    stacked = np.zeros((le.size - 1, c.shape[1]), np.int64)
    halos = np.zeros(le.size - 1, np.int64)
    inside = (which >= 0) & (which < le.size - 1)
    np.add.at(stacked, which[inside], c[inside].astype(np.int64))
    np.add.at(halos, which[inside], 1)
    return stacked, halos


# ---- velocity moments about centres ---------------------------------------------------------------

def _velocity_count(A, VA, B, VB, L, T, ncell, blocks, form=None, timer=None, records=None):
    """Device work of radial_velocity_moments: ((H, nb, 6) int64 tensor of N and the five sums, the exponent).  VA None:
    centres at rest.  `form`, `timer` and `records` as _count (tools/time_pairvel.py)."""
    l = _lib.lib()
    dev = _device_of(A[0])
    tick = timer or (lambda name: None)
    nb = len(T) - 1
    thresholds = (C.c_int64 * (nb + 1))(*T)
    with torch.cuda.device(dev):
        s = _stream(dev)
        tick("range")
        va = None if VA is None else CF._on_device(VA, dev)
        vb = CF._on_device(VB, dev)
        e = CF._velocity_exponent(l, [vb] if va is None else [va, vb], s, dev, "radial_velocity_moments")
        PA, skA = CF._sorted_records(l, A[0], A[1], A[2], L, ncell, blocks, dev, s, tick)
        PB, skB = CF._sorted_records(l, B[0], B[1], B[2], L, ncell, blocks, dev, s, tick)
        tick("words")
        WA = None if va is None else CF._velocity_words(l, va, A[1], A[2], e, PA, blocks, dev, s)
        WB = CF._velocity_words(l, vb, B[1], B[2], e, PB, blocks, dev, s)
        tick("moments")
        sums = torch.empty((A[2], nb, 6), dtype=torch.int64, device=dev)            # every row is written whole
        args = (_ptr(PA), _ptr(skA), _ptr(WA) if WA is not None else None, A[2], _ptr(PB), _ptr(skB), _ptr(WB), B[2], ncell,
                thresholds, nb, blocks)
        if form is None:
            _lib.check(l.nbe_halo_velocity_profiles(*args, _ptr(sums), s))
        else:
            _lib.check(l.nbe_halo_velocity_profiles_form(*args, int(form), _ptr(sums), s))
        tick(None)
        if records is not None:
            records.update(PA=PA, skA=skA, WA=WA, PB=PB, skB=skB, WB=WB)
    return sums, e


def radial_velocity_moments(centres, centre_velocity, matter, matter_velocity, boxsize, r_edges, _max_blocks=None, _form=None):
    """The velocity moments of `matter` per shell about every centre: radial_counts's counts and, beside each, the five
    integer sums of correlation.pairwise_velocity for the pairs (centre, row of matter) -- infall and dispersion profiles.
    correlation's module docstring has the definition; the velocity of a pair is the matter's minus the centre's, and its
    radial word is negative for infall.

    centres, matter, boxsize, r_edges: as radial_counts.  centre_velocity: (H, 3) float32 / float64, or None for centres at
    rest (the matter velocity is then taken in the box frame).  matter_velocity: of the shape of matter, (count, 3) float32
    / float64 or (3, n, n, n) float32 / float16.  All of one kind and device.  `_max_blocks` and `_form` as radial_counts:
    the sums depend on neither.

    Returns a dict: counts int64 (H, nb), the bits of radial_counts's; sums int64 (H, nb, 5): S1, vr^2 low and high, |dW|^2
    low and high; r_edges float64; thresholds int64 -- NumPy arrays for NumPy input, tensors on the input's device for
    tensors --, exponent, ncell, count_a (H) and count_b (ints).  velocity_profile turns counts and sums into v_r, sigma_r
    and sigma_t.  The column sums over the centres are pairwise_velocity(a=centres, b=matter)'s.

    Raises as radial_counts, and ValueError for a non-finite velocity; the memory check takes 112 bytes per row of both
    catalogues plus 48 H nb."""
    A, B, L, edges, T, ncell, blocks, form = _validate(centres, matter, boxsize, r_edges, _max_blocks, _form)
    VA = None if centre_velocity is None else CF._velocity(centre_velocity, A, "centre_velocity", "radial_velocity_moments")
    VB = CF._velocity(matter_velocity, B, "matter_velocity", "radial_velocity_moments")
    dev = _device_of(A[0])
    rows, H, nb = A[2] + B[2], A[2], len(T) - 1
    each = CF.BYTES_PER_PARTICLE + CF.VELOCITY_BYTES
    _check_free_memory(dev, each * rows + 48 * H * nb, "radial_velocity_moments: %d rows and %d x %d x 6 sums" % (rows, H, nb),
                       "%d bytes a row, 48 a bin" % each)
    table, e = _velocity_count(A, VA, B, VB, L, T, ncell, blocks, form)
    tens = _is_torch(A[0])
    kind = (lambda v: torch.from_numpy(v).to(dev)) if tens else (lambda v: v)
    host = None if tens else table.cpu().numpy()
    return {"counts": table[:, :, 0].contiguous() if tens else host[:, :, 0].copy(),
            "sums": table[:, :, 1:].contiguous() if tens else host[:, :, 1:].copy(), "r_edges": kind(edges),
            "thresholds": kind(np.array(T, dtype=np.int64)), "exponent": e, "ncell": ncell, "count_a": A[2], "count_b": B[2]}


def velocity_profile(counts, sums, exponent):
    """The infall and dispersion profile of radial_velocity_moments's tables, on the host in float64 from the exact integers
    (correlation.velocity_moments): a dict with v_r, the mean radial velocity of the matter about the centre (negative:
    infall), sigma_r, the radial dispersion about that mean, and sigma_t, the dispersion per transverse direction, each
    of the shape of counts and NaN for an empty shell; vr2 and vt2, the second moments they come from.  counts (..., nb) and
    sums (..., nb, 5) may be a table per centre or integer sums of such tables over halos (stack_velocity_profiles)."""
    m = CF.velocity_moments(counts, sums, exponent)
    return {"v_r": m["v12"], "sigma_r": m["sigma_r"], "sigma_t": m["sigma_t"], "vr2": m["vr2"], "vt2": m["vt2"]}


def stack_velocity_profiles(counts, sums, lengths, length_edges):
    """stack_profiles for radial_velocity_moments's tables: (stacked counts (nl, nb), stacked sums (nl, nb, 5), halos (nl,)),
    all int64 -- every sum is an integer, so a stack of halos is the sum of their rows, and velocity_profile takes it as it
    takes one halo's."""
    c, s = _host(counts), _host(sums)
    if c.ndim != 2 or s.shape != c.shape + (5,) or s.dtype.kind not in "iu":
        raise ValueError("stack_velocity_profiles: counts must be an (H, nb) integer table and sums (H, nb, 5), got %s and %s"
                         % (c.shape, s.shape))
    stacked, halos = stack_profiles(c, lengths, length_edges)
    ssum, _ = stack_profiles(s.reshape(c.shape[0], -1), lengths, length_edges)
    return stacked, ssum.reshape(stacked.shape + (5,)), halos
