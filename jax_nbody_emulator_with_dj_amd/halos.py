"""Friends-of-friends halos of an emulated box, on the GPU: the step of the reference's `scripts/halos.py`.

That script turns the saved displacement into particle positions (`:359-404`), runs nbodykit's MPI FoF finder on them
(`run_fof`, `:407-450`), writes `fof_catalog.npz` (`:871-881`) and derives the empirical halo mass function (`:317-349`).
Here the displacement stays where `process_box` left it:

    from jax_nbody_emulator_with_dj_amd.halos import fof_halos, particle_mass, halo_mass_function, density_slab

    cat = fof_halos(displacement, boxsize=1000.0, linking_length=0.2, nmin=20)      # CMPosition, Length, label, ...
    m = particle_mass(0.3175, 1000.0, 512)
    hmf = halo_mass_function(cat["Length"], 1000.0, m, np.linspace(12.5, 15.5, 31))
    slab, ncells = density_slab(delta, 1000.0, axis=0, center=500.0, width=20.0)
    delta_h, info = paint_halos(cat, 1000.0, res=512, min_length=100)               # the halo density contrast
    hb = halo_bias(cat, delta_m, 1000.0, min_length=100)                            # P_hh, P_mm, P_hm, r(k), bias, shot noise
    xi = halo_correlation(cat, 1000.0, np.linspace(1.0, 50.0, 21), min_length=100)  # xi_hh(r) by pair counts; matter=: xi_hm
    hp = halo_profiles(cat, displacement, 1000.0, profile_edges(0.05, 5.0, 20), overdensity=200.0)   # counts (H, 20), R, N
    vp = halo_velocity_profiles(cat, displacement, velocity, 1000.0, edges)         # v_r, sigma_r, sigma_t (H, nb); cat with CMVelocity
    v12 = halo_pairwise_velocity(cat, 1000.0, np.linspace(1.0, 50.0, 21))           # v12, sigma_r, sigma_t of the halos
    env = halo_environment(cat, delta_m, 1000.0, smoothing=8.0, threshold=0.2)      # eigenvalues, delta_s, web_type per halo

    python -m jax_nbody_emulator_with_dj_amd.halos --displacement_file emu_dis.npy --output_dir out/ [--halo_pk 256]
        [--halo_xi [--xi_rmin 1 --xi_rmax 50 --xi_nbins 20 --xi_log] [--xi_nmu N]]
        [--halo_profiles [--profile_rmin 0.05 --profile_rmax 5 --profile_nbins 20] [--so_overdensity 200 --so_reference mean]]
        [--velocity_file emu_vel.npy [--halo_vprofiles] [--halo_v12]]
        [--halo_environment 256 [--web_smoothing 8 --web_threshold 0.2]]

Definition (DESIGN.md section 12.5 has the proofs; tests/fof_ref.py restates it in NumPy).  With U = 2^30, particle
p = (i0 n + i1) n + i2 of the (n, n, n) lattice has the integer coordinates X_c = rint((i_c / n + psi_c / L) U) mod U,
formed in float64 from the stored float32 / float16 value: the lattice of `scripts/halos.py:394-403` in units of L / U.
The linking length is l = linking_length L / n, or linking_length itself with absolute=True (nbodykit's meanings), and
R2 = floor((l / L)^2 2^60).  The minimum-image difference d_c(p, q) is (X_c(p) - X_c(q)) mod U mapped to [-U/2, U/2);
p != q are linked iff d_0^2 + d_1^2 + d_2^2 <= R2 in 64-bit integers, so no rounding decides a link and coincident
particles link.  A group is a connected component of the links, its label its smallest particle index, Length its size; a
halo is a group with Length >= nmin; halos are ordered by Length descending, then label ascending.  With S_c the integer
sum of d_c(p, label) over the members, CMPosition_c = (((X_c(label) + S_c / Length) mod U) / U) L in float64: nbodykit's
periodic convention (offsets from one member), meaningful for groups narrower than L / 2.  With a velocity, channel c has
the exponent e_c of `paint_field` (max |v_c| < 2^e_c), a member adds rint(v 2^(24 - e_c)) to an integer sum, and
CMVelocity_c = sum 2^(e_c - 24) / Length.  All sums are integers: every output is the same bits for every launch
geometry, tie order of the sort and stream.

Residency as in density.py: NumPy in gives NumPy out, a CUDA tensor in gives CUDA tensors on its device, on torch's
current stream.  There is no CPU fallback.  Arguments are validated before any device work.
"""

import argparse
import ctypes as C
import math
import numbers
import os
import sys

import numpy as np

from . import _lib
from .density import (_back, _check_array, _check_free_memory, _check_los, _check_max_blocks, _device_of, _dtype_name,
                      _is_torch, _ptr, _real, _same_kind, _stream, _to_device, _triple)

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["fof_halos", "particle_mass", "halo_mass_function", "density_slab", "paint_halos", "halo_bias",
           "halo_correlation", "halo_profiles", "halo_velocity_profiles", "halo_pairwise_velocity",
           "halo_environment"]

_U = 1 << 30                    # include/nbe.h, "Halos": coordinate units per box side
_MIN_N, _MAX_N = 2, 1024        # NBE_FOF_MIN_N, NBE_FOF_MAX_N
_MAX_CELLS = 4096               # NBE_FOF_MAX_CELLS
BYTES_PER_PARTICLE = 72         # peak device memory of fof_halos beside its inputs
RHO_CRIT = 2.77536627e11        # h^2 M_sun / Mpc^3 (scripts/halos.py, RHO_CRIT_H2_MSUN_MPC3)


def _int(v, name, lo):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or int(v) < lo:
        raise ValueError("fof_halos: %s must be an int >= %d, got %r" % (name, lo, v))
    return int(v)


def linking_geometry(n, boxsize, linking_length, absolute):
    """(l, R2, ncell) of a call: the absolute linking length, floor((l / L)^2 2^60), and the cells per axis
    min(4096, U // (isqrt(R2) + 1)).  ValueError for a length that is not positive or leaves fewer than 3 cells."""
    b = _real(linking_length, "fof_halos: linking_length", positive=True)
    ell = b if absolute else b * boxsize / n
    if not ell < boxsize:
        raise ValueError("fof_halos: the linking length %g must stay below L / 3 = %g (at least 3 cells per axis)"
                         % (ell, boxsize / 3.0))
    R2 = int(math.floor((ell / boxsize) ** 2 * 2.0 ** 60))
    ncell = min(_MAX_CELLS, _U // (math.isqrt(R2) + 1))
    if ncell < 3:
        raise ValueError("fof_halos: the linking length %g must stay below L / 3 = %g (at least 3 cells per axis)"
                         % (ell, boxsize / 3.0))
    return ell, R2, ncell


def _validate(displacement, boxsize, linking_length, nmin, absolute, velocity, max_blocks):
    x = _check_array(displacement, "displacement")
    if x.ndim != 4 or x.shape[0] != 3 or len(set(x.shape[1:])) != 1:
        raise ValueError("fof_halos: displacement must have shape (3, n, n, n), got %s" % (tuple(x.shape),))
    if _dtype_name(x) not in ("float32", "float16"):
        raise ValueError("fof_halos: displacement must be float32 or float16, got %s" % _dtype_name(x))
    n = int(x.shape[1])
    if not _MIN_N <= n <= _MAX_N:
        raise ValueError("fof_halos: lattice size %d unsupported (%d .. %d)" % (n, _MIN_N, _MAX_N))
    L = _triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("fof_halos needs a cubic box, got boxsize %s" % (L,))
    nmin = _int(nmin, "nmin", 1)
    ell, R2, ncell = linking_geometry(n, L[0], linking_length, bool(absolute))
    v = None
    if velocity is not None:
        v = _check_array(velocity, "velocity")
        if tuple(v.shape) != tuple(x.shape):
            raise ValueError("fof_halos: velocity must have the displacement's shape %s, got %s"
                             % (tuple(x.shape), tuple(v.shape)))
        if _dtype_name(v) not in ("float32", "float16"):
            raise ValueError("fof_halos: velocity must be float32 or float16, got %s" % _dtype_name(v))
        _same_kind(x, v, "fof_halos: displacement", "velocity")
    return x, n, L[0], nmin, ell, R2, ncell, v, _check_max_blocks(max_blocks, "fof_halos")


def _velocity_exponents(l, vd, count, s, dev):
    """(C int[3]) e_c with max |v_c| < 2^e_c, by nbe_quantity_range; ValueError for a non-finite value."""
    rng = torch.zeros(4, dtype=torch.int32, device=dev)
    _lib.check(l.nbe_quantity_range(_ptr(vd), 1 if vd.dtype == torch.float16 else 0, 3, count, _ptr(rng), s))
    r = rng.cpu().numpy()
    if int(r[3]):
        raise ValueError("fof_halos: %d value(s) of the velocity are not finite" % int(r[3:].view(np.uint32)[0]))
    exps = (C.c_int * 3)()
    for c, e in enumerate(np.frexp(r[:3].view(np.float32).astype(np.float64))[1]):
        exps[c] = int(e)
    return exps


def _stages(xd, vd, n, L, nmin, R2, ncell, blocks, want_labels, wave_reduce=False, timer=None):
    """Device work of fof_halos on contiguous CUDA tensors.  Returns (label, length, X of the labels (H, 3), sums (H, 3 or 6)
    -- all host int64 arrays --, velocity exponents or None, ngroups, labels tensor or None).  wave_reduce adds runs of one halo inside a
    wave before the atomic: the same integers, slower where few particles belong to halos, so off.
    `timer(name)` is called before every stage (cells, sort, gather, link, labels, select, catalog, finish) and timer(None) at the end
    (tools/time_fof.py)."""
    l = _lib.lib()
    dev = xd.device
    count = n ** 3
    tick = timer or (lambda name: None)
    with torch.cuda.device(dev):
        s = _stream(dev)
        exps = None if vd is None else _velocity_exponents(l, vd, count, s, dev)
        tick("cells")
        X = torch.empty((3, count), dtype=torch.int32, device=dev)
        keys = torch.empty(count, dtype=torch.int64, device=dev)
        parent = torch.empty(count, dtype=torch.int32, device=dev)
        stats = torch.zeros(1, dtype=torch.int32, device=dev)
        _lib.check(l.nbe_fof_cells(_ptr(xd), 1 if xd.dtype == torch.float16 else 0, n, L, ncell, blocks, _ptr(X), _ptr(keys),
                                   _ptr(parent), _ptr(stats), s))
        tick("sort")
        sk, order = torch.sort(keys)
        del keys
        tick("gather")
        bad = int(stats.item())
        if bad:
            raise ValueError("fof_halos: %d particle(s) have a non-finite or out-of-range displacement" % bad)
        P = torch.empty((count, 4), dtype=torch.int32, device=dev)
        _lib.check(l.nbe_fof_gather(_ptr(X), _ptr(order), count, blocks, _ptr(P), s))
        del order
        tick("link")
        _lib.check(l.nbe_fof_link(_ptr(P), _ptr(sk), count, ncell, R2, blocks, _ptr(parent), s))
        tick("labels")
        del P, sk
        sizes = torch.zeros(count, dtype=torch.int32, device=dev)
        _lib.check(l.nbe_fof_labels(_ptr(parent), count, blocks, _ptr(sizes), s))
        tick("select")
        ngroups = int(torch.count_nonzero(sizes))
        label = torch.nonzero(sizes >= nmin).reshape(-1)
        length = sizes[label].to(torch.int64)
        rank = torch.argsort(((1 << 31) - length) * (1 << 31) + label)      # Length descending, then label ascending
        label, length = label[rank], length[rank]
        H = int(label.numel())
        slot = sizes.fill_(-1)                                                # the sizes are spent: reuse their memory
        slot[label] = torch.arange(H, dtype=torch.int32, device=dev)
        nv = 3 if vd is None else 6
        sums = torch.zeros((max(H, 1), nv), dtype=torch.int64, device=dev)
        labels = torch.empty(count, dtype=torch.int32, device=dev) if want_labels else None
        tick("catalog")
        _lib.check(l.nbe_fof_catalog(_ptr(X), _ptr(parent), _ptr(slot), _ptr(vd) if vd is not None else None,
                                     1 if vd is not None and vd.dtype == torch.float16 else 0, exps, count,
                                     int(bool(wave_reduce)), blocks, _ptr(sums), _ptr(labels) if want_labels else None, s))
        tick("finish")
        Xl = X[:, label].t().to(torch.int64).cpu().numpy()
        out = (label.cpu().numpy(), length.cpu().numpy(), Xl, sums[:H].cpu().numpy(),
               None if exps is None else np.array(list(exps), np.int64), ngroups, labels)
        tick(None)
    return out


def fof_halos(displacement, boxsize=1000.0, linking_length=0.2, nmin=20, absolute=False, velocity=None,
              return_labels=False, _max_blocks=None):
    """Friends-of-friends halos of the displaced lattice (reference scripts/halos.py:359-450: the positions, nbodykit's
    FOF(linking_length, nmin, absolute, periodic=True) and fof_catalog).  The module docstring has the definition.

    displacement: (3, n, n, n) float32 / float16, 2 <= n <= 1024, NumPy array or CUDA tensor (process_box's output).
    boxsize: L (scalar, or a 3-tuple of equal values).  linking_length: in units of the mean particle spacing L / n, or
    of the box with absolute=True; positive, below about L / 3 (the cell grid needs 3 cells per axis).  nmin >= 1.
    velocity: (3, n, n, n) float32 / float16 of the same kind and device.  `_max_blocks` caps the grid of every launch
    (tests): the results do not depend on it.

    Returns a dict: CMPosition (H, 3) float64, Length (H,) int64, label (H,) int64, with a velocity CMVelocity (H, 3)
    float64, with return_labels labels (n, n, n) int32 (the halo's row in the catalogue, or -1) -- NumPy arrays for a NumPy
    input, tensors on the input's device for a tensor --, ngroups (int, the groups of any size) and linking_length (float,
    the absolute length used).

    Raises ValueError, before any device work, for bad shapes or kinds, nmin < 1, a non-positive or too large linking
    length, n > 1024 and a mismatched velocity; ValueError for a non-finite displacement or velocity value or
    |psi_c / L| >= 2^20 (no partial catalogue is returned); NBEError when the device's free memory cannot take
    72 bytes per particle."""
    x, n, L, nmin, ell, R2, ncell, v, blocks = _validate(displacement, boxsize, linking_length, nmin, absolute, velocity,
                                                         _max_blocks)
    dev = _device_of(x)
    _check_free_memory(dev, BYTES_PER_PARTICLE * n ** 3, "fof_halos: %d particles" % n ** 3, "%d bytes each" % BYTES_PER_PARTICLE)
    dtypes = (torch.float32, torch.float16)
    xd = _to_device(x, dev, dtypes)
    vd = None if v is None else _to_device(v, dev, dtypes)
    label, length, Xl, sums, exps, ngroups, labels = _stages(xd, vd, n, L, nmin, R2, ncell, blocks, bool(return_labels))
    lf = length.astype(np.float64)[:, None]
    cm = np.mod(Xl + sums[:, :3].astype(np.float64) / lf, float(_U)) / float(_U) * L
    kind = (lambda a: torch.from_numpy(a).to(dev)) if _is_torch(x) else (lambda a: a)
    out = {"CMPosition": kind(cm), "Length": kind(length.astype(np.int64)), "label": kind(label.astype(np.int64))}
    if v is not None:
        out["CMVelocity"] = kind(np.ldexp(sums[:, 3:].astype(np.float64), (exps - 24)[None, :].astype(np.int32)) / lf)
    out["ngroups"] = ngroups
    out["linking_length"] = ell
    if return_labels:
        out["labels"] = _back(x, labels.reshape(n, n, n))
    return out


def particle_mass(Om, boxsize, n):
    """Mass of one particle of an n^3 load in M_sun / h: Om rho_crit L^3 / n^3 with rho_crit = 2.77536627e11 h^2 M_sun /
    Mpc^3 (reference scripts/halos.py:345-349)."""
    return float(Om) * RHO_CRIT * float(boxsize) ** 3 / float(n) ** 3


def halo_mass_function(npart, boxsize, particle_mass, log_edges, fof_correction=False):
    """Empirical dn / dlog10 M of a halo catalogue in Pylians' convention (reference scripts/halos.py:317-342), on the
    host in float64.  npart: particles per halo (fof_halos's Length); masses are particle_mass N, or
    particle_mass N (1 - N^-0.6) with fof_correction (Warren et al. 2006); they are histogrammed over 10**log_edges and
    the counts / (dM L^3) are multiplied by the geometric bin centres and ln 10.  NaN in every bin when there is no halo."""
    if _is_torch(npart):
        npart = npart.cpu().numpy()
    n_h = np.asarray(npart, dtype=np.float64).ravel()
    n_h = n_h[n_h > 0.0]
    log_edges = np.asarray(log_edges, dtype=np.float64)
    centres = 10.0 ** (0.5 * (log_edges[1:] + log_edges[:-1]))
    if n_h.size == 0:
        return np.full_like(centres, np.nan)
    masses = float(particle_mass) * (n_h * (1.0 - n_h ** (-0.6)) if fof_correction else n_h)
    edges = 10.0 ** log_edges
    counts, _ = np.histogram(masses, bins=edges)
    dndm = counts.astype(np.float64) / ((edges[1:] - edges[:-1]) * float(boxsize) ** 3)
    return dndm * centres * np.log(10.0)


def density_slab(delta, boxsize, axis, center, width):
    """Mean of a cubic density field over a slab normal to `axis` (reference scripts/halos.py:468-501,
    project_density_slab): the planes whose cell centres (j + 1/2) L / n lie within width / 2 of `center` in the periodic
    distance, or the nearest plane if none does.  delta: (n, n, n) NumPy array or torch tensor, read where it is.  axis: 0,
    1, 2 or 'x', 'y', 'z'.  Returns (map (n, n) float32 of the input's kind, number of planes)."""
    if not (_is_torch(delta) or isinstance(delta, np.ndarray)) or delta.ndim != 3 or len(set(delta.shape)) != 1:
        raise ValueError("density_slab needs a cubic (n, n, n) field, got %s"
                         % (tuple(delta.shape) if hasattr(delta, "shape") else type(delta).__name__,))
    axis = {"x": 0, "y": 1, "z": 2}.get(axis, axis)
    if isinstance(axis, (bool, np.bool_)) or axis not in (0, 1, 2):
        raise ValueError("density_slab: axis must be 0, 1, 2 or 'x', 'y', 'z', got %r" % (axis,))
    L = _real(boxsize, "boxsize", positive=True)
    n = int(delta.shape[0])
    dist = np.abs((np.arange(n, dtype=np.float64) + 0.5) * (L / n) - _real(center, "center"))
    dist = np.minimum(dist, L - dist)
    planes = np.nonzero(dist <= 0.5 * _real(width, "width"))[0]
    if planes.size == 0:
        planes = np.array([int(np.argmin(dist))])
    if _is_torch(delta):
        idx = torch.from_numpy(planes).to(delta.device)
        return delta.index_select(axis, idx).to(torch.float32).mean(dim=axis), int(planes.size)
    return np.take(delta, planes, axis=axis).astype(np.float32).mean(axis=axis).astype(np.float32), int(planes.size)


# ---- halo fields ----------------------------------------------------------------------------

_HALO_WEIGHTS = (None, "Length")


def _select_halos(cat, weight, min_length, max_length, redshift_space):
    """(rows mask or None for all, count) of a paint_halos call, validated."""
    if not isinstance(cat, dict) or "CMPosition" not in cat or "Length" not in cat:
        raise ValueError("paint_halos needs fof_halos's dict (CMPosition, Length), got %s" % type(cat).__name__)
    if weight not in _HALO_WEIGHTS:
        raise ValueError("paint_halos: weight must be None (number-weighted) or 'Length', got %r" % (weight,))
    if redshift_space and "CMVelocity" not in cat:
        raise ValueError("paint_halos: redshift_space needs a catalogue with CMVelocity (fof_halos(..., velocity=v))")
    for name, v in (("min_length", min_length), ("max_length", max_length)):
        if v is not None and (isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or not v == v):
            raise ValueError("paint_halos: %s must be a number or None, got %r" % (name, v))
    length = cat["Length"]
    keep = None
    if min_length is not None:
        keep = length >= min_length
    if max_length is not None:
        keep = (length <= max_length) if keep is None else keep & (length <= max_length)
    count = int(length.shape[0]) if keep is None else int(keep.sum())
    if count == 0:
        raise ValueError("paint_halos: no halo is left by the selection (%d in the catalogue, min_length %r, max_length %r)"
                         % (int(length.shape[0]), min_length, max_length))
    return keep, count


def paint_halos(cat, boxsize, res=512, worder=2, deconvolve=True, weight=None, min_length=None, max_length=None,
                redshift_space=False, los=2, velocity_to_length=None):
    """The density contrast of a halo catalogue (density.paint_particles of fof_halos's CMPosition; nbodykit's
    catalogue-to-mesh step on the reference's fof_catalog).

    cat: fof_halos's dict, NumPy arrays or CUDA tensors.  min_length, max_length: keep the halos with min_length <= Length
    <= max_length (None: no bound).  weight: None counts halos, "Length" weights each by its particle count (its mass).
    redshift_space: move every halo by velocity_to_length * CMVelocity[:, los] along array axis los first (rsd_factor(z,
    Om) for velocity_to_length; the catalogue needs fof_halos(..., velocity=v)).  boxsize, res, worder, deconvolve: as
    paint_particles.  Returns (delta_h, info): delta_h float32 of shape res in the catalogue's kind, info = {"count": the
    halos painted, "shot_noise": density.shot_noise of them (L^3 / count, or L^3 sum(w^2) / sum(w)^2 Length-weighted)}.
    A selection that leaves no halo raises ValueError."""
    from .density import paint_particles, shot_noise
    keep, count = _select_halos(cat, weight, min_length, max_length, redshift_space)
    rows = (lambda a: a) if keep is None else (lambda a: a[keep])
    pos, length = rows(cat["CMPosition"]), rows(cat["Length"])
    w = None
    if weight == "Length":
        w = length.to(torch.float64) if _is_torch(length) else np.asarray(length, dtype=np.float64)
    vel = rows(cat["CMVelocity"]) if redshift_space else None
    if redshift_space and velocity_to_length is None:
        raise ValueError("velocity_to_length is required with redshift_space (rsd_factor(z, Om))")
    delta = paint_particles(pos, boxsize=boxsize, res=res, worder=worder, deconvolve=deconvolve, weights=w, velocity=vel,
                            los=los, velocity_to_length=velocity_to_length if redshift_space else None)
    return delta, {"count": count, "shot_noise": shot_noise(boxsize, count=count, weights=w)}


def halo_bias(cat, delta_m, boxsize, **kwargs):
    """Halo auto spectrum, halo-matter cross spectrum, r(k) and bias: paint_halos(cat, boxsize, res=n, **kwargs) on the mesh
    of the (n, n, n) float32 matter field delta_m, then density.cross_correlation(delta_h, delta_m).  Returns that dict
    (a = halos, b = matter: bias = P_hm / P_mm) with shot_noise and count added.  Nothing is subtracted for the caller:
    p_aa still holds the shot noise."""
    from .density import cross_correlation
    if "res" in kwargs:
        raise ValueError("halo_bias takes the mesh size from delta_m")
    if not hasattr(delta_m, "shape") or len(delta_m.shape) != 3:
        raise ValueError("halo_bias needs a cubic (n, n, n) matter field")
    delta_h, info = paint_halos(cat, boxsize, res=int(delta_m.shape[0]), **kwargs)
    out = cross_correlation(delta_h, delta_m, boxsize=boxsize)
    out.update(shot_noise=info["shot_noise"], count=info["count"])
    return out


def halo_correlation(cat, boxsize, r_edges, matter=None, min_length=None, max_length=None, redshift_space=None, los=2,
                     velocity_to_length=None, nmu=None):
    """The two-point function of a halo catalogue by pair counts (correlation.correlation_function of fof_halos's
    CMPosition; Corrfunc's theory.DD / DDsmu, nbodykit's SimulationBox2PCF on the reference's fof_catalog): the auto
    function xi_hh, or with `matter` -- (count, 3) positions or a (3, n, n, n) displacement of the catalogue's kind -- the
    cross function xi_hm.

    cat, min_length, max_length, redshift_space, los, velocity_to_length: the halos and their selection as paint_halos (a
    true redshift_space moves every halo by velocity_to_length * CMVelocity[:, los] along array axis los first).  r_edges,
    nmu: as correlation.pair_counts; los is also the axis of the mu bins.  Returns correlation_function's dict (npairs, rr,
    xi, r_mid, ..., with nmu xi0, xi2, xi4) with count, the halos selected, added."""
    from .correlation import correlation_function
    keep, count = _select_halos(cat, None, min_length, max_length, redshift_space)
    pos = cat["CMPosition"] if keep is None else cat["CMPosition"][keep]
    if redshift_space:
        if velocity_to_length is None:
            raise ValueError("velocity_to_length is required with redshift_space (rsd_factor(z, Om))")
        los = _check_los(los)
        vel = cat["CMVelocity"] if keep is None else cat["CMVelocity"][keep]
        pos = pos.clone() if _is_torch(pos) else np.array(pos, dtype=np.float64)
        pos[:, los] += _real(velocity_to_length, "velocity_to_length") * vel[:, los]
    out = correlation_function(pos, boxsize, r_edges, b=matter, nmu=nmu, los=los)
    out["count"] = count
    return out


def halo_profiles(cat, matter, boxsize, r_edges, min_length=None, max_length=None, overdensity=None, reference="mean",
                  Om=None, z=0.0, particle_mass=None):
    """The matter profile around every halo of a catalogue and, with `overdensity`, its spherical-overdensity radius and
    mass (profiles.radial_counts on fof_halos's CMPosition; the profile and SO step of a halo finder such as Rockstar or
    AHF, which the reference does not have).

    cat, min_length, max_length: the halos and their selection as paint_halos.  matter: (count, 3) positions or the
    (3, n, n, n) displacement, of the catalogue's kind.  boxsize, r_edges: as profiles.radial_counts.  overdensity: None, or
    the Delta of profiles.spherical_overdensity with reference, Om, z and particle_mass (r_edges[0] must then be 0).
    Returns radial_counts's dict (counts (H, nb), r_edges, thresholds, ncell, count_a, count_b) with Length, the selected
    halos' lengths in the kind of the catalogue, and count, their number, added, and with overdensity R, N, M, flag and
    delta_eff (host float64 / int8, as spherical_overdensity returns them)."""
    from .profiles import radial_counts, spherical_overdensity
    keep, count = _select_halos(cat, None, min_length, max_length, False)
    if overdensity is not None and not float(np.asarray(r_edges, dtype=np.float64).ravel()[0]) == 0.0:
        raise ValueError("spherical_overdensity needs r_edges[0] == 0 (enclosed counts), got %g"
                         % float(np.asarray(r_edges, dtype=np.float64).ravel()[0]))
    if overdensity is not None and reference == "critical" and Om is None:
        raise ValueError("spherical_overdensity: reference='critical' needs Om")
    pos = cat["CMPosition"] if keep is None else cat["CMPosition"][keep]
    out = radial_counts(pos, matter, boxsize, r_edges)
    out["Length"] = cat["Length"] if keep is None else cat["Length"][keep]
    out["count"] = count
    if overdensity is not None:
        L = float(np.asarray(boxsize, dtype=np.float64).ravel()[0])
        out.update(spherical_overdensity(out["counts"], out["r_edges"], L, out["count_b"], overdensity=overdensity,
                                         reference=reference, Om=Om, z=z, particle_mass=particle_mass))
    return out


def halo_environment(cat, delta, boxsize, smoothing, threshold=0.0, worder=1, min_length=None):
    """Where in the cosmic web every halo of a catalogue sits: the eigenvalues of the tidal tensor of the smoothed matter
    field and the smoothed density contrast, read at the halo's centre of mass (web.cosmic_web's eigenvalue mesh through
    density.read_mesh; the environment that assembly-bias studies of a halo catalogue are cut on, which the reference
    does not have).

    cat, min_length: the halos and their selection as paint_halos.  delta: cubic (n, n, n) float32 matter density contrast
    of the catalogue's kind.  boxsize, smoothing (a length, or None), threshold (one number): as web.cosmic_web.  worder: the
    window of the readout; 1 (NGP) reads the voxel that holds the centre, so that web_type is that voxel's type exactly.
    Returns a dict in the catalogue's kind: eigenvalues (H, 3) float32, lambda_1 >= lambda_2 >= lambda_3 for worder = 1 (an
    interpolation of each sorted mesh otherwise); delta_s (H,) float32; web_type (H,) uint8, the number of read eigenvalues
    above the threshold in float32 comparison, 255 for a NaN; Length (H,), and count."""
    from . import web
    from .density import _check_worder, _read_mesh
    keep, count = _select_halos(cat, None, min_length, None, False)
    d, n, L, sigma, th, _, _, _ = web._validate_web(delta, boxsize, smoothing, threshold, "tidal", None, 1.0, None,
                                                    "halo_environment")
    if len(th) != 1:
        raise ValueError("halo_environment takes one threshold, got %d" % len(th))
    worder = _check_worder(worder)
    pos = cat["CMPosition"] if keep is None else cat["CMPosition"][keep]
    pos = _check_array(pos, "CMPosition")
    _same_kind(d, pos, "delta", "CMPosition")
    dev = _device_of(d)
    with torch.cuda.device(dev):
        eig, _, _, _, smooth = web._web(_to_device(d, dev, (torch.float32,)), n, L, sigma, th, None, 1.0, None,
                                        want_smooth=True)
        field = torch.cat([eig, smooth[None]])
        del eig, smooth
        pd = _to_device(pos, dev, (torch.float32, torch.float64))
        if pd.dtype not in (torch.float32, torch.float64):
            pd = pd.to(torch.float64)
        out, _ = _read_mesh(field, (n, n, n), (L, L, L), worder, float("nan"), p=pd.contiguous(), sort=False)
        e = out[:3]
        above = (e > float(th[0])).sum(0).to(torch.uint8)
        wt = torch.where(torch.isnan(e).any(0), torch.full_like(above, web.NO_TYPE), above)
    return {"eigenvalues": _back(d, out[:3].t().contiguous()), "delta_s": _back(d, out[3].contiguous()),
            "web_type": _back(d, wt), "Length": cat["Length"] if keep is None else cat["Length"][keep], "count": count}


def _select_moving_halos(cat, min_length, max_length, what):
    """_select_halos for a function that reads CMVelocity: (rows mask or None, count)."""
    if isinstance(cat, dict) and "CMPosition" in cat and "CMVelocity" not in cat:
        raise ValueError("%s needs a catalogue with CMVelocity (fof_halos(..., velocity=v))" % what)
    return _select_halos(cat, None, min_length, max_length, False)


def halo_velocity_profiles(cat, displacement, velocity, boxsize, r_edges, min_length=None, max_length=None):
    """The infall and velocity-dispersion profile of the matter about every halo of a catalogue
    (profiles.radial_velocity_moments with fof_halos's CMPosition and CMVelocity as the centres and their velocities; the
    velocity-profile step of a halo finder such as Rockstar or AHF, which the reference does not have).

    cat, min_length, max_length: the halos and their selection as paint_halos; the catalogue needs CMVelocity.
    displacement, velocity: the matter, (count, 3) positions with (count, 3) velocities or the (3, n, n, n) fields, of the
    catalogue's kind.  boxsize, r_edges: as profiles.radial_counts.  Returns radial_velocity_moments's dict (counts, sums,
    exponent, r_edges, thresholds, ncell, count_a, count_b) with v_r, sigma_r, sigma_t, vr2, vt2 (H, nb) of
    profiles.velocity_profile (host float64; v_r < 0 is infall), Length, the selected halos' lengths in the kind of the
    catalogue, and count, their number, added."""
    from .profiles import radial_velocity_moments, velocity_profile
    keep, count = _select_moving_halos(cat, min_length, max_length, "halo_velocity_profiles")
    rows = (lambda a: a) if keep is None else (lambda a: a[keep])
    out = radial_velocity_moments(rows(cat["CMPosition"]), rows(cat["CMVelocity"]), displacement, velocity, boxsize, r_edges)
    out.update(velocity_profile(out["counts"], out["sums"], out["exponent"]))
    out["Length"] = rows(cat["Length"])
    out["count"] = count
    return out


def halo_pairwise_velocity(cat, boxsize, r_edges, min_length=None, max_length=None):
    """The mean pairwise velocity v12(r) and the pairwise dispersions of a halo catalogue
    (correlation.pairwise_velocity of fof_halos's CMPosition and CMVelocity).  cat, min_length, max_length: the halos and
    their selection as paint_halos; the catalogue needs CMVelocity.  Returns pairwise_velocity's dict with count, the halos
    selected, added."""
    from .correlation import pairwise_velocity
    keep, count = _select_moving_halos(cat, min_length, max_length, "halo_pairwise_velocity")
    rows = (lambda a: a) if keep is None else (lambda a: a[keep])
    out = pairwise_velocity(rows(cat["CMPosition"]), rows(cat["CMVelocity"]), boxsize, r_edges)
    out["count"] = count
    return out


HALO_DELTA_FILE, HALO_PK_FILE, HALO_XI_FILE = "halo_delta.npy", "halo_pk.npz", "halo_xi.npz"
HALO_PROFILES_FILE = "halo_profiles.npz"
HALO_VPROFILES_FILE, HALO_V12_FILE = "halo_vprofiles.npz", "halo_v12.npz"
HALO_WEIGHT_NAMES = {"number": None, "length": "Length"}


def halo_spectra(cat, disp, boxsize, res, worder=2, weight=None):
    """The arrays of halo_delta.npy and halo_pk.npz for a catalogue and the displacement it was found in: the matter field
    is paint_density(disp, boxsize, res, worder), the halos are painted onto the same mesh with the same order.  Returns
    (delta_h as a NumPy array, dict with k, p_hh, p_mm, p_hm, r, bias, nmodes, shot_noise, count), or None for a
    catalogue without a halo."""
    from .density import cross_correlation, paint_density
    if int(cat["Length"].shape[0]) == 0:
        return None
    delta_m = paint_density(disp, boxsize=boxsize, res=res, worder=worder)
    delta_h, info = paint_halos(cat, boxsize, res=res, worder=worder, weight=weight)
    cc = cross_correlation(delta_h, delta_m, boxsize=boxsize)
    host = delta_h.cpu().numpy() if _is_torch(delta_h) else delta_h
    return host, dict(k=cc["k"], p_hh=cc["p_aa"], p_mm=cc["p_bb"], p_hm=cc["p_ab"], r=cc["r"], bias=cc["bias"],
                      nmodes=cc["nmodes"], shot_noise=np.float64(info["shot_noise"]), count=np.int64(info["count"]))


def xi_edges(rmin=1.0, rmax=50.0, nbins=20, log=False):
    """The nbins + 1 edges of --halo_xi: linear from rmin to rmax, or logarithmic with --xi_log (rmin > 0)."""
    if not (np.isfinite(rmin) and np.isfinite(rmax)) or rmin < 0.0 or not rmax > rmin or nbins < 1:
        raise ValueError("--halo_xi needs 0 <= xi_rmin < xi_rmax and xi_nbins >= 1, got %r, %r, %r" % (rmin, rmax, nbins))
    if log:
        if not rmin > 0.0:
            raise ValueError("--xi_log needs xi_rmin > 0, got %r" % (rmin,))
        return np.geomspace(rmin, rmax, nbins + 1)
    return np.linspace(rmin, rmax, nbins + 1)


def halo_xi_arrays(cat, boxsize, r_edges, nmu=None, los=2):
    """The arrays of halo_xi.npz: r_edges, r_mid, npairs, rr, xi, count, and with nmu mu_edges, xi0, xi2, xi4 -- or None
    for a catalogue without a halo."""
    if int(cat["Length"].shape[0]) == 0:
        return None
    out = halo_correlation(cat, boxsize, r_edges, nmu=nmu, los=los)
    to_np = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    names = ("r_edges", "r_mid", "npairs", "rr", "xi") + (("mu_edges", "xi0", "xi2", "xi4") if nmu is not None else ())
    arrs = {k: to_np(out[k]) for k in names}
    arrs["count"] = np.int64(out["count"])
    return arrs


def save_halo_xi(out_dir, arrs):
    """Write halo_xi.npz, or print the one line that says why not (halo_xi_arrays's None)."""
    if arrs is None:
        print("no halo in the catalogue: %s is not written" % HALO_XI_FILE)
        return
    np.savez(os.path.join(str(out_dir), HALO_XI_FILE), **arrs)


# ---- drivers -----------------------------------------------------------------------------------------------------------

CATALOG_FILE = "fof_catalog.npz"


def catalog_arrays(cat, n, boxsize, Om, linking_length, absolute, nmin):
    """The arrays of the reference's fof_catalog.npz (scripts/halos.py:871-881), same keys and dtypes, from fof_halos's
    dict.  LinkingLength and AbsoluteLinking are the command line's values, as there."""
    to_np = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    length = to_np(cat["Length"])
    return dict(CMPosition=to_np(cat["CMPosition"]).astype(np.float32).reshape(-1, 3),
                Npart=length.astype(np.int32),
                Mass=length.astype(np.float64) * particle_mass(Om, boxsize, n),
                BoxSize=np.array([boxsize] * 3, dtype=np.float64),
                NpartPerDim=np.int32(n),
                LinkingLength=np.float64(linking_length),
                AbsoluteLinking=np.bool_(absolute),
                Nmin=np.int32(nmin))


def build_parser():
    ap = argparse.ArgumentParser(description="Friends-of-friends halo catalogue of a saved displacement field, on the GPU.")
    ap.add_argument("--displacement_file", required=True, help="(3, N, N, N) or (N, N, N, 3) array (.npy)")
    ap.add_argument("--output_dir", required=True)
    ap.add_argument("--boxsize", type=float, default=1000.0, help="box size in Mpc/h (default: 1000.0)")
    ap.add_argument("--omega_m", "--omega-m", type=float, default=0.3175, dest="omega_m",
                    help="Omega_m of the particle mass (default: 0.3175)")
    ap.add_argument("--linking-length", type=float, default=0.2, dest="linking_length",
                    help="linking length in units of the mean particle spacing (unless --absolute-linking)")
    ap.add_argument("--absolute-linking", action=argparse.BooleanOptionalAction, default=False, dest="absolute_linking",
                    help="treat --linking-length as an absolute length in Mpc/h")
    ap.add_argument("--nmin", type=int, default=20, help="smallest particle count of a halo")
    ap.add_argument("--catalog-file", default=CATALOG_FILE, dest="catalog_file",
                    help="name of the catalogue inside --output_dir (default: %s)" % CATALOG_FILE)
    ap.add_argument("--halo_pk", type=int, default=None, metavar="RES",
                    help="also paint the halos and the matter onto a RES^3 mesh: %s and %s (k, p_hh, p_mm, p_hm, r, bias, "
                         "nmodes, shot_noise, count) inside --output_dir" % (HALO_DELTA_FILE, HALO_PK_FILE))
    ap.add_argument("--mas_worder", type=int, choices=(1, 2, 3, 4), default=2,
                    help="with --halo_pk or --halo_environment: 1 NGP, 2 CIC, 3 TSC, 4 PCS (default: 2)")
    ap.add_argument("--halo_weight", choices=sorted(HALO_WEIGHT_NAMES), default="number",
                    help="with --halo_pk: count halos, or weight each by its particle count (default: number)")
    add_xi_arguments(ap)
    add_profile_arguments(ap)
    ap.add_argument("--velocity_file", default=None,
                    help="the velocity of the same particles, (3, N, N, N) or (N, N, N, 3) (.npy): the catalogue's CMVelocity, "
                         "for --halo_vprofiles and --halo_v12")
    add_velocity_arguments(ap)
    add_environment_arguments(ap)
    return ap


def add_xi_arguments(ap, suppress=False):
    """The options of --halo_xi, shared with run_emulator (whose parser leaves an option that was not given out of the
    namespace: suppress)."""
    flag, value = (argparse.SUPPRESS, argparse.SUPPRESS) if suppress else (False, None)
    ap.add_argument("--halo_xi", action="store_true", default=flag,
                    help="also count the halo pairs: %s (r_edges, r_mid, npairs, rr, xi, count; with --xi_nmu also mu_edges, "
                         "xi0, xi2, xi4) inside the output directory" % HALO_XI_FILE)
    ap.add_argument("--xi_rmin", type=float, default=value, help="with --halo_xi: smallest edge in Mpc/h (default: 1)")
    ap.add_argument("--xi_rmax", type=float, default=value,
                    help="with --halo_xi: largest edge in Mpc/h, below boxsize / 3 (default: 50)")
    ap.add_argument("--xi_nbins", type=int, default=value, help="with --halo_xi: number of bins, 1 .. 128 (default: 20)")
    ap.add_argument("--xi_log", action="store_true", default=flag, help="with --halo_xi: logarithmic bins")
    ap.add_argument("--xi_nmu", type=int, default=value, metavar="N",
                    help="with --halo_xi: N uniform mu bins about axis 2 and the multipoles xi0, xi2, xi4")


def xi_options(args, boxsize, die):
    """The settings of --halo_xi of a parsed command line as a dict (r_edges, nmu), or None without it; `die(message)` for
    an option without --halo_xi and for edges or mu bins that pair_counts would refuse."""
    from .correlation import MAX_IMAGE, MAX_MU, pair_geometry
    given = [n for n in ("xi_rmin", "xi_rmax", "xi_nbins", "xi_nmu") if getattr(args, n, None) is not None]
    if getattr(args, "xi_log", False):
        given.append("xi_log")
    if not getattr(args, "halo_xi", False):
        if getattr(args, "halo_v12", False):                # --halo_v12 takes its edges from the same options
            given = [n for n in given if n == "xi_nmu"]
        if given:
            die("--%s needs --halo_xi" % given[0])
        return None
    get = lambda n, d: d if getattr(args, n, None) is None else getattr(args, n)
    nmu = getattr(args, "xi_nmu", None)
    try:
        edges = xi_edges(get("xi_rmin", 1.0), get("xi_rmax", 50.0), get("xi_nbins", 20), bool(getattr(args, "xi_log", False)))
        pair_geometry(boxsize, edges)
        if nmu is not None and (not 1 <= nmu <= MAX_MU or nmu * (len(edges) - 1) > MAX_IMAGE):
            raise ValueError("--xi_nmu must be in 1 .. %d with xi_nbins xi_nmu <= %d, got %d" % (MAX_MU, MAX_IMAGE, nmu))
    except ValueError as e:
        die(str(e))
    return dict(r_edges=edges, nmu=nmu)


SO_REFERENCES = ("mean", "critical")


def add_profile_arguments(ap, suppress=False):
    """The options of --halo_profiles, shared with run_emulator as add_xi_arguments's are."""
    flag, value = (argparse.SUPPRESS, argparse.SUPPRESS) if suppress else (False, None)
    ap.add_argument("--halo_profiles", action="store_true", default=flag,
                    help="also count the matter in shells about every halo: %s (r_edges, r_mid, counts, rho, Length, R_delta, "
                         "N_delta, M_delta, flag, overdensity, reference, count) inside the output directory"
                         % HALO_PROFILES_FILE)
    ap.add_argument("--profile_rmin", type=float, default=value,
                    help="with --halo_profiles: first edge after 0 in Mpc/h (default: 0.05)")
    ap.add_argument("--profile_rmax", type=float, default=value,
                    help="with --halo_profiles: largest edge in Mpc/h, below boxsize / 3 (default: 5)")
    ap.add_argument("--profile_nbins", type=int, default=value,
                    help="with --halo_profiles: edges from rmin to rmax, logarithmic, after the one at 0; 2 .. 128 (default: 20)")
    ap.add_argument("--so_overdensity", type=float, default=value,
                    help="with --halo_profiles: the spherical overdensity Delta of R_delta, N_delta, M_delta (default: 200)")
    ap.add_argument("--so_reference", choices=SO_REFERENCES, default=value,
                    help="with --halo_profiles: Delta times the mean matter density, or the critical density (default: mean)")


def profile_options(args, boxsize, die):
    """The settings of --halo_profiles of a parsed command line as a dict (r_edges, overdensity, reference), or None without
    it; `die(message)` for an option without --halo_profiles and for edges that radial_counts would refuse."""
    from .correlation import pair_geometry
    from .profiles import profile_edges
    names = ("profile_rmin", "profile_rmax", "profile_nbins", "so_overdensity", "so_reference")
    given = [n for n in names if getattr(args, n, None) is not None]
    if not getattr(args, "halo_profiles", False):
        if getattr(args, "halo_vprofiles", False):          # --halo_vprofiles takes its edges from the same options
            given = [n for n in given if n.startswith("so_")]
        if given:
            die("--%s needs --halo_profiles" % given[0])
        return None
    get = lambda n, d: d if getattr(args, n, None) is None else getattr(args, n)
    delta = get("so_overdensity", 200.0)
    try:
        edges = profile_edges(get("profile_rmin", 0.05), get("profile_rmax", 5.0), get("profile_nbins", 20))
        pair_geometry(boxsize, edges)
        if not (np.isfinite(delta) and delta > 0.0):
            raise ValueError("--so_overdensity must be positive, got %r" % (delta,))
    except ValueError as e:
        die(str(e))
    return dict(r_edges=edges, overdensity=float(delta), reference=get("so_reference", "mean"))


def halo_profile_arrays(cat, matter, boxsize, n, Om, r_edges, overdensity=200.0, reference="mean", z=0.0):
    """The arrays of halo_profiles.npz for a catalogue and the displacement it was found in (an n^3 load at redshift z,
    Omega_m Om): r_edges, r_mid, counts, rho, Length, R_delta, N_delta, M_delta, flag, overdensity, reference, count -- or None for
    a catalogue without a halo."""
    from .profiles import density_profile
    if int(cat["Length"].shape[0]) == 0:
        return None
    out = halo_profiles(cat, matter, boxsize, r_edges, overdensity=overdensity, reference=reference, Om=Om, z=z,
                        particle_mass=particle_mass(Om, boxsize, n))
    to_np = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    counts, edges = to_np(out["counts"]), to_np(out["r_edges"])
    prof = density_profile(counts, edges, boxsize, out["count_b"])
    return dict(r_edges=edges, r_mid=prof["r_mid"], counts=counts, rho=prof["rho"],
                Length=to_np(out["Length"]).astype(np.int64), R_delta=out["R"], N_delta=out["N"], M_delta=out["M"],
                flag=out["flag"], overdensity=np.float64(overdensity), reference=np.str_(reference),
                count=np.int64(out["count"]))


def save_halo_profiles(out_dir, arrs):
    """Write halo_profiles.npz, or print the one line that says why not (halo_profile_arrays's None)."""
    if arrs is None:
        print("no halo in the catalogue: %s is not written" % HALO_PROFILES_FILE)
        return
    np.savez(os.path.join(str(out_dir), HALO_PROFILES_FILE), **arrs)


def add_velocity_arguments(ap, suppress=False):
    """The options --halo_vprofiles and --halo_v12, shared with run_emulator as add_xi_arguments's are."""
    flag = argparse.SUPPRESS if suppress else False
    ap.add_argument("--halo_vprofiles", action="store_true", default=flag,
                    help="with a velocity: also the infall and dispersion profile of the matter about every halo, in the "
                         "shells of --profile_rmin / --profile_rmax / --profile_nbins: %s (r_edges, r_mid, counts, sums, exponent, "
                         "v_r, sigma_r, sigma_t, Length, count) inside the output directory" % HALO_VPROFILES_FILE)
    ap.add_argument("--halo_v12", action="store_true", default=flag,
                    help="with a velocity: also the mean pairwise velocity and the pairwise dispersions of the halos, in the "
                         "bins of --xi_rmin / --xi_rmax / --xi_nbins / --xi_log: %s (r_edges, r_mid, npairs, sums, exponent, v12, "
                         "sigma_r, sigma_t, count) inside the output directory" % HALO_V12_FILE)


def velocity_moment_options(args, boxsize, have_velocity, die, need="--velocity_file"):
    """The settings of --halo_vprofiles and --halo_v12 of a parsed command line as a dict (vprofiles: r_edges or None, v12:
    r_edges or None), or None without either; `die(message)` where the velocity they need (`need` names its option) is
    missing and for edges that pair_counts would refuse."""
    from .correlation import pair_geometry
    from .profiles import profile_edges
    vp, v12 = bool(getattr(args, "halo_vprofiles", False)), bool(getattr(args, "halo_v12", False))
    if not (vp or v12):
        return None
    if not have_velocity:
        die("--%s needs %s" % ("halo_vprofiles" if vp else "halo_v12", need))
    get = lambda n, d: d if getattr(args, n, None) is None else getattr(args, n)
    out = dict(vprofiles=None, v12=None)
    try:
        if vp:
            out["vprofiles"] = profile_edges(get("profile_rmin", 0.05), get("profile_rmax", 5.0), get("profile_nbins", 20))
            pair_geometry(boxsize, out["vprofiles"])
        if v12:
            out["v12"] = xi_edges(get("xi_rmin", 1.0), get("xi_rmax", 50.0), get("xi_nbins", 20), bool(getattr(args, "xi_log", False)))
            pair_geometry(boxsize, out["v12"])
    except ValueError as e:
        die(str(e))
    return out


def halo_vprofile_arrays(cat, matter, velocity, boxsize, r_edges):
    """The arrays of halo_vprofiles.npz for a catalogue with CMVelocity and the displacement and velocity it was found in:
    r_edges, r_mid, counts, sums, exponent, v_r, sigma_r, sigma_t, Length, count -- or None for a catalogue without a halo."""
    if int(cat["Length"].shape[0]) == 0:
        return None
    out = halo_velocity_profiles(cat, matter, velocity, boxsize, r_edges)
    to_np = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    edges = to_np(out["r_edges"])
    return dict(r_edges=edges, r_mid=0.5 * (edges[1:] + edges[:-1]), counts=to_np(out["counts"]), sums=to_np(out["sums"]),
                exponent=np.int64(out["exponent"]), v_r=out["v_r"], sigma_r=out["sigma_r"], sigma_t=out["sigma_t"],
                Length=to_np(out["Length"]).astype(np.int64), count=np.int64(out["count"]))


def halo_v12_arrays(cat, boxsize, r_edges):
    """The arrays of halo_v12.npz for a catalogue with CMVelocity: r_edges, r_mid, npairs, sums, exponent, v12, sigma_r,
    sigma_t, count -- or None for a catalogue without a halo."""
    if int(cat["Length"].shape[0]) == 0:
        return None
    out = halo_pairwise_velocity(cat, boxsize, r_edges)
    to_np = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    edges = to_np(out["r_edges"])
    arrs = {k: to_np(out[k]) for k in ("npairs", "sums", "v12", "sigma_r", "sigma_t")}
    arrs.update(r_edges=edges, r_mid=0.5 * (edges[1:] + edges[:-1]), exponent=np.int64(out["exponent"]),
                count=np.int64(out["count"]))
    return arrs


HALO_ENVIRONMENT_FILE = "halo_environment.npz"


def add_environment_arguments(ap, suppress=False, scan=False):
    """The options --halo_environment, --web_smoothing and --web_threshold, shared with run_emulator as add_xi_arguments's
    are; there --web_threshold takes several values for --cosmic_web (scan), of which --halo_environment reads the first."""
    value = argparse.SUPPRESS if suppress else None
    ap.add_argument("--halo_environment", type=int, default=value, metavar="RES",
                    help="also paint the matter onto a RES^3 mesh (--mas_worder) and read the tidal tensor's eigenvalues, the "
                         "smoothed density and the T-web type at every halo: %s (eigenvalues, delta_s, web_type, Length, count, "
                         "smoothing, threshold) inside the output directory" % HALO_ENVIRONMENT_FILE)
    ap.add_argument("--web_smoothing", type=float, default=value, metavar="R",
                    help="the Gaussian smoothing length of the web in Mpc/h (default: two cells of its mesh)")
    if scan:
        ap.add_argument("--web_threshold", type=float, nargs="+", default=value, metavar="T",
                        help="the eigenvalue threshold(s) of the web, up to 64 (default: 0)")
    else:
        ap.add_argument("--web_threshold", type=float, default=value, metavar="T",
                        help="the eigenvalue threshold of the web (default: 0)")


def web_settings(args, boxsize, res, die):
    """(smoothing, thresholds) of a parsed command line for a web on a res^3 mesh: --web_smoothing or two cells, and
    --web_threshold as a list (default [0.0]); `die(message)` for values web.cosmic_web would refuse."""
    smoothing = getattr(args, "web_smoothing", None)
    smoothing = 2.0 * boxsize / res if smoothing is None else float(smoothing)
    if not (smoothing > 0 and math.isfinite(smoothing)):
        die("--web_smoothing must be positive, got %r" % smoothing)
    th = getattr(args, "web_threshold", None)
    th = [0.0] if th is None else [float(v) for v in (th if isinstance(th, (list, tuple)) else [th])]
    if not 1 <= len(th) <= 64 or not all(math.isfinite(v) and abs(v) < 3.0e38 for v in th):
        die("--web_threshold takes 1 .. 64 finite values, got %r" % th)
    return smoothing, th


def environment_options(args, boxsize, die, worder=2):
    """The settings of --halo_environment as a dict (res, worder, smoothing, threshold), or None without it; `die(message)`
    for --web_smoothing / --web_threshold without a consumer (`args.cosmic_web` is run_emulator's other one)."""
    res = getattr(args, "halo_environment", None)
    if res is None:
        if not getattr(args, "cosmic_web", False):
            for name in ("web_smoothing", "web_threshold"):
                if getattr(args, name, None) is not None:
                    die("--%s needs --halo_environment%s" % (name, " or --cosmic_web" if hasattr(args, "ndiv") else ""))
        return None
    if not 2 <= res <= 2048:
        die("--halo_environment must be in 2 .. 2048, got %d" % res)
    smoothing, th = web_settings(args, boxsize, res, die)
    return dict(res=int(res), worder=int(worder), smoothing=smoothing, threshold=th[0])


def halo_environment_arrays(cat, disp, boxsize, env):
    """The arrays of halo_environment.npz for a catalogue and the displacement it was found in: the matter painted onto
    env's mesh (density.paint_density, deconvolved), halo_environment's eigenvalues, delta_s, web_type (NGP readout), Length
    and count, with smoothing and threshold -- or None for a catalogue without a halo."""
    if int(cat["Length"].shape[0]) == 0:
        return None
    from .density import paint_density
    delta = paint_density(disp, boxsize=boxsize, res=env["res"], worder=env["worder"], deconvolve=True)
    out = halo_environment(cat, delta, boxsize, env["smoothing"], threshold=env["threshold"], worder=1)
    to_np = lambda a: a.cpu().numpy() if _is_torch(a) else np.asarray(a)
    return dict(eigenvalues=to_np(out["eigenvalues"]), delta_s=to_np(out["delta_s"]), web_type=to_np(out["web_type"]),
                Length=to_np(out["Length"]).astype(np.int64), count=np.int64(out["count"]),
                smoothing=np.float64(env["smoothing"]), threshold=np.float32(env["threshold"]))


def save_halo_environment(out_dir, arrs):
    """Write halo_environment.npz, or print the one line that says why not (None for no halo)."""
    if arrs is None:
        print("no halo in the catalogue: %s is not written" % HALO_ENVIRONMENT_FILE)
        return
    np.savez(os.path.join(str(out_dir), HALO_ENVIRONMENT_FILE), **arrs)


def save_halo_velocity(out_dir, name, arrs):
    """Write halo_vprofiles.npz or halo_v12.npz (`name`), or print the one line that says why not (None for no halo)."""
    if arrs is None:
        print("no halo in the catalogue: %s is not written" % name)
        return
    np.savez(os.path.join(str(out_dir), name), **arrs)


def save_halo_spectra(out_dir, spectra):
    """Write halo_delta.npy and halo_pk.npz, or print the one line that says why not (halo_spectra's None)."""
    if spectra is None:
        print("no halo in the catalogue: %s and %s are not written" % (HALO_DELTA_FILE, HALO_PK_FILE))
        return
    np.save(os.path.join(str(out_dir), HALO_DELTA_FILE), spectra[0])
    np.savez(os.path.join(str(out_dir), HALO_PK_FILE), **spectra[1])


def load_displacement(path):
    """A (3, N, N, N) float32 / float16 array from a (3, N, N, N) or (N, N, N, 3) file (scripts/halos.py:372-379)."""
    disp = np.load(path, mmap_mode="r")
    if disp.ndim != 4:
        sys.exit("Displacement field must be 4D, got shape=%s." % (tuple(disp.shape),))
    if disp.shape[0] == 3:
        arr = np.asarray(disp)
    elif disp.shape[-1] == 3:
        arr = np.moveaxis(np.asarray(disp), -1, 0)
    else:
        sys.exit("Displacement shape must be (3,N,N,N) or (N,N,N,3), got %s." % (tuple(disp.shape),))
    return np.ascontiguousarray(arr, dtype=arr.dtype if arr.dtype in (np.float32, np.float16) else np.float32)


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.halo_pk is not None and a.halo_pk < 1:
        sys.exit("--halo_pk must be >= 1, got %d" % a.halo_pk)
    xi = xi_options(a, a.boxsize, sys.exit)
    prof = profile_options(a, a.boxsize, sys.exit)
    vmom = velocity_moment_options(a, a.boxsize, a.velocity_file is not None, sys.exit)
    if a.velocity_file is not None and vmom is None:
        sys.exit("--velocity_file needs --halo_vprofiles or --halo_v12")
    env = environment_options(a, a.boxsize, sys.exit, a.mas_worder)
    disp = load_displacement(a.displacement_file)
    vel = None
    if vmom is not None:
        vel = load_displacement(a.velocity_file)
        if vel.shape != disp.shape:
            sys.exit("--velocity_file has shape %s, the displacement %s." % (tuple(vel.shape), tuple(disp.shape)))
    try:
        cat = fof_halos(disp, boxsize=a.boxsize, linking_length=a.linking_length, nmin=a.nmin, absolute=a.absolute_linking,
                        velocity=vel)
    except ValueError as e:
        sys.exit(str(e))
    os.makedirs(a.output_dir, exist_ok=True)
    path = os.path.join(a.output_dir, a.catalog_file)
    np.savez_compressed(path, **catalog_arrays(cat, disp.shape[1], a.boxsize, a.omega_m, a.linking_length,
                                               a.absolute_linking, a.nmin))
    print("%d halos of %d groups (linking length %g) -> %s" % (len(cat["Length"]), cat["ngroups"], cat["linking_length"],
                                                               path))
    if a.halo_pk is not None:
        save_halo_spectra(a.output_dir, halo_spectra(cat, disp, a.boxsize, a.halo_pk, a.mas_worder,
                                                     HALO_WEIGHT_NAMES[a.halo_weight]))
    if xi is not None:
        save_halo_xi(a.output_dir, halo_xi_arrays(cat, a.boxsize, xi["r_edges"], xi["nmu"]))
    if prof is not None:
        save_halo_profiles(a.output_dir, halo_profile_arrays(cat, disp, a.boxsize, disp.shape[1], a.omega_m, prof["r_edges"],
                                                             prof["overdensity"], prof["reference"]))
    if vmom is not None and vmom["vprofiles"] is not None:
        save_halo_velocity(a.output_dir, HALO_VPROFILES_FILE, halo_vprofile_arrays(cat, disp, vel, a.boxsize, vmom["vprofiles"]))
    if vmom is not None and vmom["v12"] is not None:
        save_halo_velocity(a.output_dir, HALO_V12_FILE, halo_v12_arrays(cat, a.boxsize, vmom["v12"]))
    if env is not None:
        save_halo_environment(a.output_dir, halo_environment_arrays(cat, disp, a.boxsize, env))


if __name__ == "__main__":
    main()
