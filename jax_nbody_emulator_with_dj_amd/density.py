"""Density fields from emulated displacements, on the GPU: mass assignment, MAS deconvolution, power spectra.

The fork's pipeline turns `process_box`'s displacement into a density field right away (reference
`scripts/core.py:447-458`: `dj.get_delta_from_psi(psi_emu, method="pm", res, worder, deconvolve)`), deconvolves the
assignment window (`scripts/utils.py:136-148`) and measures P(k) (`scripts/utils.py:1083-1085`, Pylians `Pk_library.Pk`).

    from jax_nbody_emulator_with_dj_amd.density import paint_density, deconvolve_mas, power_spectrum

    delta = paint_density(displacement, boxsize=1000.0, res=512, worder=2, deconvolve=True)
    k, pk, nmodes = power_spectrum(delta, boxsize=1000.0)
    k, pk, nmodes = power_spectrum(delta_emu, boxsize=1000.0, other=delta_lpt)     # cross spectrum Re<a b*>
    mp = power_spectrum_multipoles(delta_s, boxsize=1000.0, los=2)          # k, p0, p2, p4, nmodes
    wd = power_spectrum_wedges(delta_s, boxsize=1000.0, los=2, nmu=5)       # k, mu, pk, nmodes (nmu, n // 2), mu_edges
    delta_c = deconvolve_mas(delta, worder=2)
    vmesh = paint_field(displacement, velocity, boxsize=1000.0, res=512)     # mass-weighted mean velocity, (3, res...)
    delta_s = paint_density(displacement, res=512, velocity=velocity, los=2, velocity_to_length=rsd_factor(z, Om))
    mf = minkowski_functionals(delta, boxsize=1000.0)    # v0 .. v3 at 41 thresholds of the standardized field
    delta_h = paint_particles(positions, boxsize=1000.0, res=512)           # a catalogue: halos, a subsample, a snapshot
    cc = cross_correlation(delta_h, delta, boxsize=1000.0)                  # k, p_aa, p_bb, p_ab, r, transfer, bias, nmodes
    bk = bispectrum(delta, boxsize=1000.0, k1=0.1, k2=0.1, theta=np.linspace(0, np.pi, 25))    # B, Q, ntriangles, ...
    st = field_statistics(delta)                         # mean, std, skewness, kurtosis_excess
    pdf = field_pdf(delta, lo=-1.0, hi=8.0, nbins=120)   # np.histogram's counts and density

Conventions (as DISCO-DJ / Pylians and the lattice of `scripts/halos.py:394-403`):

- `displacement` is (3, N0, N1, N2) in the units of the box (Mpc/h); channel c moves along array axis c.  Particle
  (i0, i1, i2) has mass 1 and sits at q_c + psi_c with the lattice q_c = i_c L_c / N_c, periodically wrapped (any
  number of boxes, negative values included).
- Mesh node j of axis c sits at j L_c / res_c; an undisplaced lattice with res == N paints delta = 0 for every order.
- `worder` 1 = NGP, 2 = CIC, 3 = TSC, 4 = PCS: the one-dimensional windows are the B-splines of that order in units of
  the mesh spacing.  The result is delta = rho / rho_mean - 1 in float32, rho_mean = N0 N1 N2 / (res0 res1 res2).
- Masses are summed in fixed point (units of 2^-22 particle masses, 64-bit integers): the painted field is bitwise
  reproducible, each particle adds exactly its unit mass, and every cell is within 2^-22 per contributing particle of the
  exact float64 sum before the conversion to float32.
- `paint_field` (reference `scripts/utils.py:151-183`, project_field_from_particles) assigns a per-particle quantity with
  the same weights: every value is carried as an integer of 25 bits relative to its channel's largest magnitude and the
  sums are 64-bit integers, so the fields are bitwise reproducible too (its docstring has the arithmetic).  `velocity`,
  `los` and `velocity_to_length` move the particles along one axis first: redshift space for
  velocity_to_length = `rsd_factor(z, Om)`.
- `paint_particles` (nbodykit's catalogue-to-mesh step) paints explicit positions, (count, 3) float32 / float64, with the
  same integers: position x_c sits at mesh coordinate x_c res_c / L_c in float64, wrapped like a lattice particle.  The
  result does not depend on the order of the rows nor on `sort`.
- Deconvolution divides the rfft of the mesh by prod_c sinc(k_c L_c / (2 res_c))^worder, sinc(x) = sin(x) / x (the
  window alone, no alias sum).
- `power_spectrum` uses the unnormalised forward FFT: P = |delta_k|^2 L^3 / n^6.  Shell b = 1 .. n/2 holds the modes
  with b - 1/2 <= |k| / k_F < b + 1/2, k_F = 2 pi / L, counted over the full complex grid; it returns the mean |k|, the
  mean P and the number of modes per shell as float64 NumPy arrays.  `power_spectrum_multipoles` and
  `power_spectrum_wedges` split the same shells by mu = k_los / |k| about an array axis.
- `minkowski_functionals` (reference `scripts/utils.py:652-763`) counts the elements of the periodic cubical complex of
  each excursion set {w >= t} in one pass over the field: see its docstring for the definition.
- `bispectrum` (reference `scripts/utils.py:1314-1399`, Pylians `Bk`) is the FFT estimator of B(k1, k2, theta) and of the
  reduced Q(theta); `field_statistics` and `field_pdf` (`scripts/utils.py:1164-1187`, `:1248-1274`) are the one-point
  moments and histogram.  Their docstrings hold the definitions; all three return small host objects.

Residency: NumPy in gives NumPy out; a CUDA torch tensor in gives a CUDA tensor on the same device, with no host copy,
enqueued on torch's current stream of that device.  float16 displacements are read as half in the kernel.  There is no CPU
fallback: without a device the first device call raises NBEError.  Arguments are validated before any device work.
"""

import ctypes as C
import numbers

import numpy as np

from . import _lib
from ._lib import NBEError

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["paint_density", "deconvolve_mas", "power_spectrum", "minkowski_functionals", "bispectrum",
           "field_statistics", "field_pdf", "paint_field", "rsd_factor", "power_spectrum_multipoles",
           "power_spectrum_wedges", "paint_particles", "cross_correlation", "shot_noise", "read_mesh"]

WORDERS = {1: "NGP", 2: "CIC", 3: "TSC", 4: "PCS"}
_UNIT = 2.0 ** 22           # fixed-point units per particle mass (include/nbe.h, nbe_paint_mesh)
_KEXP = 36                  # the |k| sums of nbe_power_spectrum are in units of 2^-36, and the |mu| sums of nbe_power_wedges
_PK_ANISO_MAX_N = 2048      # include/nbe.h: NBE_PK_ANISO_MAX_N, NBE_PK_MAX_MU
_PK_MAX_MU = 64
_MF_MAX_N = 2048            # include/nbe.h: NBE_MF_MAX_N, NBE_MF_MAX_THRESHOLDS, NBE_MOMENTS_WORDS
_MF_MAX_T = 1024
_MOMENT_WORDS = 2050
MF_CONVENTION = "periodic_voxel_cubical_complex"
_BK_MIN_N, _BK_MAX_N = 4, 2048   # include/nbe.h: NBE_BK_MIN_N, NBE_BK_MAX_N, NBE_BK_MAX_SHELLS - 2, NBE_BK_PARTIALS
_BK_MAX_T = 256
_BK_PARTIALS = 2048
_MOMENT4_WORDS = 6148           # include/nbe.h: NBE_MOMENTS4_WORDS, NBE_PDF_MAX_BINS, NBE_ONEPOINT_MAX_VOXELS
_PDF_MAX_BINS = 4096
_ONEPOINT_MAX = 1 << 40
_MAX_CHANNELS = 4               # include/nbe.h: NBE_PAINT_MAX_CHANNELS, NBE_FIELD_DENSITY, NBE_FIELD_MEAN
_NORMALIZE = {"density": 0, "mean": 1}


def _is_torch(x):
    return torch is not None and isinstance(x, torch.Tensor)


def _triple(v, name, kind):
    if isinstance(v, (tuple, list, np.ndarray)):
        vals = list(np.asarray(v).ravel())
        if len(vals) != 3:
            raise ValueError("%s must be a scalar or a 3-tuple, got %r" % (name, v))
    else:
        vals = [v] * 3
    out = []
    for x in vals:
        if isinstance(x, (bool, np.bool_)):
            raise ValueError("%s must be %s, got %r" % (name, kind, v))
        if kind == "an int":
            if not isinstance(x, numbers.Integral):
                raise ValueError("%s must be an int or a 3-tuple of ints, got %r" % (name, v))
            if int(x) < 1:
                raise ValueError("%s must be >= 1, got %r" % (name, v))
            out.append(int(x))
        else:
            if not isinstance(x, numbers.Real) or not np.isfinite(float(x)) or float(x) <= 0:
                raise ValueError("%s must be positive and finite, got %r" % (name, v))
            out.append(float(x))
    return tuple(out)


def _check_worder(worder):
    if isinstance(worder, (bool, np.bool_)) or not isinstance(worder, numbers.Integral) or int(worder) not in WORDERS:
        raise ValueError("worder must be 1 (NGP), 2 (CIC), 3 (TSC) or 4 (PCS), got %r" % (worder,))
    return int(worder)


def _real(v, name, positive=False):
    """v as a float: a finite (with `positive`, positive) real number that is not a bool."""
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Real) or not np.isfinite(float(v)) or \
            (positive and float(v) <= 0):
        raise ValueError("%s must be a %sfinite number, got %r" % (name, "positive " if positive else "", v))
    return float(v)


def _dtype_name(x):
    return str(x.dtype).replace("torch.", "")


def _check_array(x, name):
    if _is_torch(x):
        if not x.is_cuda:
            raise ValueError("%s: a torch tensor must live on a CUDA (HIP) device; pass a NumPy array for host data" % name)
        return x
    if isinstance(x, np.ndarray):
        return x
    raise ValueError("%s must be a NumPy array or a CUDA torch tensor, got %s" % (name, type(x).__name__))


def _cubic(x, name, boxsize, what, noun, lo, hi):
    """A cubic float32 mesh of size lo .. hi in a cubic box, for the public function `what` (which calls it a `noun`):
    (array, n, L)."""
    x = _check_array(x, name)
    if x.ndim != 3 or len(set(x.shape)) != 1:
        raise ValueError("%s needs a cubic %s, got shape %s" % (what, noun, tuple(x.shape)))
    n = int(x.shape[0])
    if not lo <= n <= hi:
        raise ValueError("%s: mesh size %d unsupported (%d .. %d)" % (what, n, lo, hi))
    if _dtype_name(x) != "float32":
        raise ValueError("%s must be float32, got %s" % (name, _dtype_name(x)))
    L = _triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("%s needs a cubic box, got boxsize %s" % (what, L))
    return x, n, L[0]


def _device():
    """The device for host (NumPy) inputs: cuda:<current>.  Raises NBEError when none is visible (no CPU fallback)."""
    if torch is None or not torch.cuda.is_available():
        raise NBEError("density: no HIP device is visible; this library has no CPU fallback")
    _lib.lib()
    return torch.device("cuda", torch.cuda.current_device())


def _device_of(x):
    """Where a public call works: the device of a tensor input, `_device()` for a NumPy input."""
    return x.device if _is_torch(x) else _device()


def _back(x, t):
    """The result tensor t (or None) in the kind of the input x: NumPy for a NumPy input, t itself for a tensor."""
    return t if t is None or _is_torch(x) else t.cpu().numpy()


def _stream(dev):
    return C.c_void_p(int(torch.cuda.current_stream(dev).cuda_stream) or None)


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _i64(v):
    return (C.c_int64 * 3)(*[int(x) for x in v])


def _to_device(x, dev, dtypes):
    if _is_torch(x):
        return x.contiguous()
    t = torch.from_numpy(np.ascontiguousarray(x))
    return t.to(dev) if t.dtype in dtypes else t.to(device=dev, dtype=torch.float32)


def _validate_paint(displacement, boxsize, res, worder):
    x = _check_array(displacement, "displacement")
    if x.ndim != 4 or x.shape[0] != 3 or min(x.shape) < 1:
        raise ValueError("displacement must have shape (3, N0, N1, N2), got %s" % (tuple(x.shape),))
    if _dtype_name(x) not in ("float32", "float16"):
        raise ValueError("displacement must be float32 or float16, got %s" % _dtype_name(x))
    return x, _triple(boxsize, "boxsize", "a length"), _triple(res, "res", "an int"), _check_worder(worder)


def _paint(x, boxsize, res, worder, deconvolve, count_atomics=False):
    """Device work of paint_density: x is a contiguous CUDA tensor.  Returns (delta tensor, stats tensor): stats[0] tiles
    on the direct path, stats[1] particles not painted, stats[2:4] (int64) mesh atomics when count_atomics is set."""
    l = _lib.lib()
    dev = x.device
    with torch.cuda.device(dev):
        s = _stream(dev)
        mesh = torch.zeros(res, dtype=torch.int64, device=dev)
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        half = x.dtype == torch.float16
        n = tuple(int(v) for v in x.shape[1:])
        _lib.check(l.nbe_paint_mesh(_ptr(x), 1 if half else 0, _i64(n), (C.c_double * 3)(*boxsize), _i64(res),
                                    worder, int(bool(count_atomics)), _ptr(mesh), _ptr(stats), s))
        delta = torch.empty(res, dtype=torch.float32, device=dev)
        _lib.check(l.nbe_mesh_to_delta(_ptr(mesh), _i64(res), n[0] * n[1] * n[2], _ptr(delta), s))
        del mesh
        if deconvolve:
            delta = _deconvolve(delta, worder)
    return delta, stats


def _deconvolve(delta, worder):
    res = tuple(int(v) for v in delta.shape)
    fk = torch.fft.rfftn(delta).contiguous()         # the kernels index the half spectrum row-major
    _lib.check(_lib.lib().nbe_deconvolve_mas(_ptr(fk), _i64(res), worder, _stream(delta.device)))
    return torch.fft.irfftn(fk, s=res).contiguous()


def _check_los(los):
    if isinstance(los, (bool, np.bool_)) or not isinstance(los, numbers.Integral) or int(los) not in (0, 1, 2):
        raise ValueError("los must be the array axis 0, 1 or 2, got %r" % (los,))
    return int(los)


def _validate_shift(velocity, los, velocity_to_length, n, kind_of, what):
    """The line-of-sight arguments: (velocity array or None, los, velocity_to_length as a float or None)."""
    los = _check_los(los)
    if velocity is None:
        return None, los, None
    v = _check_array(velocity, "velocity")
    if tuple(v.shape) not in ((3,) + tuple(n), tuple(n)):
        raise ValueError("velocity must have shape %s or %s, got %s" % ((3,) + tuple(n), tuple(n), tuple(v.shape)))
    if _dtype_name(v) not in ("float32", "float16"):
        raise ValueError("velocity must be float32 or float16, got %s" % _dtype_name(v))
    _same_kind(kind_of, v, what, "velocity")
    if velocity_to_length is None:
        raise ValueError("velocity_to_length is required with a velocity (rsd_factor(z, Om) for redshift space)")
    return v, los, _real(velocity_to_length, "velocity_to_length")


def _same_kind(a, b, name_a, name_b):
    if _is_torch(a) != _is_torch(b) or (_is_torch(a) and a.device != b.device):
        raise ValueError("%s and %s must both be NumPy arrays or both tensors on one device" % (name_a, name_b))


def _check_max_blocks(max_blocks, who):
    """The cap on the grid of every launch as the C side takes it: 0 for None, else the int >= 1."""
    if max_blocks is None:
        return 0
    if isinstance(max_blocks, (bool, np.bool_)) or not isinstance(max_blocks, numbers.Integral) or int(max_blocks) < 1:
        raise ValueError("%s: _max_blocks must be an int >= 1, got %r" % (who, max_blocks))
    return int(max_blocks)


def _free_memory(dev):
    free, _ = torch.cuda.mem_get_info(dev)
    return free + torch.cuda.memory_reserved(dev) - torch.cuda.memory_allocated(dev)     # cached blocks are reusable


def _check_free_memory(dev, need, what, detail):
    """NBEError "<what> need about .. GB of device memory (<detail>), .. GB are free" where `need` bytes are not free."""
    free = _free_memory(dev)
    if need > free:
        raise NBEError("%s need about %.1f GB of device memory (%s), %.1f GB are free" % (what, need / 1e9, detail, free / 1e9))


def _validate_field(displacement, quantity, boxsize, res, worder, normalize, fill, velocity, los, velocity_to_length):
    q = _check_array(quantity, "quantity")
    if q.ndim not in (3, 4) or min(q.shape) < 1 or (q.ndim == 4 and q.shape[0] > _MAX_CHANNELS):
        raise ValueError("quantity must have shape (N0, N1, N2) or (C, N0, N1, N2) with 1 <= C <= %d, got %s"
                         % (_MAX_CHANNELS, tuple(q.shape)))
    if _dtype_name(q) not in ("float32", "float16"):
        raise ValueError("quantity must be float32 or float16, got %s" % _dtype_name(q))
    n = tuple(int(v) for v in q.shape[-3:])
    if displacement is None:
        x, boxsize, res, worder = None, _triple(boxsize, "boxsize", "a length"), _triple(res, "res", "an int"), \
            _check_worder(worder)
    else:
        x, boxsize, res, worder = _validate_paint(displacement, boxsize, res, worder)
        if tuple(x.shape[1:]) != n:
            raise ValueError("quantity must have the lattice shape %s of the displacement, got %s"
                             % (tuple(x.shape[1:]), tuple(q.shape)))
        _same_kind(x, q, "displacement", "quantity")
    if normalize not in _NORMALIZE:
        raise ValueError("normalize must be 'density' or 'mean', got %r" % (normalize,))
    _real(fill, "fill")
    v, los, f = _validate_shift(velocity, los, velocity_to_length, n, q, "quantity")
    return x, q, v, los, f, n, boxsize, res, worder


def _paint_fields(x, q, v, los, scale, n, boxsize, res, worder, normalize="density", fill=0.0, want_delta=False):
    """Device work of paint_field and of paint_density with a velocity.  x: contiguous CUDA (3,) + n tensor or None (the
    lattice); q: contiguous (C,) + n tensor or None (masses only); v: contiguous n tensor (the line-of-sight component) or
    None.  Returns (field (C,) + res or None, delta or None, stats): stats[0] tiles on the direct path, stats[1]
    particles not painted, stats[2] cells at the overflow limit.  Raises NBEError for a non-finite quantity."""
    l = _lib.lib()
    dev = (q if q is not None else x).device
    half = lambda t: 1 if t is not None and t.dtype == torch.float16 else 0
    nchan = 0 if q is None else int(q.shape[0])
    count = n[0] * n[1] * n[2]
    with torch.cuda.device(dev):
        s = _stream(dev)
        exps = (C.c_int * _MAX_CHANNELS)()
        if nchan:
            rng = torch.zeros(nchan + 1, dtype=torch.int32, device=dev)
            _lib.check(l.nbe_quantity_range(_ptr(q), half(q), nchan, count, _ptr(rng), s))
            r = rng.cpu().numpy()
            if int(r[nchan]):
                raise NBEError("paint_field: %d value(s) of the quantity are not finite" % int(r[nchan].view(np.uint32)))
            amax = r[:nchan].view(np.float32).astype(np.float64)
            for c, e in enumerate(np.frexp(amax)[1]):             # A_c = m 2^e, m in [0.5, 1): A_c < 2^e; 0 for A_c = 0
                exps[c] = int(e)
        mesh = torch.zeros(res, dtype=torch.int64, device=dev)
        qmesh = torch.zeros((nchan,) + tuple(res), dtype=torch.int64, device=dev) if nchan else None
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(l.nbe_paint_fields(_ptr(x) if x is not None else None, half(x), _ptr(q) if nchan else None, half(q),
                                      nchan, exps, _ptr(v) if v is not None else None, half(v), los,
                                      float(scale) if v is not None else 0.0, _i64(n), (C.c_double * 3)(*boxsize),
                                      _i64(res), worder, _ptr(mesh), _ptr(qmesh) if nchan else None, _ptr(stats), s))
        field = delta = None
        if nchan:
            field = torch.empty((nchan,) + tuple(res), dtype=torch.float32, device=dev)
            _lib.check(l.nbe_mesh_to_field(_ptr(mesh), _ptr(qmesh), nchan, exps, _i64(res), count, _NORMALIZE[normalize],
                                           float(fill), _ptr(field), _ptr(stats), s))
        if want_delta:
            delta = torch.empty(res, dtype=torch.float32, device=dev)
            _lib.check(l.nbe_mesh_to_delta(_ptr(mesh), _i64(res), count, _ptr(delta), s))
    return field, delta, stats


def _los_component(v, los, n):
    """The contiguous (N0, N1, N2) line-of-sight component of a device velocity."""
    return (v[los] if v.ndim == 4 else v).contiguous()


def _check_stats(stats, what, overflow):
    st = stats.cpu().tolist()
    if st[1]:
        raise NBEError("%s: %d particle(s) have a non-finite or out-of-range position" % (what, st[1]))
    if overflow and st[2]:
        raise NBEError("%s: %d cell(s) hold 2^17 particle masses or more (2^39 mass units), beyond which the 64-bit "
                       "sums of a quantity can overflow" % (what, st[2]))


def paint_density(displacement, boxsize=1000.0, res=512, worder=2, deconvolve=True, velocity=None, los=2,
                  velocity_to_length=None):
    """Mass assignment of the displaced lattice onto a periodic mesh (reference scripts/core.py:449,
    dj.get_delta_from_psi(psi, method="pm", res, worder, deconvolve)).

    displacement: (3, N0, N1, N2) float32 / float16, NumPy array or CUDA torch tensor (process_box's output).
    boxsize: L (scalar or 3-tuple, units of the displacement).  res: mesh size (int or 3-tuple; any value >= 1).
    worder: 1 NGP, 2 CIC, 3 TSC, 4 PCS.  deconvolve: divide by the assignment window (deconvolve_mas).
    velocity, los, velocity_to_length: with a velocity ((3, N0, N1, N2), of which component `los` is read, or
    (N0, N1, N2); float32 / float16, same kind and device as the displacement) every particle is moved by
    velocity_to_length * v along array axis los (0, 1 or 2) before it is painted: the plane-parallel redshift-space
    density for velocity_to_length = rsd_factor(z, Om).  The position along los is i a + psi s + v vs in float64 (mesh
    units; vs = velocity_to_length res / L).  Without a velocity the call is what it was before these arguments existed.
    Returns delta = rho / rho_mean - 1, float32, shape res; NumPy for NumPy input, a CUDA tensor on the input's device
    for tensor input.  Raises NBEError if a displacement or velocity is not finite (those particles could not be painted).
    See the module docstring for the conventions."""
    x, boxsize, res, worder = _validate_paint(displacement, boxsize, res, worder)
    n = tuple(int(d) for d in x.shape[1:])
    v, los, f = _validate_shift(velocity, los, velocity_to_length, n, x, "displacement")
    dev = _device_of(x)
    dtypes = (torch.float32, torch.float16)
    xd = _to_device(x, dev, dtypes)
    if v is None:
        delta, stats = _paint(xd, boxsize, res, worder, bool(deconvolve))
        _check_stats(stats, "paint_density", False)
        return _back(x, delta)
    vd = _los_component(_to_device(v, dev, dtypes), los, n)
    _, delta, stats = _paint_fields(xd, None, vd, los, f, n, boxsize, res, worder, want_delta=True)
    _check_stats(stats, "paint_density", False)
    if deconvolve:
        with torch.cuda.device(dev):
            delta = _deconvolve(delta, worder)
    return _back(x, delta)


def paint_field(displacement, quantity, boxsize=1000.0, res=512, worder=2, normalize="density", deconvolve=False,
                fill=0.0, return_delta=False, velocity=None, los=2, velocity_to_length=None):
    """Assign a per-particle quantity to a periodic mesh with the weights of paint_density (reference
    scripts/utils.py:151-183, project_field_from_particles: DISCO-DJ compute_field_quantity_from_particles(pos, quantity,
    method="pm", res, worder, deconvolve, normalize_by_density=True); scripts/halos.py:468, project_density_slab).

    displacement: as paint_density, or None for the undisplaced lattice (the reference's use: a field of the particle grid
    carried to another mesh); the lattice shape then comes from `quantity`.
    quantity: (N0, N1, N2) or (C, N0, N1, N2), 1 <= C <= 4, float32 / float16, same kind (NumPy or tensor) and device as
    the displacement.  process_box's velocity is a valid quantity as it stands.
    normalize: "density" gives sum(w q) / sum(w) per cell, the mass-weighted mean (normalize_by_density=True), and `fill`
    in cells without mass.  "mean" gives sum(w q) / (N_p / n_cells), the momentum-like field (1 + delta) q.
    deconvolve: divide every channel of the finished field by the assignment window (deconvolve_mas).  DISCO-DJ is not
    available where this library is developed, so whether it deconvolves the numerator and the density separately before
    it divides them under normalize_by_density cannot be pinned; here the window is divided out of the ratio.
    return_delta: also return the density contrast of the same pass, bit for bit paint_density(..., deconvolve=False).
    velocity, los, velocity_to_length: the line-of-sight shift of paint_density.
    Returns the field, float32, shape res or (C,) + res (and delta with return_delta): NumPy for NumPy input, CUDA tensors
    on the input's device for tensor input, on torch's current stream.

    Arithmetic.  The mass of a cell is paint_density's integer M (2^-22 particle masses).  For channel c let A_c = max |q_c|
    and e_c the binary exponent with A_c < 2^e_c.  Particle p carries V_p = rint(q_p 2^(24 - e_c)), |V_p| <= 2^24: a
    float32 value in the channel's top binade is exact, smaller ones are rounded at 2^(e_c - 25).  The cell holds S = sum
    of w V_p in a 64-bit integer, w the integer weights of the mass.  In float64, rounded once to float32: "mean" is
    S 2^(e_c - 46) n_cells / N_p, "density" is S 2^(e_c - 24) / M.  Before that rounding the numerator of a cell of mass m
    (particle masses) is within 2^-22 sum |q_p| + m 2^(e_c - 25) of the exact sum.  Integer adds commute: the result is
    the same bits on every call, whichever path a tile takes on the device, and whatever the other channels are; a
    float16 input gives the bits of its float32 widening.

    Raises NBEError for a non-finite position, velocity or quantity value, and when a cell holds 2^17 particle masses or
    more: |S| <= M 2^24 stays below 2^63 only for M < 2^39 units."""
    x, q, v, los, f, n, boxsize, res, worder = _validate_field(displacement, quantity, boxsize, res, worder, normalize,
                                                               fill, velocity, los, velocity_to_length)
    dev = _device_of(q)
    dtypes = (torch.float32, torch.float16)
    xd = None if x is None else _to_device(x, dev, dtypes)
    qd = _to_device(q, dev, dtypes)
    single = qd.ndim == 3
    if single:
        qd = qd[None]
    vd = None if v is None else _los_component(_to_device(v, dev, dtypes), los, n)
    field, delta, stats = _paint_fields(xd, qd, vd, los, f, n, boxsize, res, worder, normalize, float(fill),
                                        bool(return_delta))
    _check_stats(stats, "paint_field", True)
    if deconvolve:
        with torch.cuda.device(dev):
            field = torch.stack([_deconvolve(field[c], worder) for c in range(field.shape[0])])
    if single:
        field = field[0]
    return (_back(q, field), _back(q, delta)) if return_delta else _back(q, field)


# ---- particle catalogues --------------------------------------------------------------------

_KEY_EDGES = (4, 8)             # nbe_particle_keys: mesh cells per tile edge below / from _KEY_SPARSE cells per particle,
_KEY_SPARSE = 4                 # row-major tiles: about 64 particles per tile (DESIGN.md section 12.6 has the runs)
_KEY_MORTON = False
_AUTO_MIN_COUNT = 1 << 18       # sort="auto" sorts from this many particles on, if the mesh has at most
_AUTO_MAX_CELLS_PER_PARTICLE = 8    # this many cells per particle: sparser chunks do not fit the LDS image, sorted or not
_MAX_PARTICLES = (1 << 31) - 1


def _check_sort(sort):
    if not (isinstance(sort, (bool, np.bool_)) or sort == "auto"):
        raise ValueError("sort must be True, False or 'auto', got %r" % (sort,))
    return sort if isinstance(sort, str) else bool(sort)


def _validate_particles(positions, boxsize, res, worder, weights, quantity, normalize, fill, velocity, los,
                        velocity_to_length, sort):
    x = _check_array(positions, "positions")
    if x.ndim != 2 or x.shape[1] != 3:
        raise ValueError("positions must have shape (count, 3), got %s" % (tuple(x.shape),))
    if _dtype_name(x) not in ("float32", "float64"):
        raise ValueError("positions must be float32 or float64, got %s" % _dtype_name(x))
    count = int(x.shape[0])
    if count < 1:
        raise ValueError("paint_particles: the catalogue is empty (positions has shape %s)" % (tuple(x.shape),))
    if count > _MAX_PARTICLES:
        raise ValueError("paint_particles: %d particles exceed one call (2^31 - 1)" % count)
    boxsize, res, worder = _triple(boxsize, "boxsize", "a length"), _triple(res, "res", "an int"), _check_worder(worder)
    if weights is not None and quantity is not None:
        raise ValueError("paint_particles: weights together with a quantity are not supported (pass one of them)")
    w = q = None
    if weights is not None:
        w = _check_array(weights, "weights")
        if tuple(w.shape) != (count,):
            raise ValueError("weights must have shape (%d,), got %s" % (count, tuple(w.shape)))
        if _dtype_name(w) not in ("float32", "float64"):
            raise ValueError("weights must be float32 or float64, got %s" % _dtype_name(w))
        _same_kind(x, w, "positions", "weights")
        if not _is_torch(w):
            _check_weights(bool(np.isfinite(w).all() and (w >= 0).all()), float(np.sum(w, dtype=np.float64)))
    if quantity is not None:
        q = _check_array(quantity, "quantity")
        if tuple(q.shape) != (count,) and not (q.ndim == 2 and 1 <= q.shape[0] <= _MAX_CHANNELS and q.shape[1] == count):
            raise ValueError("quantity must have shape (%d,) or (C, %d) with 1 <= C <= %d, got %s"
                             % (count, count, _MAX_CHANNELS, tuple(q.shape)))
        if _dtype_name(q) not in ("float32", "float16"):
            raise ValueError("quantity must be float32 or float16, got %s" % _dtype_name(q))
        _same_kind(x, q, "positions", "quantity")
    if normalize not in _NORMALIZE:
        raise ValueError("normalize must be 'density' or 'mean', got %r" % (normalize,))
    _real(fill, "fill")
    los = _check_los(los)
    v = f = None
    if velocity is not None:
        v = _check_array(velocity, "velocity")
        if tuple(v.shape) not in ((count,), (count, 3)):
            raise ValueError("velocity must have shape (%d,) or (%d, 3), got %s" % (count, count, tuple(v.shape)))
        if _dtype_name(v) not in ("float32", "float64", "float16"):
            raise ValueError("velocity must be float32, float64 or float16, got %s" % _dtype_name(v))
        _same_kind(x, v, "positions", "velocity")
        if velocity_to_length is None:
            raise ValueError("velocity_to_length is required with a velocity (rsd_factor(z, Om) for redshift space)")
        f = _real(velocity_to_length, "velocity_to_length")
    return x, count, boxsize, res, worder, w, q, v, los, f, _check_sort(sort)


def _check_weights(valid, total):
    if not valid:
        raise ValueError("weights must be finite and non-negative")
    if not total > 0:
        raise ValueError("paint_particles: the total weight is zero")


def _exact_sum(t):
    """The sum of an int64 tensor as a Python int: exact where torch.sum over all of it would wrap."""
    return (int(torch.sum(t >> 32)) << 32) + int(torch.sum(t & 0xFFFFFFFF))


def _paint_particles(p, q, v, los, scale, boxsize, res, worder, sort="auto", normalize="density", fill=0.0,
                     want_delta=False, weighted=False, tile_edge=None, morton=None, timer=None):
    """Device work of paint_particles.  p: contiguous CUDA (count, 3) float32 / float64 tensor; q: contiguous (C, count)
    float32 / float16 tensor or None (masses only); v: contiguous (count,) float32 / float16 tensor or None.  With
    `weighted`, q is the (1, count) weights and delta is their density contrast.  tile_edge and morton override the key of
    the sort (measurements).  `timer(name)` is called before every stage (range, keys, sort, paint, convert) and
    timer(None) at the end (tools/time_particles.py).  Returns (field (C,) + res or None, delta or None, stats):
    stats[0] chunks of 512 particles on the direct path, stats[1] particles not painted, stats[2] cells at the overflow
    limit.  Raises NBEError for a non-finite quantity."""
    l = _lib.lib()
    dev = p.device
    half = lambda t: 1 if t is not None and t.dtype == torch.float16 else 0
    pdt = 2 if p.dtype == torch.float64 else 0              # include/nbe.h: NBE_F64, NBE_F32
    nchan = 0 if q is None else int(q.shape[0])
    count = int(p.shape[0])
    cells = res[0] * res[1] * res[2]
    tick = timer or (lambda name: None)
    if sort == "auto":
        sort = count >= _AUTO_MIN_COUNT and cells <= _AUTO_MAX_CELLS_PER_PARTICLE * count
    with torch.cuda.device(dev):
        s = _stream(dev)
        L3, r3 = (C.c_double * 3)(*boxsize), _i64(res)
        shift = (_ptr(v) if v is not None else None, half(v), los, float(scale) if v is not None else 0.0)
        tick("range")
        exps = (C.c_int * _MAX_CHANNELS)()
        if nchan:
            rng = torch.zeros(nchan + 1, dtype=torch.int32, device=dev)
            _lib.check(l.nbe_quantity_range(_ptr(q), half(q), nchan, count, _ptr(rng), s))
            r = rng.cpu().numpy()
            if int(r[nchan]):
                raise NBEError("paint_particles: %d value(s) of the %s are not finite"
                               % (int(r[nchan].view(np.uint32)), "weights" if weighted else "quantity"))
            for c, e in enumerate(np.frexp(r[:nchan].view(np.float32).astype(np.float64))[1]):
                exps[c] = int(e)
        order = None
        if sort:
            tick("keys")
            keys = torch.empty(count, dtype=torch.int64, device=dev)
            edge = tile_edge or _KEY_EDGES[cells >= _KEY_SPARSE * count]
            _lib.check(l.nbe_particle_keys(_ptr(p), pdt, *shift, count, L3, r3, int(edge),
                                           int(_KEY_MORTON if morton is None else morton), _ptr(keys), s))
            tick("sort")
            order = torch.sort(keys)[1]
            del keys
        tick("paint")
        mesh = torch.zeros(res, dtype=torch.int64, device=dev)
        qmesh = torch.zeros((nchan,) + tuple(res), dtype=torch.int64, device=dev) if nchan else None
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(l.nbe_paint_particles(_ptr(p), pdt, _ptr_or_null(order), _ptr(q) if nchan else None, half(q), nchan,
                                         exps, *shift, count, L3, r3, worder, _ptr(mesh),
                                         _ptr(qmesh) if nchan else None, _ptr(stats), s))
        tick("convert")
        field = delta = None
        if weighted:
            # every painted particle's weights sum to exactly 2^22: the total is 2^22 sum(V), and sum(V) takes the place of
            # the particle count in the mean
            total = max(_exact_sum(qmesh[0]) >> 22, 1)
            delta = torch.empty(res, dtype=torch.float32, device=dev)
            _lib.check(l.nbe_mesh_to_delta(_ptr(qmesh[0]), r3, total, _ptr(delta), s))
            stats[2] = torch.count_nonzero(mesh >= (1 << 39)).to(torch.int32)     # nbe_mesh_to_field's overflow guard
        else:
            if nchan:
                field = torch.empty((nchan,) + tuple(res), dtype=torch.float32, device=dev)
                _lib.check(l.nbe_mesh_to_field(_ptr(mesh), _ptr(qmesh), nchan, exps, r3, count, _NORMALIZE[normalize],
                                               float(fill), _ptr(field), _ptr(stats), s))
            if want_delta:
                delta = torch.empty(res, dtype=torch.float32, device=dev)
                _lib.check(l.nbe_mesh_to_delta(_ptr(mesh), r3, count, _ptr(delta), s))
        tick(None)
    return field, delta, stats


def paint_particles(positions, boxsize=1000.0, res=512, worder=2, deconvolve=True, weights=None, velocity=None, los=2,
                    velocity_to_length=None, sort="auto", quantity=None, normalize="density", fill=0.0,
                    return_delta=False):
    """Mass assignment of a particle catalogue onto a periodic mesh: halos, a subsample, an N-body snapshot (nbodykit's
    catalogue-to-mesh step, ArrayCatalog(...).to_mesh(Nmesh, resampler).compute(); the positions the reference builds in
    scripts/halos.py:394-403 reach a mesh this way).  paint_density and paint_field for positions that are not a lattice.

    positions: (count, 3) float32 / float64, NumPy array or CUDA tensor, in the units of the box; any number of boxes away,
    negative values included.  Particle p sits at the mesh coordinate x_c res_c / L_c (float64), wrapped periodically.
    boxsize, res, worder, deconvolve: as paint_density.
    weights: (count,) non-negative float32 / float64 (read as float32), same kind and device.  The call then returns
    sum(w m) / mean - 1, m the assignment weights: the weights ride as a quantity channel, and the mean is the exact
    integer total of that channel's mesh over the number of cells.
    quantity: (count,) or (C, count), C <= 4, float32 / float16: paint_field's two normalisations (`normalize`, `fill`,
    `return_delta`, and `deconvolve` divides every channel by the window) with unit masses.  The call returns the field
    (res, or (C,) + res), and with return_delta also the density contrast of the same pass, not deconvolved.
    weights together with a quantity raise ValueError: a weighted mean of a quantity is not built.
    velocity, los, velocity_to_length: velocity (count,) or (count, 3), of which component `los` is read (as float32),
    moves every particle by velocity_to_length * v along array axis los first (paint_density's redshift-space shift).
    sort: True sorts the particles by the mesh tile they fall into before painting (nbe_particle_keys, torch.sort), so
    that the 512 particles a workgroup paints share an LDS image; False paints them in the order given; "auto" sorts
    from 2^18 particles on where the mesh has at most 8 cells per particle.  The sums are
    integers: the result is the same bits for every `sort` and every order of the rows.

    Returns float32, NumPy for NumPy input, CUDA tensors on the input's device (torch's current stream) for tensors.
    Raises ValueError, before any device work, for an empty catalogue, wrong shapes, kinds or devices, and for NumPy
    weights that are negative, not finite or sum to zero (tensor weights are checked on the device first); NBEError for a
    non-finite or out-of-range position or velocity (the message names their number), a non-finite quantity, and a cell
    that holds 2^17 particle masses or more under a quantity or weights (paint_field's limit)."""
    x, count, boxsize, res, worder, w, q, v, los, f, sort = _validate_particles(
        positions, boxsize, res, worder, weights, quantity, normalize, fill, velocity, los, velocity_to_length, sort)
    dev = _device_of(x)
    pd = _to_device(x, dev, (torch.float32, torch.float64))
    vd = None
    if v is not None:
        vd = _to_device(v, dev, (torch.float32, torch.float64, torch.float16))
        vd = (vd[:, los] if vd.ndim == 2 else vd)
        vd = (vd if vd.dtype == torch.float16 else vd.to(torch.float32)).contiguous()
    qd, single = None, False
    if w is not None:
        wd = _to_device(w, dev, (torch.float32, torch.float64))
        if _is_torch(w):
            _check_weights(bool((torch.isfinite(wd) & (wd >= 0)).all()), float(wd.sum(dtype=torch.float64)))
        qd = wd.to(torch.float32).reshape(1, count).contiguous()
    elif q is not None:
        qd = _to_device(q, dev, (torch.float32, torch.float16))
        single = qd.ndim == 1
        qd = qd.reshape(-1, count)
    field, delta, stats = _paint_particles(pd, qd, vd, los, f, boxsize, res, worder, sort, normalize, float(fill),
                                           want_delta=q is None or bool(return_delta), weighted=w is not None)
    _check_stats(stats, "paint_particles", qd is not None)
    with torch.cuda.device(dev):
        if q is None:
            return _back(x, _deconvolve(delta, worder) if deconvolve else delta)
        if deconvolve:
            field = torch.stack([_deconvolve(field[c], worder) for c in range(field.shape[0])])
    if single:
        field = field[0]
    return (_back(x, field), _back(x, delta)) if return_delta else _back(x, field)


# ---- mesh readout ----------------------------------------------------------------------------

def _validate_read(field, boxsize, positions, displacement, lattice, worder, fill, sort):
    f = _check_array(field, "field")
    if f.ndim not in (3, 4) or min(f.shape) < 1 or (f.ndim == 4 and f.shape[0] > _MAX_CHANNELS):
        raise ValueError("field must have shape (r0, r1, r2) or (C, r0, r1, r2) with 1 <= C <= %d, got %s"
                         % (_MAX_CHANNELS, tuple(f.shape)))
    if _dtype_name(f) != "float32":
        raise ValueError("field must be float32, got %s" % _dtype_name(f))
    res = tuple(int(v) for v in f.shape[-3:])
    if max(res) > 1 << 20:
        raise ValueError("read_mesh: mesh %s unsupported (up to 2^20 cells a side)" % (res,))
    boxsize, worder = _triple(boxsize, "boxsize", "a length"), _check_worder(worder)
    if isinstance(fill, (bool, np.bool_)) or not isinstance(fill, numbers.Real):
        raise ValueError("fill must be a number (nan included), got %r" % (fill,))
    sort = _check_sort(sort)
    if sum(a is not None for a in (positions, displacement, lattice)) != 1:
        raise ValueError("read_mesh needs exactly one of positions, displacement and lattice")
    x = n = None
    if positions is not None:
        x = _check_array(positions, "positions")
        if x.ndim != 2 or x.shape[1] != 3:
            raise ValueError("positions must have shape (count, 3), got %s" % (tuple(x.shape),))
        if _dtype_name(x) not in ("float32", "float64"):
            raise ValueError("positions must be float32 or float64, got %s" % _dtype_name(x))
        if not 1 <= int(x.shape[0]) <= _MAX_PARTICLES:
            raise ValueError("read_mesh: %d rows unsupported (1 .. 2^31 - 1)" % int(x.shape[0]))
    elif displacement is not None:
        x = _check_array(displacement, "displacement")
        if x.ndim != 4 or x.shape[0] != 3 or min(x.shape) < 1:
            raise ValueError("displacement must have shape (3, N0, N1, N2), got %s" % (tuple(x.shape),))
        if _dtype_name(x) not in ("float32", "float16"):
            raise ValueError("displacement must be float32 or float16, got %s" % _dtype_name(x))
        n = tuple(int(v) for v in x.shape[1:])
    else:
        n = _triple(lattice, "lattice", "an int")
    if n is not None and n[0] * n[1] * n[2] > _MAX_PARTICLES:
        raise ValueError("read_mesh: a lattice of %s exceeds one call (2^31 - 1 rows)" % (n,))
    if x is not None:
        _same_kind(f, x, "field", "positions" if positions is not None else "displacement")
    return f, res, boxsize, worder, float(fill), sort, x, n


def _read_mesh(f, res, boxsize, worder, fill, p=None, x=None, n=None, sort=False):
    """Device work of read_mesh.  f: contiguous CUDA (C,) + res float32 tensor; p: contiguous (count, 3) float32 / float64
    positions, or None: the lattice n, displaced by the contiguous (3,) + n float32 / float16 tensor x or bare.  Returns
    (out (C, count) float32, stats): stats[1] rows that got `fill`."""
    l = _lib.lib()
    dev = f.device
    nchan = int(f.shape[0])
    count = int(p.shape[0]) if p is not None else n[0] * n[1] * n[2]
    cells = res[0] * res[1] * res[2]
    if sort == "auto":
        # paint_particles sorts from 2^18 rows on because an LDS image saves it global atomics; the readout has none to save,
        # and on a fully shuffled catalogue of 512^3 rows keys + torch.sort cost more than the locality returns (19.7 ms
        # sorted against 16.7 ms unsorted, profiles/web_timing_512.txt): "auto" reads in the order given
        sort = False
    with torch.cuda.device(dev):
        s = _stream(dev)
        L3, r3 = (C.c_double * 3)(*boxsize), _i64(res)
        order = None
        pdt = 0
        if p is not None:
            pdt = 2 if p.dtype == torch.float64 else 0
            if sort:
                keys = torch.empty(count, dtype=torch.int64, device=dev)
                edge = _KEY_EDGES[cells >= _KEY_SPARSE * count]
                _lib.check(l.nbe_particle_keys(_ptr(p), pdt, None, 0, 0, 0.0, count, L3, r3, int(edge), int(_KEY_MORTON),
                                               _ptr(keys), s))
                order = torch.sort(keys)[1]
                del keys
        out = torch.empty((nchan, count), dtype=torch.float32, device=dev)
        stats = torch.zeros(4, dtype=torch.int32, device=dev)
        _lib.check(l.nbe_mesh_read(_ptr(f), nchan, r3, _ptr_or_null(x), 1 if x is not None and x.dtype == torch.float16 else 0,
                                   _i64(n) if n is not None else None, _ptr_or_null(p), pdt, _ptr_or_null(order), count, L3,
                                   worder, fill, _ptr(out), _ptr(stats), s))
    return out, stats


def read_mesh(field, boxsize=1000.0, positions=None, displacement=None, worder=2, fill=float("nan"), sort="auto",
              lattice=None, return_stats=False):
    """The value of a mesh at particles: the adjoint of the painters (nbodykit's mesh.readout(position, resampler),
    Pylians' MASL.CIC_interp; the reference has no such step).  What a halo's environment, a reconstruction or a velocity
    at a particle is read with.

    field: (r0, r1, r2) or (C, r0, r1, r2) float32, C <= 4, NumPy array or CUDA tensor; a periodic mesh over boxsize.
    Exactly one of: positions, (count, 3) float32 / float64 as paint_particles takes them (any number of boxes away);
    displacement, (3, N0, N1, N2) float32 / float16, the displaced lattice of paint_density; lattice, an int or a 3-tuple,
    the bare lattice.  worder: the window, as the painters'.  Returns float32 of the field's kind: (count,) or (C, count)
    for positions, (N0, N1, N2) or (C, N0, N1, N2) for the lattice forms.  With return_stats also {"not_read": rows}.

    out_c = 2^-22 sum of q f_c[node] over the integer weights q that the painter of the same worder adds for the row (they
    sum to exactly 2^22), summed in float64 in the weights' order and rounded once: a constant field reads back as itself,
    and sum(mesh * g) == sum(read(g) * 2^22) holds exactly for paint_particles' integer mesh and an integer-valued g.  A
    row the painters would reject (non-finite, or beyond 2^30 mesh cells) gets `fill` in every channel.  sort: True reads
    the rows in the order of the mesh tile they fall into, with paint_particles' key and torch.sort (locality only: one
    writer per word, the same bits for every sort and every order of the rows); False reads them in the order given;
    "auto" is False, because the sort measured slower than what it saves."""
    f, res, boxsize, worder, fill, sort, x, n = _validate_read(field, boxsize, positions, displacement, lattice, worder,
                                                               fill, sort)
    if not isinstance(return_stats, (bool, np.bool_)):
        raise ValueError("return_stats must be a bool, got %r" % (return_stats,))
    dev = _device_of(f)
    fd = _to_device(f, dev, (torch.float32,))
    single = fd.ndim == 3
    fd = fd.reshape((-1,) + res)
    if positions is not None:
        out, stats = _read_mesh(fd, res, boxsize, worder, fill, p=_to_device(x, dev, (torch.float32, torch.float64)),
                                sort=sort)
    else:
        xd = None if x is None else _to_device(x, dev, (torch.float32, torch.float16))
        out, stats = _read_mesh(fd, res, boxsize, worder, fill, x=xd, n=n)
        out = out.reshape((-1,) + tuple(n))
    if single:
        out = out[0]
    out = _back(f, out)
    return (out, {"not_read": int(stats[1])}) if return_stats else out


def shot_noise(boxsize, count=None, weights=None):
    """Poisson shot noise of a catalogue's power spectrum, on the host: L^3 / count, or L^3 sum(w^2) / sum(w)^2 with
    weights.  A float, in the units of power_spectrum's P."""
    L = _triple(boxsize, "boxsize", "a length")
    vol = L[0] * L[1] * L[2]
    if weights is not None:
        w = weights.cpu().numpy() if _is_torch(weights) else np.asarray(weights)
        w = w.astype(np.float64).ravel()
        if w.size == 0 or not np.isfinite(w).all() or (w < 0).any() or not w.sum() > 0:
            raise ValueError("shot_noise: weights must be finite, non-negative and not all zero")
        return float(vol * np.sum(w * w) / np.sum(w) ** 2)
    if isinstance(count, (bool, np.bool_)) or not isinstance(count, numbers.Integral) or int(count) < 1:
        raise ValueError("shot_noise needs weights or a count >= 1, got %r" % (count,))
    return float(vol / int(count))


def correlation_arrays(k, p_aa, p_bb, p_ab, nmodes):
    """cross_correlation's dict from the three spectra (host float64 arithmetic): r = p_ab / sqrt(p_aa p_bb),
    transfer = sqrt(p_aa / p_bb), bias = p_ab / p_bb; NaN, without a warning, where a denominator is 0."""
    k, p_aa, p_bb, p_ab, nmodes = (np.asarray(v, dtype=np.float64) for v in (k, p_aa, p_bb, p_ab, nmodes))
    with np.errstate(invalid="ignore", divide="ignore"):
        den = np.sqrt(p_aa * p_bb)
        r = np.where(den > 0, p_ab / den, np.nan)
        transfer = np.where(p_bb > 0, np.sqrt(p_aa / p_bb), np.nan)
        bias = np.where(p_bb > 0, p_ab / p_bb, np.nan)
    return dict(k=k, p_aa=p_aa, p_bb=p_bb, p_ab=p_ab, nmodes=nmodes, r=r, transfer=transfer, bias=bias)


def cross_correlation(a, b, boxsize=1000.0):
    """Cross-correlation coefficient, transfer function and bias of two fields per shell (Pylians' Pk_library.XPk as the
    reference uses it, scripts/utils.py:1451-1470 and scripts/test_upsampling.py:159-183: XPk / sqrt(Pk_a Pk_b) of the
    emulated against the target field).

    a, b: (n, n, n) float32, NumPy arrays or CUDA tensors on one device.  boxsize: L (scalar, or a 3-tuple of equal
    values).  Returns a dict of float64 NumPy arrays of n // 2 shells: k, p_aa, p_bb, p_ab, nmodes -- bit for bit what
    power_spectrum(a), power_spectrum(b) and power_spectrum(a, other=b) return, from one rfftn per field --, and
    r = p_ab / sqrt(p_aa p_bb), transfer = sqrt(p_aa / p_bb), bias = p_ab / p_bb (NaN where a denominator is 0).  For
    halos against matter (a = delta_h, b = delta_m) `bias` is the cross bias P_hm / P_mm; nothing is subtracted."""
    if b is None:
        raise ValueError("cross_correlation needs two fields, got b = None")
    d, n, L, o = _validate_spectrum(a, boxsize, b, "cross_correlation", 4096)
    dev = _device_of(d)
    nb = n // 2 + 1
    koff = np.arange(1, nb, dtype=np.float64)
    with torch.cuda.device(dev):
        fa, fb = _half_spectra(d, o, dev)
        out = []
        for x, y in ((fa, None), (fb, None), (fa, fb)):
            binmax = torch.zeros(nb, dtype=torch.int32, device=dev)
            sums = torch.zeros(3 * nb, dtype=torch.int64, device=dev)
            _lib.check(_lib.lib().nbe_power_spectrum(_ptr(x), _ptr_or_null(y), n, _ptr(binmax), _ptr(sums), _stream(dev)))
            sm = sums.cpu().numpy().reshape(3, nb)[:, 1:]
            out.append(_shell_means(binmax.cpu().numpy()[1:], sm[0], sm[1], sm[2], koff, _KEXP, L, n))
    return correlation_arrays(out[0][0], out[0][1], out[1][1], out[2][1], out[0][2])


def rsd_factor(z, Om):
    """(1 + z) / H(z) in (Mpc/h) per (km/s): the comoving displacement of a proper peculiar velocity along the line of
    sight, s = x + v_los (1 + z) / H(z), with cosmology.hubble_rate.  A Python float."""
    from .cosmology import hubble_rate
    z, Om = _real(z, "z"), _real(Om, "Om")
    return (1.0 + z) / float(hubble_rate(z, Om))


def deconvolve_mas(delta, worder=2):
    """Divide a painted field by its assignment window (reference scripts/utils.py:136-148, deconvolve_mas_kernel):
    delta_k / prod_c sinc(k_c L_c / (2 res_c))^worder on the rfft of the mesh.  The window depends on k_c L_c / res_c
    only, so no box size is needed.  delta: 3-D float32 NumPy array or CUDA tensor; returns the same kind."""
    d = _check_array(delta, "delta")
    if d.ndim != 3 or min(d.shape) < 1:
        raise ValueError("delta must be a 3-D mesh, got shape %s" % (tuple(d.shape),))
    if _dtype_name(d) != "float32":
        raise ValueError("delta must be float32, got %s" % _dtype_name(d))
    worder = _check_worder(worder)
    dev = _device_of(d)
    with torch.cuda.device(dev):
        return _back(d, _deconvolve(_to_device(d, dev, (torch.float32,)), worder))


def power_spectrum(delta, boxsize=1000.0, other=None):
    """Shell-averaged power spectrum of a cubic mesh (reference scripts/utils.py:1083-1085, Pylians Pk_library.Pk);
    with `other`, the cross spectrum Re<delta other*>.

    delta / other: (n, n, n) float32, NumPy arrays or CUDA tensors on one device.  boxsize: L (scalar, or a 3-tuple of
    equal values).  Returns (k, pk, nmodes), float64 NumPy arrays of n // 2 shells: the mean |k| (h/Mpc for L in Mpc/h),
    the mean P = |delta_k|^2 L^3 / n^6 and the number of modes of the full complex grid."""
    d, n, L, o = _validate_spectrum(delta, boxsize, other, "power_spectrum", 4096)
    dev = _device_of(d)
    nb = n // 2 + 1
    with torch.cuda.device(dev):
        a, b = _half_spectra(d, o, dev)
        binmax = torch.zeros(nb, dtype=torch.int32, device=dev)
        sums = torch.zeros(3 * nb, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().nbe_power_spectrum(_ptr(a), _ptr_or_null(b), n, _ptr(binmax), _ptr(sums), _stream(dev)))
        bm = binmax.cpu().numpy()[1:]
        sm = sums.cpu().numpy().reshape(3, nb)[:, 1:]
    return _shell_means(bm, sm[0], sm[1], sm[2], np.arange(1, nb, dtype=np.float64), _KEXP, L, n)


def _validate_spectrum(delta, boxsize, other, what, max_n):
    """The inputs of the two-point calls: (delta, n, L, other or None)."""
    d, n, L = _cubic(delta, "delta", boxsize, what, "mesh", 2, max_n)
    o = None
    if other is not None:
        o = _check_array(other, "other")
        if tuple(o.shape) != tuple(d.shape) or _dtype_name(o) != "float32":
            raise ValueError("other must match delta: float32 %s, got %s %s"
                             % (tuple(d.shape), _dtype_name(o), tuple(o.shape)))
        _same_kind(d, o, "delta", "other")
    return d, n, L, o


def _half_spectra(d, o, dev):
    """(a, b or None): the row-major half spectra of delta and, where given, of other, on the device."""
    a = torch.fft.rfftn(_to_device(d, dev, (torch.float32,))).contiguous()
    b = torch.fft.rfftn(_to_device(o, dev, (torch.float32,))).contiguous() if o is not None else None
    return a, b


def _ptr_or_null(t):
    return _ptr(t) if t is not None else None


def power_spectrum_multipoles(delta, boxsize=1000.0, los=2, other=None):
    """Monopole, quadrupole and hexadecapole of the power spectrum about the array axis `los` (reference
    scripts/utils.py:1083-1085, :1447-1449: the columns Pk[:, 0..2] of Pylians' Pk_library.Pk(delta, boxsize, axis));
    with `other`, of the cross spectrum Re<delta other*>.

    P_l(s) = (2 l + 1) sum(w p L_l(mu)) / sum(w) L^3 / n^6 over the shells, weights and terms p of `power_spectrum`, with
    mu^2 = m_los^2 / |m|^2 and the Legendre polynomials L_0 = 1, L_2 = (3 mu^2 - 1) / 2, L_4 = (35 mu^4 - 30 mu^2 + 3) / 8.
    For a redshift-space density, los is the axis the particles were moved along (paint_density's `los`).

    delta / other: (n, n, n) float32, 2 <= n <= 2048, NumPy arrays or CUDA tensors on one device.  Returns a dict of
    float64 NumPy arrays of n // 2 shells: k, p0, p2, p4, nmodes.  k, p0 and nmodes are the bits of `power_spectrum`;
    values are NaN in a shell that holds a non-finite term."""
    d, n, L, o = _validate_spectrum(delta, boxsize, other, "power_spectrum_multipoles", _PK_ANISO_MAX_N)
    los = _check_los(los)
    dev = _device_of(d)
    nb = n // 2 + 1
    with torch.cuda.device(dev):
        a, b = _half_spectra(d, o, dev)
        binmax = torch.zeros(nb, dtype=torch.int32, device=dev)
        sums = torch.zeros(5 * nb, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().nbe_power_multipoles(_ptr(a), _ptr_or_null(b), n, los, _ptr(binmax), _ptr(sums),
                                                   _stream(dev)))
        bm = binmax.cpu().numpy()[1:]
        sm = sums.cpu().numpy().reshape(5, nb)[:, 1:]
    koff = np.arange(1, nb, dtype=np.float64)
    k, p0, cnt = _shell_means(bm, sm[0], sm[1], sm[2], koff, _KEXP, L, n)
    p2, p4 = (_shell_means(bm, sm[0], sm[1], sm[w], koff, _KEXP, L, n)[1] for w in (3, 4))
    return dict(k=k, p0=p0, p2=5.0 * p2, p4=9.0 * p4, nmodes=cnt)


def _check_nmu(nmu):
    if isinstance(nmu, (bool, np.bool_)) or not isinstance(nmu, numbers.Integral) or not 1 <= int(nmu) <= _PK_MAX_MU:
        raise ValueError("nmu must be an int in 1 .. %d, got %r" % (_PK_MAX_MU, nmu))
    return int(nmu)


def power_spectrum_wedges(delta, boxsize=1000.0, los=2, nmu=5, other=None, _max_bins=None):
    """The power spectrum in wedges of |mu| = |k_los| / |k| about the array axis `los` (reference scripts/utils.py:1083-1085,
    :1447-1449: the 2-D spectrum of Pylians' Pk_library.Pk(delta, boxsize, axis), here binned in (k, mu)); with `other`,
    the cross spectrum Re<delta other*>.

    The shells, weights and terms are those of `power_spectrum`.  Of `nmu` equal bins of |mu| in [0, 1], 1 <= nmu <= 64,
    mode m falls into bin floor(nmu |mu|), and |mu| = 1 into the last: decided in integers as
    min(nmu - 1, #{ j in 1 .. nmu-1 : j^2 |m|^2 <= nmu^2 m_los^2 }), so no bin edge depends on a rounding.

    delta / other: (n, n, n) float32, 2 <= n <= 2048, NumPy arrays or CUDA tensors on one device.  Returns a dict of
    float64 NumPy arrays: k, mu (the mean |k| and |mu| of the bin's modes), pk and nmodes of shape (nmu, n // 2), and
    mu_edges = arange(nmu + 1) / nmu.  A bin without a mode, or in a shell that holds a non-finite term, is NaN.
    `_max_bins` caps the (mu, k) bins of one launch (tests): the sums are integers, so the bits do not depend on it."""
    d, n, L, o = _validate_spectrum(delta, boxsize, other, "power_spectrum_wedges", _PK_ANISO_MAX_N)
    los, nmu = _check_los(los), _check_nmu(nmu)
    dev = _device_of(d)
    nb = n // 2 + 1
    with torch.cuda.device(dev):
        a, b = _half_spectra(d, o, dev)
        binmax = torch.zeros(nb, dtype=torch.int32, device=dev)
        sums = torch.zeros(4 * nmu * nb, dtype=torch.int64, device=dev)
        _lib.check(_lib.lib().nbe_power_wedges(_ptr(a), _ptr_or_null(b), n, los, nmu, int(_max_bins or 0), _ptr(binmax),
                                               _ptr(sums), _stream(dev)))
        bm = np.tile(binmax.cpu().numpy()[1:], (nmu, 1))
        sm = sums.cpu().numpy().reshape(4, nmu, nb)[:, :, 1:]
    koff = np.tile(np.arange(1, nb, dtype=np.float64), (nmu, 1))
    k, pk, cnt = _shell_means(bm, sm[0], sm[1], sm[3], koff, _KEXP, L, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        mu = np.ldexp(sm[2].astype(np.float64), -_KEXP) / cnt
    return dict(k=k, mu=mu, pk=pk, nmodes=cnt, mu_edges=np.arange(nmu + 1) / nmu)


def _shell_means(binmax, weight, ksum, psum, koff, kexp, L, n):
    """(k, pk, modes), float64, from the integer shell sums of nbe_power_spectrum / nbe_shell_filter: binmax the shells'
    uint32 words, ksum in units of 2^-kexp about koff, psum in units of 2^(e - 32).  pk is NaN in a non-finite shell."""
    bm = binmax.view(np.float32).astype(np.float64)
    cnt = weight.astype(np.float64)
    _, e = np.frexp(np.where(np.isfinite(bm), bm, 1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        k = (koff + np.ldexp(ksum.astype(np.float64), -np.asarray(kexp, np.int64)) / cnt) * (2.0 * np.pi / L)
        pk = np.ldexp(psum.astype(np.float64), e - 32) / cnt * (L ** 3 / float(n) ** 6)
    return k, np.where(np.isfinite(bm), pk, np.nan), cnt


def _mf_thresholds(thresholds):
    if thresholds is None:
        return np.linspace(-3.0, 3.0, 41, dtype=np.float32)
    try:
        t = np.asarray(thresholds, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        raise ValueError("thresholds must be numbers, got %r" % (thresholds,))
    with np.errstate(over="ignore"):
        t = t.astype(np.float32)
    if not 2 <= t.size <= _MF_MAX_T:
        raise ValueError("thresholds must hold 2 .. %d values, got %d" % (_MF_MAX_T, t.size))
    if not np.isfinite(t).all():
        raise ValueError("thresholds must be finite in float32")
    return t


def _mf_validate(field, boxsize, thresholds):
    return _cubic(field, "field", boxsize, "minkowski_functionals", "(n, n, n) field", 1, _MF_MAX_N) + \
        (_mf_thresholds(thresholds),)


def _mf_values(counts, n, boxsize):
    """(v0, v1, v2, v3) float64 from (T, 4) element counts (n0, n1, n2, n3) of an n^3 mesh in a box of side boxsize."""
    c = np.asarray(counts, dtype=np.float64)
    n0, n1, n2, n3 = c[:, 0], c[:, 1], c[:, 2], c[:, 3]
    h = float(boxsize) / float(n)
    vol = float(boxsize) ** 3
    m0 = h ** 3 * n3
    m1 = h ** 2 * ((-2.0 / 3.0) * n3 + (2.0 / 9.0) * n2)
    m2 = h * ((2.0 / 3.0) * n3 - (4.0 / 9.0) * n2 + (2.0 / 9.0) * n1)
    m3 = n0 - n1 + n2 - n3
    return m0 / vol, m1 / vol, m2 / vol, m3 / vol


def minkowski_functionals(field, boxsize=1000.0, thresholds=None, standardize=True):
    """Minkowski functionals of the excursion sets of a periodic density field (reference scripts/utils.py:652-763,
    compute_minkowski_functionals; the driver scripts call it for every field they paint).

    field: (n, n, n) float32, NumPy array or CUDA torch tensor (read where it lives, on torch's current stream of its
    device), 1 <= n <= 2048.  Other dtypes raise ValueError (the reference casts to float32).  boxsize: L (scalar, or a
    3-tuple of equal values).  thresholds: default np.linspace(-3, 3, 41, dtype=float32); otherwise flattened and cast to
    float32, 2 .. 1024 finite values in any order, duplicates allowed; results come in the caller's order.

    Definition.  w is the field, standardized by default: w = (x - float32(mean)) / float32(std) in float32 (w = 0 where
    float32(std) is 0), where mean and the population std are taken on the device in float64, reproducibly.  For a
    threshold t, M = {voxels with w >= t}, indices mod n.  With e_a the unit step along axis a:
      n3 = |M|                                                    (cubes)
      n2 = sum over a of #{v : v or v - e_a in M}                 (faces between v and v - e_a)
      n1 = sum over a of #{v : v, v - e_b, v - e_c or v - e_b - e_c in M}, {b, c} the other axes   (edges along a)
      n0 = #{v : v - s in M for some s in {0, 1}^3}              (vertices)
    and with h = L / n: M0 = h^3 n3, M1 = h^2 (-2/3 n3 + 2/9 n2), M2 = h (2/3 n3 - 4/9 n2 + 2/9 n1),
    M3 = n0 - n1 + n2 - n3 (the Euler characteristic); v_i = M_i / L^3.

    Returns a dict of host objects: thresholds (float64 copies of the float32 values), v0 .. v3 (float64), mean and std
    (floats), standardize (bool), convention ("periodic_voxel_cubical_complex") and counts, an int64 (T, 4) array of
    (n0, n1, n2, n3).  A non-finite value anywhere in the field raises NBEError.

    Difference from the reference: it takes np.mean and np.std in float32; here they are float64.  A voxel whose
    standardized value is within a float32 rounding of a threshold can therefore fall on the other side of it than in the
    reference's own run.  The counts are computed in one pass over the field for all thresholds (DESIGN.md section
    12.1)."""
    f, n, L, thr = _mf_validate(field, boxsize, thresholds)
    standardize = bool(standardize)
    dev = _device_of(f)
    l = _lib.lib()
    T = int(thr.size)
    order = np.argsort(thr, kind="stable")
    with torch.cuda.device(dev):
        s = _stream(dev)
        x = _to_device(f, dev, (torch.float32,))
        thr_d = torch.from_numpy(np.ascontiguousarray(thr[order])).to(dev)
        mom = torch.empty(_MOMENT_WORDS, dtype=torch.float64, device=dev)
        hist = torch.zeros(4 * (T + 1) + 1, dtype=torch.int64, device=dev)
        _lib.check(l.nbe_field_moments(_ptr(x), n, _ptr(mom), s))
        _lib.check(l.nbe_minkowski_counts(_ptr(x), n, _ptr(thr_d), T, _ptr(mom) if standardize else None, _ptr(hist), s))
        h = hist.cpu().numpy()
        mean, std = (float(v) for v in mom[:2].cpu().numpy())
    bad = int(h[-1])
    if bad:
        raise NBEError("minkowski_functionals: %d voxel(s) of the field are not finite" % bad)
    tail = np.cumsum(h[:-1].reshape(4, T + 1)[:, ::-1], axis=1)[:, ::-1]     # tail[f, b] = elements with bin >= b
    counts = np.empty((T, 4), np.int64)
    counts[order] = tail[:, 1:].T                                              # sorted threshold k: bins > k
    v0, v1, v2, v3 = _mf_values(counts, n, L)
    return {"thresholds": thr.astype(np.float64), "v0": v0, "v1": v1, "v2": v2, "v3": v3, "mean": mean, "std": std,
            "standardize": standardize, "convention": MF_CONVENTION, "counts": counts}


# ---- bispectrum -----------------------------------------------------------------------------

def bispectrum_kappa3(kappa1, kappa2, theta):
    """|k1 + k2| / k_F for the angle theta between the vectors k1 and k2 (theta = 0: kappa1 + kappa2)."""
    th = np.asarray(theta, dtype=np.float64)
    return np.sqrt((kappa2 * np.sin(th)) ** 2 + (kappa2 * np.cos(th) + kappa1) ** 2)


def bispectrum_shell_bounds(kappa, dk):
    """Integer bounds [lo2, hi2) on |m|^2 of the shell lo^2 <= |m|^2 < hi^2, lo = max(kappa - dk/2, 0), hi = kappa + dk/2:
    the squares in float64, their ceilings as integers, and lo2 >= 1 because the DC mode belongs to no shell."""
    kappa = np.asarray(kappa, dtype=np.float64)
    lo = np.maximum(kappa - 0.5 * dk, 0.0)
    hi = kappa + 0.5 * dk
    lo2 = np.maximum(np.ceil(lo * lo), 1.0).astype(np.int64)
    hi2 = np.ceil(hi * hi).astype(np.int64)
    return lo2, hi2


def _shell_modes(lo2, hi2):
    """The wave vectors m of the full grid with lo2 <= |m|^2 < hi2 as (count, 4) int32 rows (m_x, m_y, m_z, 0)."""
    if hi2 <= lo2:
        return np.zeros((0, 4), np.int32)
    r = int(np.floor(np.sqrt(float(hi2 - 1))))
    while (r + 1) ** 2 < hi2:
        r += 1
    while r * r >= hi2:
        r -= 1
    a = np.arange(-r, r + 1, dtype=np.int64)
    plane = a[:, None] ** 2 + a[None, :] ** 2
    rows = []
    for mx in a:
        q = plane + mx * mx
        jy, jz = np.nonzero((q >= lo2) & (q < hi2))
        if jy.size:
            m = np.zeros((jy.size, 4), np.int32)
            m[:, 0] = mx
            m[:, 1] = a[jy]
            m[:, 2] = a[jz]
            rows.append(m)
    return np.concatenate(rows) if rows else np.zeros((0, 4), np.int32)


def _bk_validate(delta, boxsize, k1, k2, theta, dk, mas_worder):
    d, n, L = _cubic(delta, "delta", boxsize, "bispectrum", "(n, n, n) field", _BK_MIN_N, _BK_MAX_N)
    vals = {name: _real(v, name, positive=True) for name, v in (("k1", k1), ("k2", k2), ("dk", dk))}
    try:
        th = np.asarray(theta, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        raise ValueError("theta must be numbers, got %r" % (theta,))
    if not 1 <= th.size <= _BK_MAX_T:
        raise ValueError("theta must hold 1 .. %d angles, got %d" % (_BK_MAX_T, th.size))
    if not np.isfinite(th).all() or (th < 0).any() or (th > np.pi).any():
        raise ValueError("theta must be finite angles in [0, pi]")
    if mas_worder is not None:
        mas_worder = _check_worder(mas_worder)
    kF = 2.0 * np.pi / L
    ka1, ka2, dk = vals["k1"] / kF, vals["k2"] / kF, vals["dk"]
    if 2.0 * (ka1 + ka2) + 1.5 * dk >= n:
        raise ValueError("bispectrum: 2 (k1 + k2) / k_F + 1.5 dk = %.6g reaches the mesh size %d: triangles would close "
                         "modulo n only" % (2.0 * (ka1 + ka2) + 1.5 * dk, n))
    kappa = np.concatenate([[ka1, ka2], bispectrum_kappa3(ka1, ka2, th)])
    lo2, hi2 = bispectrum_shell_bounds(kappa, dk)
    modes = [_shell_modes(int(lo2[i]), int(hi2[i])) for i in (0, 1)]
    for i in (0, 1):
        if not len(modes[i]):
            raise ValueError("bispectrum: shell %d (k%d = %g, |m| in [%g, %g)) holds no mode of the mesh"
                             % (i + 1, i + 1, vals["k%d" % (i + 1)], max(kappa[i] - dk / 2, 0.0), kappa[i] + dk / 2))
    return d, n, L, th, kappa, lo2, hi2, modes, mas_worder


def _bk_shell_params(n, lo2, hi2):
    """(S, 4) int64 rows (lo2, hi2, koff, kexp) of nbe_shell_filter: |m| - koff is summed in units of 2^-kexp, chosen so
    that the sum over every mode the shell can hold stays below 2^62."""
    par = np.zeros((len(lo2), 4), np.int64)
    par[:, 0], par[:, 1] = lo2, hi2
    koff = np.floor(np.sqrt(lo2.astype(np.float64))).astype(np.int64)
    koff = np.where(koff * koff > lo2, koff - 1, koff)
    top = np.sqrt(np.maximum(hi2, 1).astype(np.float64)) + 1.0
    cap = np.minimum(float(n) ** 3, (2.0 * top + 1.0) ** 3)
    kexp = np.floor(60.0 - np.log2(cap * (top - koff + 1.0))).astype(np.int64)
    par[:, 2], par[:, 3] = koff, np.clip(kexp, 0, 36)
    return par


def _bk_batch(dev, n, want, max_batch):
    """How many third shells are filtered and transformed at once: from the free memory of the device.  A shell in flight
    costs its half spectrum, the copy the complex-to-real transform works on, its real field and the transform's
    workspace: four fields of 4 n^3 bytes are reserved for each."""
    if max_batch is not None:
        return max(1, min(int(max_batch), want))
    free = _free_memory(dev)
    per_shell = 16 * (n ** 3 + 2 * n * n)
    return max(1, min(want, int(0.7 * free) // per_shell))


def bispectrum(delta, boxsize=1000.0, k1=0.1, k2=0.1, theta=None, dk=1.0, mas_worder=None, _max_batch=None,
               _timings=None):
    """Bispectrum B(k1, k2, theta) and reduced bispectrum Q(theta) of a periodic density field (reference
    scripts/utils.py:1314-1399: Pylians Bk_library.Bk with threads=1, for k1 = k2 = 0.1 and k1 = 0.05, k2 = 0.1 h/Mpc at
    25 angles).

    delta: cubic (n, n, n) float32, NumPy array or CUDA tensor (read where it lives, on torch's current stream of its
    device), 4 <= n <= 2048.  boxsize: L (scalar, or a 3-tuple of equal values).  k1, k2: positive, in the units in which
    power_spectrum returns k (h/Mpc for a box in Mpc/h).  theta: 1 .. 256 finite angles in [0, pi], any order, duplicates
    allowed (default np.linspace(0, pi, 25)); results come in the caller's order.  dk: full shell width in units of
    k_F = 2 pi / L, positive.  mas_worder: None, or 1-4 to divide the spectrum by the assignment window first
    (deconvolve_mas's kernel; Pylians' MAS= argument).

    Definition.  Let kappa = k / k_F, let m in Z^3 run over the wave vectors of the full complex grid (each component in
    (-n/2, n/2]), and let delta_m be the unnormalised forward FFT.
    - kappa3(theta) = sqrt((kappa2 sin theta)^2 + (kappa2 cos theta + kappa1)^2).  theta is the angle between the vectors
      k1 and k2, so theta = 0 gives kappa1 + kappa2.
    - Shell S(kappa) = { m != 0 : lo^2 <= |m|^2 < hi^2 } with lo = max(kappa - dk/2, 0) and hi = kappa + dk/2.  The squares
      are taken in float64 and compared with the integer |m|^2.  The DC mode belongs to no shell.  Shells of neighbouring
      theta may overlap or leave gaps.
    - N_tri(theta) = #{ (m1, m2, m3) : m1 in S(kappa1), m2 in S(kappa2), m3 in S(kappa3(theta)), m1 + m2 + m3 = 0 }, an
      int64.
    - B(theta) = L^6 / n^9 * sum over those triangles of Re(delta_m1 delta_m2 delta_m3), divided by N_tri(theta).
    - P_i = L^3 / n^6 * mean of |delta_m|^2 over shell i.  Q(theta) = B / (P1 P2 + P2 P3(theta) + P3(theta) P1).
    - pk, k, nmodes have 2 + T entries: shell 1, shell 2, then one per theta.  They hold the mean power, the mean |k| and
      the mode count of each shell, computed by the integer-sum scheme of power_spectrum.
    - A theta whose N_tri is 0 returns ntriangles = 0 and NaN in B and Q.  An empty third shell gives NaN in its pk and k.
      (For k1 = k2 and theta = pi the third shell is empty.)  No warning, no exception.
    - Closure is exact, not modulo n: if 2 (kappa1 + kappa2) + 1.5 dk >= n the three outer radii can sum to n, and the
      call raises ValueError.

    Returns a dict of host arrays: theta, k3 (= kappa3 k_F), B, Q (float64, T entries), ntriangles (int64, T), pk, k
    (float64, 2 + T) and nmodes (int64, 2 + T).  ValueError before any device work for: an empty shell 1 or shell 2, a
    non-cubic or non-float32 field, a non-cubic box, theta outside [0, pi], n outside 4 .. 2048, and the closure condition
    above.  A non-finite voxel raises NBEError.

    This is the standard FFT estimator (Scoccimarro 2000), which is what Pylians' Bk computes: with I_S the indicator of a
    shell and F_S = irfftn(delta I_S), the sum over the voxels of F1 F2 F3 is n^-6 times the sum over the triangles.  The
    sums go through float32 transforms and a float64 reduction in a fixed order: the arrays are the same bits on every
    call and for every batch size.  N_tri is not taken from transforms of the indicators but counted in integers over the
    pairs (m1, m2), so it is exact at every mesh size (at the cost of |S1| |S2| integer operations).

    Difference from the reference: Pylians is not available where this library is developed, so its exact bin edges
    cannot be pinned; the shells are the ones defined above, and dk is a parameter so that a caller can match the width
    their Pylians uses.  Matching Pylians' numbers bit for bit is not claimed."""
    if theta is None:
        theta = np.linspace(0.0, np.pi, 25)
    d, n, L, th, kappa, lo2, hi2, modes, mas_worder = _bk_validate(delta, boxsize, k1, k2, theta, dk, mas_worder)
    dev = _device_of(d)
    l = _lib.lib()
    T, S = int(th.size), int(th.size) + 2
    kF = 2.0 * np.pi / L
    par = _bk_shell_params(n, lo2, hi2)
    edges = np.unique(np.concatenate([lo2[2:], hi2[2:]])).astype(np.int32)
    h = n // 2 + 1
    ev = []

    def mark(name):
        if _timings is not None:
            e = torch.cuda.Event(enable_timing=True)
            e.record(torch.cuda.current_stream(dev))
            ev.append((name, e))

    with torch.cuda.device(dev):
        s = _stream(dev)
        mark("start")
        x = _to_device(d, dev, (torch.float32,))
        spec = torch.fft.rfftn(x).contiguous()            # the kernels index the half spectrum row-major
        del x
        if mas_worder is not None:
            _lib.check(l.nbe_deconvolve_mas(_ptr(spec), _i64((n, n, n)), mas_worder, s))
        mark("rfftn")
        par_d = torch.from_numpy(par).to(dev)
        binmax = torch.zeros(S, dtype=torch.int32, device=dev)
        sums = torch.zeros((S, 3), dtype=torch.int64, device=dev)
        out = torch.zeros(T, dtype=torch.float64, device=dev)

        def fields(s0, cnt):
            """The real fields of shells s0 .. s0 + cnt - 1: filter (with the shells' sums), then one batched irfftn."""
            filt = torch.empty((cnt, n, n, h), dtype=torch.complex64, device=dev)
            mark("other")
            _lib.check(l.nbe_shell_filter(_ptr(spec), n, C.c_void_p(par_d.data_ptr() + 32 * s0), cnt, _ptr(filt),
                                          C.c_void_p(binmax.data_ptr() + 4 * s0), C.c_void_p(sums.data_ptr() + 24 * s0), s))
            mark("shell_filter")
            f = torch.fft.irfftn(filt, s=(n, n, n), dim=(1, 2, 3)).contiguous()
            mark("irfftn")
            return f

        f12 = fields(0, 2)
        batch = _bk_batch(dev, n, T, _max_batch)
        partials = torch.empty((min(batch, T), _BK_PARTIALS), dtype=torch.float64, device=dev)
        for t0 in range(0, T, batch):
            cnt = min(batch, T - t0)
            f3 = fields(2 + t0, cnt)
            _lib.check(l.nbe_triple_sums(_ptr(f12[0]), _ptr(f12[1]), _ptr(f3), cnt, n, _ptr(partials),
                                         C.c_void_p(out.data_ptr() + 8 * t0), s))
            mark("triple_sums")
            del f3
        del f12, spec
        hist = None
        if edges.size >= 2:
            m1 = torch.from_numpy(modes[0]).to(dev)
            m2 = torch.from_numpy(modes[1]).to(dev)
            ed = torch.from_numpy(edges).to(dev)
            hist_d = torch.zeros(edges.size + 1, dtype=torch.int64, device=dev)
            mark("other")
            _lib.check(l.nbe_triangle_counts(_ptr(m1), len(modes[0]), _ptr(m2), len(modes[1]), _ptr(ed), int(edges.size),
                                             _ptr(hist_d), s))
            mark("triangle_counts")
            hist = hist_d.cpu().numpy()
        tri = out.cpu().numpy()
        bm = binmax.cpu().numpy()
        sm = sums.cpu().numpy()
        if _timings is not None:
            torch.cuda.synchronize(dev)
            for (_, a), (name, b) in zip(ev[:-1], ev[1:]):
                _timings[name] = _timings.get(name, 0.0) + a.elapsed_time(b)
            _timings["batch"] = batch
    if not np.isfinite(bm.view(np.float32)).all() or not np.isfinite(tri).all():
        raise NBEError("bispectrum: the field has voxels that are not finite")
    ntri = np.zeros(T, np.int64)
    if hist is not None:
        cum = np.cumsum(hist)
        ntri = cum[np.searchsorted(edges, hi2[2:])] - cum[np.searchsorted(edges, lo2[2:])]
        ntri = np.where(hi2[2:] > lo2[2:], ntri, 0).astype(np.int64)
    k, pk, _ = _shell_means(bm, sm[:, 0], sm[:, 1], sm[:, 2], par[:, 2], par[:, 3], L, n)
    with np.errstate(invalid="ignore", divide="ignore"):
        B = np.where(ntri > 0, tri * (L ** 6 / float(n) ** 3) / ntri, np.nan)
        Q = B / (pk[0] * pk[1] + pk[1] * pk[2:] + pk[2:] * pk[0])
    return {"theta": th.copy(), "k3": kappa[2:] * kF, "B": B, "Q": Q, "ntriangles": ntri, "pk": pk, "k": k,
            "nmodes": sm[:, 0].astype(np.int64)}


# ---- one-point statistics --------------------------------------------------------------------------------------------

def _onepoint_validate(field, what):
    f = _check_array(field, "field")
    if f.ndim != 3 or min(f.shape) < 1:
        raise ValueError("%s needs a 3-D field, got shape %s" % (what, tuple(f.shape)))
    if _dtype_name(f) != "float32":
        raise ValueError("field must be float32, got %s" % _dtype_name(f))
    count = int(f.shape[0]) * int(f.shape[1]) * int(f.shape[2])
    if count > _ONEPOINT_MAX:
        raise ValueError("%s: %d voxels unsupported (1 .. 2^40)" % (what, count))
    return f, count


def field_statistics(field):
    """Mean, population standard deviation, skewness m3 / sigma^3 and excess kurtosis m4 / sigma^4 - 3 of a field
    (reference scripts/utils.py:1164-1187, _field_moments), with m_p the mean of (x - mean)^p.

    field: any 3-D float32 NumPy array or CUDA tensor.  The sums are float64 on the device, over a partition of the
    voxels that depends on their number only and in a fixed order: the same bits on every call.  Returns a dict of Python
    floats: mean, std, skewness, kurtosis_excess; the last two are 0.0 when std <= 0, as in the reference."""
    f, count = _onepoint_validate(field, "field_statistics")
    dev = _device_of(f)
    l = _lib.lib()
    with torch.cuda.device(dev):
        x = _to_device(f, dev, (torch.float32,))
        mom = torch.empty(_MOMENT4_WORDS, dtype=torch.float64, device=dev)
        _lib.check(l.nbe_field_moments4(_ptr(x), count, _ptr(mom), _stream(dev)))
        mean, std, m3, m4 = (float(v) for v in mom[:4].cpu().numpy())
    skew = m3 / std ** 3 if std > 0 else 0.0
    kurt = m4 / std ** 4 - 3.0 if std > 0 else 0.0
    return {"mean": mean, "std": std, "skewness": skew, "kurtosis_excess": kurt}


def pdf_edges(lo, hi, nbins):
    """The float64 edges np.linspace(lo, hi, nbins + 1) of field_pdf, validated."""
    flo, fhi = _real(lo, "lo"), _real(hi, "hi")
    if isinstance(nbins, (bool, np.bool_)) or not isinstance(nbins, numbers.Integral) or not 2 <= int(nbins) <= _PDF_MAX_BINS:
        raise ValueError("nbins must be an int in 2 .. %d, got %r" % (_PDF_MAX_BINS, nbins))
    if not fhi > flo:
        raise ValueError("hi must exceed lo, got lo %r, hi %r" % (lo, hi))
    edges = np.linspace(flo, fhi, int(nbins) + 1)
    if not (np.diff(edges) > 0).all():
        raise ValueError("lo %r and hi %r are too close for %d distinct float64 edges" % (lo, hi, nbins))
    return edges


def pdf_from_counts(counts, edges):
    """np.histogram's density=True: counts / (counts.sum() * bin width), float64 (NaN when every count is 0)."""
    c = np.asarray(counts, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return c / np.diff(edges) / c.sum()


def field_pdf(field, lo, hi, nbins=120):
    """One-point histogram and PDF of a field, replacing np.histogram(x[np.isfinite(x)], bins=np.linspace(lo, hi,
    nbins + 1), density=True) (reference scripts/utils.py:1248-1274; choosing lo and hi is the caller's business).

    field: any 3-D float32 NumPy array or CUDA tensor.  edges = np.linspace(lo, hi, nbins + 1) in float64, hi > lo,
    2 <= nbins <= 4096.  A voxel x (float32, widened to float64) falls into bin searchsorted(edges, x, "right") - 1, and
    x == hi into the last bin: NumPy's rule, so counts equals np.histogram's.  Returns a dict of host objects: edges,
    centers, pdf (float64), counts (int64), outside (finite voxels beyond the edges) and nonfinite (ints).  pdf = counts /
    (counts.sum() * bin width).  One pass over the field, integer sums: reproducible bit for bit."""
    f, count = _onepoint_validate(field, "field_pdf")
    edges = pdf_edges(lo, hi, nbins)
    nbins = int(nbins)
    dev = _device_of(f)
    l = _lib.lib()
    with torch.cuda.device(dev):
        x = _to_device(f, dev, (torch.float32,))
        ed = torch.from_numpy(edges).to(dev)
        cd = torch.zeros(nbins + 2, dtype=torch.int64, device=dev)
        _lib.check(l.nbe_field_histogram(_ptr(x), count, float(edges[0]), float(edges[-1]), _ptr(ed), nbins, _ptr(cd),
                                         _stream(dev)))
        c = cd.cpu().numpy()
    counts = c[:nbins].copy()
    return {"edges": edges, "centers": 0.5 * (edges[:-1] + edges[1:]), "counts": counts,
            "pdf": pdf_from_counts(counts, edges), "outside": int(c[nbins]), "nonfinite": int(c[nbins + 1])}
