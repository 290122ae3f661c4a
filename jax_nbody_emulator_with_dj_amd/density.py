"""Density fields from emulated displacements, on the GPU: mass assignment, MAS deconvolution, power spectra.

The fork's pipeline turns `process_box`'s displacement into a density field right away (reference
`scripts/core.py:447-458`: `dj.get_delta_from_psi(psi_emu, method="pm", res, worder, deconvolve)`), deconvolves the
assignment window (`scripts/utils.py:136-148`) and measures P(k) (`scripts/utils.py:1083-1085`, Pylians `Pk_library.Pk`).

    from jax_nbody_emulator_with_dj_amd.density import paint_density, deconvolve_mas, power_spectrum

    delta = paint_density(displacement, boxsize=1000.0, res=512, worder=2, deconvolve=True)
    k, pk, nmodes = power_spectrum(delta, boxsize=1000.0)
    k, pk, nmodes = power_spectrum(delta_emu, boxsize=1000.0, other=delta_lpt)     # cross spectrum Re<a b*>
    delta_c = deconvolve_mas(delta, worder=2)
    mf = minkowski_functionals(delta, boxsize=1000.0)    # v0 .. v3 at 41 thresholds of the standardized field

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
- Deconvolution divides the rfft of the mesh by prod_c sinc(k_c L_c / (2 res_c))^worder, sinc(x) = sin(x) / x (the
  window alone, no alias sum).
- `power_spectrum` uses the unnormalised forward FFT: P = |delta_k|^2 L^3 / n^6.  Shell b = 1 .. n/2 holds the modes
  with b - 1/2 <= |k| / k_F < b + 1/2, k_F = 2 pi / L, counted over the full complex grid; it returns the mean |k|, the
  mean P and the number of modes per shell as float64 NumPy arrays.
- `minkowski_functionals` (reference `scripts/utils.py:652-763`) counts the elements of the periodic cubical complex of
  each excursion set {w >= t} in one pass over the field: see its docstring for the definition.

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

__all__ = ["paint_density", "deconvolve_mas", "power_spectrum", "minkowski_functionals"]

WORDERS = {1: "NGP", 2: "CIC", 3: "TSC", 4: "PCS"}
_UNIT = 2.0 ** 22           # fixed-point units per particle mass (include/nbe.h, nbe_paint_mesh)
_KUNIT = 2.0 ** -36         # units of the |k| sums of nbe_power_spectrum
_MF_MAX_N = 2048            # include/nbe.h: NBE_MF_MAX_N, NBE_MF_MAX_THRESHOLDS, NBE_MOMENTS_WORDS
_MF_MAX_T = 1024
_MOMENT_WORDS = 2050
MF_CONVENTION = "periodic_voxel_cubical_complex"


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


def _device():
    """The device for host (NumPy) inputs: cuda:<current>.  Raises NBEError when none is visible (no CPU fallback)."""
    if torch is None or not torch.cuda.is_available():
        raise NBEError("density: no HIP device is visible; this library has no CPU fallback")
    _lib.lib()
    return torch.device("cuda", torch.cuda.current_device())


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


def paint_density(displacement, boxsize=1000.0, res=512, worder=2, deconvolve=True):
    """Mass assignment of the displaced lattice onto a periodic mesh (reference scripts/core.py:449,
    dj.get_delta_from_psi(psi, method="pm", res, worder, deconvolve)).

    displacement: (3, N0, N1, N2) float32 / float16, NumPy array or CUDA torch tensor (process_box's output).
    boxsize: L (scalar or 3-tuple, units of the displacement).  res: mesh size (int or 3-tuple; any value >= 1).
    worder: 1 NGP, 2 CIC, 3 TSC, 4 PCS.  deconvolve: divide by the assignment window (deconvolve_mas).
    Returns delta = rho / rho_mean - 1, float32, shape res; NumPy for NumPy input, a CUDA tensor on the input's device
    for tensor input.  Raises NBEError if a displacement is not finite (those particles could not be painted).
    See the module docstring for the conventions."""
    x, boxsize, res, worder = _validate_paint(displacement, boxsize, res, worder)
    host = not _is_torch(x)
    xd = _to_device(x, _device() if host else x.device, (torch.float32, torch.float16) if torch else ())
    delta, stats = _paint(xd, boxsize, res, worder, bool(deconvolve))
    bad = int(stats[1].item())
    if bad:
        raise NBEError("paint_density: %d particle(s) have a non-finite or out-of-range position" % bad)
    return delta.cpu().numpy() if host else delta


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
    host = not _is_torch(d)
    dd = _to_device(d, _device() if host else d.device, (torch.float32,) if torch else ())
    with torch.cuda.device(dd.device):
        out = _deconvolve(dd, worder)
    return out.cpu().numpy() if host else out


def power_spectrum(delta, boxsize=1000.0, other=None):
    """Shell-averaged power spectrum of a cubic mesh (reference scripts/utils.py:1083-1085, Pylians Pk_library.Pk);
    with `other`, the cross spectrum Re<delta other*>.

    delta / other: (n, n, n) float32, NumPy arrays or CUDA tensors on one device.  boxsize: L (scalar, or a 3-tuple of
    equal values).  Returns (k, pk, nmodes), float64 NumPy arrays of n // 2 shells: the mean |k| (h/Mpc for L in Mpc/h),
    the mean P = |delta_k|^2 L^3 / n^6 and the number of modes of the full complex grid."""
    d = _check_array(delta, "delta")
    L = _triple(boxsize, "boxsize", "a length")
    if d.ndim != 3 or len(set(d.shape)) != 1:
        raise ValueError("power_spectrum needs a cubic mesh, got shape %s" % (tuple(d.shape),))
    if len(set(L)) != 1:
        raise ValueError("power_spectrum needs a cubic box, got boxsize %s" % (L,))
    n = int(d.shape[0])
    if n < 2 or n > 4096:
        raise ValueError("power_spectrum: mesh size %d unsupported (2 .. 4096)" % n)
    if _dtype_name(d) != "float32":
        raise ValueError("delta must be float32, got %s" % _dtype_name(d))
    o = None
    if other is not None:
        o = _check_array(other, "other")
        if tuple(o.shape) != tuple(d.shape) or _dtype_name(o) != "float32":
            raise ValueError("other must match delta: float32 %s, got %s %s"
                             % (tuple(d.shape), _dtype_name(o), tuple(o.shape)))
        if _is_torch(o) != _is_torch(d) or (_is_torch(o) and o.device != d.device):
            raise ValueError("delta and other must both be NumPy arrays or both tensors on one device")
    dev = _device() if not _is_torch(d) else d.device
    l = _lib.lib()
    nb = n // 2 + 1
    with torch.cuda.device(dev):
        a = torch.fft.rfftn(_to_device(d, dev, (torch.float32,))).contiguous()
        b = torch.fft.rfftn(_to_device(o, dev, (torch.float32,))).contiguous() if o is not None else None
        binmax = torch.zeros(nb, dtype=torch.int32, device=dev)
        sums = torch.zeros(3 * nb, dtype=torch.int64, device=dev)
        _lib.check(l.nbe_power_spectrum(_ptr(a), _ptr(b) if b is not None else None, n, _ptr(binmax), _ptr(sums),
                                        _stream(dev)))
        bm = binmax.cpu().numpy().view(np.float32).astype(np.float64)[1:]
        sm = sums.cpu().numpy().reshape(3, nb)[:, 1:]
    cnt = sm[0].astype(np.float64)
    shell = np.arange(1, nb, dtype=np.float64)
    kF = 2.0 * np.pi / L[0]
    _, e = np.frexp(np.where(np.isfinite(bm), bm, 1.0))
    with np.errstate(invalid="ignore", divide="ignore"):
        k = (shell + sm[1].astype(np.float64) * _KUNIT / cnt) * kF
        pk = np.ldexp(sm[2].astype(np.float64), e - 32) / cnt * (L[0] ** 3 / float(n) ** 6)
    pk = np.where(np.isfinite(bm), pk, np.nan)
    return k, pk, cnt


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
    f = _check_array(field, "field")
    if f.ndim != 3 or len(set(f.shape)) != 1:
        raise ValueError("minkowski_functionals needs a cubic (n, n, n) field, got shape %s" % (tuple(f.shape),))
    n = int(f.shape[0])
    if not 1 <= n <= _MF_MAX_N:
        raise ValueError("minkowski_functionals: mesh size %d unsupported (1 .. %d)" % (n, _MF_MAX_N))
    if _dtype_name(f) != "float32":
        raise ValueError("field must be float32, got %s" % _dtype_name(f))
    L = _triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("minkowski_functionals needs a cubic box, got boxsize %s" % (L,))
    return f, n, L[0], _mf_thresholds(thresholds)


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
    host = not _is_torch(f)
    dev = _device() if host else f.device
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
