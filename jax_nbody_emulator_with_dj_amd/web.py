"""Where in the cosmic web a voxel sits, on the GPU: the tidal tensor or the velocity shear of a smoothed mesh, its
eigenvalues per voxel, and the classification into voids, sheets, filaments and knots with their volume and mass fractions.

The reference's pipeline has no such step.  These stand in for the T-web of Hahn et al. (2007) with the free threshold of
Forero-Romero et al. (2009), and for the V-web of Hoffman et al. (2012), as their authors' codes run them on a mesh.

    from jax_nbody_emulator_with_dj_amd.web import cosmic_web, tidal_tensor, tensor_eigenvalues, classify_web

    web = cosmic_web(delta, boxsize=1000.0, smoothing=4.0, threshold=[0.0, 0.2, 0.4], mass=delta)
    web["types"]                # (n, n, n) uint8: 0 void, 1 sheet, 2 filament, 3 knot under threshold[0]; 255 without a type
    web["volume_fraction"]      # (3, 4) float64, web["mass_fraction"] likewise
    vweb = cosmic_web(delta, 1000.0, 4.0, threshold=0.44, kind="shear", vmesh=v, scale=1.0 / H0)
    eig = tensor_eigenvalues(tidal_tensor(delta, 1000.0, smoothing=4.0))          # the steps one by one

Definitions:

- The tidal tensor is T_ij = phi,ij with nabla^2 phi = delta, so its trace is delta (dimensionless; the box size enters
  through the smoothing length only): lpt.lpt2_source's Hessian, with its Nyquist rule.  The velocity shear is
  Sigma_ij = -scale (d_i v_j + d_j v_i) / 2 with lpt.divergence's derivative, so its trace is -scale div v; Hoffman et al.
  take scale = 1 / H0, which makes it dimensionless and equal to the tidal tensor in linear theory up to the growth rate.
- Components are in the pair order (0,0), (1,1), (2,2), (0,1), (0,2), (1,2).  `smoothing` is the standard deviation of a
  Gaussian, in the unit of boxsize (lpt.gaussian_smooth).
- Eigenvalues are lambda_1 >= lambda_2 >= lambda_3 per voxel, computed in float64 from the float32 tensor and rounded once.
- A voxel's type under a threshold is the number of its eigenvalues above it, compared as float32.  A voxel with a NaN
  eigenvalue has no type: it gets 255 and is counted in counts[t][4].

Residency as in lpt: NumPy in, NumPy out; CUDA tensors in, CUDA tensors out on the same device and torch's current stream.
The small tables (thresholds, counts, fractions) are NumPy always.  No CPU fallback; arguments are validated first.
"""

import ctypes as C
import numbers

import numpy as np

from . import _lib
from .density import (_back, _bk_batch, _check_array, _check_max_blocks, _cubic, _device_of, _dtype_name, _ptr, _real,
                      _same_kind, _stream, _to_device, _triple)
from .lpt import COMPONENTS, MAX_N, MIN_N, _empty_spectrum, _flag, _half_spectrum, _real_field

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["tidal_tensor", "velocity_shear", "tensor_eigenvalues", "classify_web", "cosmic_web"]

MAX_THRESHOLDS = 64                     # include/nbe.h: NBE_WEB_MAX_THRESHOLDS
TYPE_NAMES = ("void", "sheet", "filament", "knot")
NO_TYPE = 255                           # `types` of a voxel with a NaN eigenvalue
KINDS = ("tidal", "shear")


# ---- validation (no device) ------------------------------------------------------------------------------------------------

def _smoothing(v):
    return None if v is None else _real(v, "smoothing", positive=True)


def _stack(x, name, lead, what):
    """A (lead, n, n, n) float32 stack of cubic meshes: (array, n)."""
    x = _check_array(x, name)
    if x.ndim != 4 or x.shape[0] != lead or len(set(x.shape[1:])) != 1:
        raise ValueError("%s needs a (%d, n, n, n) %s, got shape %s" % (what, lead, name, tuple(x.shape)))
    n = int(x.shape[1])
    if not MIN_N <= n <= MAX_N:
        raise ValueError("%s: mesh size %d unsupported (%d .. %d)" % (what, n, MIN_N, MAX_N))
    if _dtype_name(x) != "float32":
        raise ValueError("%s must be float32, got %s" % (name, _dtype_name(x)))
    return x, n


def _cubic_box(boxsize, what):
    L = _triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("%s needs a cubic box, got boxsize %s" % (what, L))
    return L[0]


def _thresholds(threshold):
    """threshold as a float32 array of 1 .. 64 finite values."""
    vals = list(np.asarray(threshold).ravel()) if isinstance(threshold, (tuple, list, np.ndarray)) else [threshold]
    if not 1 <= len(vals) <= MAX_THRESHOLDS:
        raise ValueError("threshold must be a number or 1 .. %d numbers, got %d" % (MAX_THRESHOLDS, len(vals)))
    vals = [_real(v.item() if isinstance(v, np.generic) else v, "threshold") for v in vals]
    with np.errstate(over="ignore"):
        out = np.array(vals, dtype=np.float32)
    if not np.isfinite(out).all():
        raise ValueError("threshold must be finite in float32, got %r" % (threshold,))
    return out


def _which(which, T):
    if isinstance(which, (bool, np.bool_)) or not isinstance(which, numbers.Integral) or not 0 <= int(which) < T:
        raise ValueError("which must be an int in 0 .. %d, got %r" % (T - 1, which))
    return int(which)


# ---- device work -----------------------------------------------------------------------------------------------------------

def _filtered(spec, n, sigma_over_L):
    """In place: nbe_gaussian_filter on a half spectrum or on each of a stack of them."""
    if sigma_over_L is not None:
        for s in (spec if spec.dim() == 4 else (spec,)):
            _lib.check(_lib.lib().nbe_gaussian_filter(_ptr(s), n, sigma_over_L, _stream(spec.device)))
    return spec


def _tensor_field(spec, n, L, scale, max_batch, max_blocks=0):
    """The six real fields (6, n, n, n) of a half spectrum (the tidal tensor: nbe_lpt2_hessian_spectrum) or of three (the
    shear: nbe_shear_spectrum), `_bk_batch` components at a time as lpt._source_field makes them: pieces give the bits of
    the whole."""
    dev = spec.device
    l = _lib.lib()
    out = torch.empty((COMPONENTS, n, n, n), dtype=torch.float32, device=dev)
    batch = _bk_batch(dev, n, COMPONENTS, max_batch)
    for first in range(0, COMPONENTS, batch):
        count = min(batch, COMPONENTS - first)
        tk = _empty_spectrum(n, dev, (count,))
        if spec.dim() == 3:
            _lib.check(l.nbe_lpt2_hessian_spectrum(_ptr(spec), n, first, count, _ptr(tk), max_blocks, _stream(dev)))
        else:
            _lib.check(l.nbe_shear_spectrum(_ptr(spec), n, L, scale, first, count, _ptr(tk), max_blocks, _stream(dev)))
        # a batch through dim=(1, 2, 3) whatever its length: see lpt._inverse_components
        out[first:first + count] = torch.fft.irfftn(tk, s=(n, n, n), dim=(1, 2, 3))
        del tk
    return out


def _eigenvalues(t, n, max_blocks=0):
    eig = torch.empty((3, n, n, n), dtype=torch.float32, device=t.device)
    _lib.check(_lib.lib().nbe_tensor_eigenvalues(_ptr(t), n, _ptr(eig), max_blocks, _stream(t.device)))
    return eig


def _classify(eig, n, th, which, want_types, max_blocks=0):
    """(counts (T, 5) int64 on the host, types tensor or None)"""
    dev = eig.device
    counts = torch.zeros((len(th), 5), dtype=torch.int64, device=dev)
    types = torch.empty((n, n, n), dtype=torch.uint8, device=dev) if want_types else None
    tharr = (C.c_float * len(th))(*[float(v) for v in th])
    _lib.check(_lib.lib().nbe_web_classify(_ptr(eig), n, tharr, len(th), which, _ptr(types) if want_types else None,
                                           _ptr(counts), max_blocks, _stream(dev)))
    return counts.cpu().numpy(), types


def _fractions(counts, n):
    return counts[:, :4].astype(np.float64) / float(n) ** 3


def _mass_fraction(eig, n, th, mass, max_blocks=0):
    """(T, 4) float64: the sum of 1 + delta over the voxels of each type, over its sum over all voxels."""
    w = mass.to(torch.float64) + 1.0
    total = w.sum()
    out = np.zeros((len(th), 4), np.float64)
    for t in range(len(th)):
        _, types = _classify(eig, n, th, t, True, max_blocks)
        sums = torch.stack([torch.where(types == m, w, torch.zeros_like(w)).sum() for m in range(4)])
        out[t] = (sums / total).cpu().numpy()
    return out


# ---- public ----------------------------------------------------------------------------------------------------------------

def tidal_tensor(delta, boxsize=1000.0, smoothing=None, _max_batch=None, _max_blocks=None):
    """The tidal tensor T_ij = phi,ij of a density contrast, nabla^2 phi = delta, on its mesh (the T-web's tensor, Hahn et
    al. 2007): (6, n, n, n) float32 in the pair order (0,0), (1,1), (2,2), (0,1), (0,2), (1,2), of the input's kind.

    delta: cubic (n, n, n) float32, NumPy array or CUDA tensor, 2 <= n <= 2048.  smoothing: None, or the standard deviation
    of the Gaussian the field is smoothed with first, in the unit of boxsize (lpt.gaussian_smooth).  T_ij_k =
    d_i d_j / |m|^2 delta_k with lpt.lpt2_source's derivative numbers, 0 at m = 0: the trace is delta less its mean.

    One rfftn, the filter, the Hessian pass in pieces sized by the free memory, one batched irfftn per piece."""
    d, n, L = _cubic(delta, "delta", boxsize, "tidal_tensor", "(n, n, n) field", MIN_N, MAX_N)
    sigma, blocks = _smoothing(smoothing), _check_max_blocks(_max_blocks, "tidal_tensor")
    dev = _device_of(d)
    with torch.cuda.device(dev):
        spec = _filtered(_half_spectrum(_to_device(d, dev, (torch.float32,))), n, None if sigma is None else sigma / L)
        return _back(d, _tensor_field(spec, n, L, 1.0, _max_batch, blocks))


def velocity_shear(vmesh, boxsize=1000.0, scale=1.0, smoothing=None, _max_batch=None, _max_blocks=None):
    """The velocity shear Sigma_ij = -scale (d_i v_j + d_j v_i) / 2 of a vector mesh (the V-web's tensor, Hoffman et al.
    2012, who take scale = 1 / H0): (6, n, n, n) float32 in tidal_tensor's order, of the input's kind.

    vmesh: (3, n, n, n) float32, component c along array axis c (density.paint_field's mass-weighted velocity, say).  The
    derivative is lpt.divergence's, so the trace is -scale * lpt.divergence(vmesh, boxsize) to rounding.  smoothing as in
    tidal_tensor, applied to every component.

    One batched rfftn, the filter, nbe_shear_spectrum in pieces, one batched irfftn per piece."""
    v, n = _stack(vmesh, "vmesh", 3, "velocity_shear")
    L, scale, sigma = _cubic_box(boxsize, "velocity_shear"), _real(scale, "scale"), _smoothing(smoothing)
    blocks = _check_max_blocks(_max_blocks, "velocity_shear")
    dev = _device_of(v)
    with torch.cuda.device(dev):
        spec = torch.fft.rfftn(_to_device(v, dev, (torch.float32,)), dim=(1, 2, 3)).contiguous()
        _filtered(spec, n, None if sigma is None else sigma / L)
        return _back(v, _tensor_field(spec, n, L, scale, _max_batch, blocks))


def tensor_eigenvalues(tensor, _max_blocks=None):
    """The eigenvalues lambda_1 >= lambda_2 >= lambda_3 of a symmetric 3x3 tensor field, per voxel: tensor (6, n, n, n)
    float32 in tidal_tensor's order, returns (3, n, n, n) float32 of the input's kind.

    Computed in float64 from the six float32 words and rounded once; the error of the float64 step stays below 0.14 of one
    float32 rounding of the tensor's Frobenius norm, so |lambda - exact| <= 2^-23 |A|_F.  Where the off-diagonal words are
    exactly 0 the result is the sorted diagonal, bit for bit.  A voxel with a non-finite word gives three NaNs."""
    t, n = _stack(tensor, "tensor", COMPONENTS, "tensor_eigenvalues")
    blocks = _check_max_blocks(_max_blocks, "tensor_eigenvalues")
    dev = _device_of(t)
    with torch.cuda.device(dev):
        return _back(t, _eigenvalues(_to_device(t, dev, (torch.float32,)), n, blocks))


def classify_web(eig, threshold=0.0, return_types=True, which=0, _max_blocks=None):
    """Voids, sheets, filaments and knots from the eigenvalues of a tensor field: a voxel's type is the number of its
    eigenvalues above the threshold (0 .. 3), compared as float32.

    eig: (3, n, n, n) float32 (tensor_eigenvalues; the order of the three does not matter).  threshold: a number or up to
    64 of them, a scan of lambda_th in one read of eig.  Returns a dict: thresholds (T,) float32, counts (T, 5) int64 --
    counts[t][m] voxels of type m under thresholds[t], counts[t][4] voxels with a NaN eigenvalue, which have no type --,
    volume_fraction (T, 4) float64 = counts[:, :4] / n^3, which sums to 1 less the share without a type, and with
    return_types types (n, n, n) uint8 of the input's kind under thresholds[which], 255 where there is no type."""
    e, n = _stack(eig, "eig", 3, "classify_web")
    th = _thresholds(threshold)
    which, want = _which(which, len(th)), _flag(return_types, "return_types")
    blocks = _check_max_blocks(_max_blocks, "classify_web")
    dev = _device_of(e)
    with torch.cuda.device(dev):
        counts, types = _classify(_to_device(e, dev, (torch.float32,)), n, th, which, want, blocks)
    out = {"thresholds": th, "counts": counts, "volume_fraction": _fractions(counts, n)}
    if want:
        out["types"] = _back(e, types)
    return out


def _validate_web(delta, boxsize, smoothing, threshold, kind, vmesh, scale, mass, what):
    d, n, L = _cubic(delta, "delta", boxsize, what, "(n, n, n) field", MIN_N, MAX_N)
    sigma, th = _smoothing(smoothing), _thresholds(threshold)
    if kind not in KINDS:
        raise ValueError("kind must be 'tidal' or 'shear', got %r" % (kind,))
    v = None
    if kind == "shear":
        if vmesh is None:
            raise ValueError("%s: kind='shear' needs vmesh, the (3, n, n, n) velocity mesh" % what)
        v, nv = _stack(vmesh, "vmesh", 3, what)
        if nv != n:
            raise ValueError("vmesh must have the mesh size %d of delta, got %d" % (n, nv))
        _same_kind(d, v, "delta", "vmesh")
    elif vmesh is not None:
        raise ValueError("%s: vmesh is read with kind='shear' only" % what)
    scale = _real(scale, "scale")
    m = None
    if mass is not None:
        m, nm, _ = _cubic(mass, "mass", boxsize, what, "(n, n, n) field", MIN_N, MAX_N)
        if nm != n:
            raise ValueError("mass must have the mesh size %d of delta, got %d" % (n, nm))
        _same_kind(d, m, "delta", "mass")
    return d, n, L, sigma, th, v, scale, m


def _web(dd, n, L, sigma, th, vd, scale, md, max_batch=None, blocks=0, want_smooth=False):
    """Device work of cosmic_web: dd, vd, md contiguous float32 tensors (vd, md or None).  Returns (eig, counts, types,
    mass_fraction or None, smoothed delta or None)."""
    so = None if sigma is None else sigma / L
    smooth = None
    if vd is None or want_smooth:
        dk = _filtered(_half_spectrum(dd), n, so)
    if vd is None:
        tensor = _tensor_field(dk, n, L, 1.0, max_batch, blocks)
    else:
        vk = _filtered(torch.fft.rfftn(vd, dim=(1, 2, 3)).contiguous(), n, so)
        tensor = _tensor_field(vk, n, L, scale, max_batch, blocks)
        del vk
    if want_smooth:
        smooth = _real_field(dk, n)
    eig = _eigenvalues(tensor, n, blocks)
    del tensor
    counts, types = _classify(eig, n, th, 0, True, blocks)
    mf = _mass_fraction(eig, n, th, md, blocks) if md is not None else None
    return eig, counts, types, mf, smooth


def cosmic_web(delta, boxsize=1000.0, smoothing=None, threshold=0.0, kind="tidal", vmesh=None, scale=1.0, mass=None,
               _max_batch=None, _max_blocks=None):
    """The cosmic web of a mesh in one call: tidal_tensor(delta, boxsize, smoothing), or with kind="shear"
    velocity_shear(vmesh, boxsize, scale, smoothing), then tensor_eigenvalues and classify_web(eig, threshold).

    delta: cubic (n, n, n) float32 density contrast (with kind="shear" it gives the mesh size and the kind of the result
    only).  smoothing: the Gaussian's standard deviation in the unit of boxsize, or None.  threshold: a number or up to
    64.  mass: None, or a density contrast of the same n (usually the unsmoothed one): the call then adds mass_fraction.

    Returns a dict: eigenvalues (3, n, n, n) float32 and types (n, n, n) uint8 under thresholds[0], of the input's kind;
    thresholds, counts (T, 5) and volume_fraction (T, 4) as classify_web; smoothing (float, or nan for None); and with
    mass mass_fraction (T, 4) float64: the sum of 1 + mass over the voxels of each type, in float64, over its sum over all
    voxels (so the rows sum to 1 less the mass share of the voxels without a type)."""
    d, n, L, sigma, th, v, scale, m = _validate_web(delta, boxsize, smoothing, threshold, kind, vmesh, scale, mass,
                                                    "cosmic_web")
    blocks = _check_max_blocks(_max_blocks, "cosmic_web")
    dev = _device_of(d)
    with torch.cuda.device(dev):
        f32 = (torch.float32,)
        eig, counts, types, mf, _ = _web(_to_device(d, dev, f32), n, L, sigma, th,
                                         None if v is None else _to_device(v, dev, f32), scale,
                                         None if m is None else _to_device(m, dev, f32), _max_batch, blocks)
    out = {"eigenvalues": _back(d, eig), "types": _back(d, types), "thresholds": th, "counts": counts,
           "volume_fraction": _fractions(counts, n), "smoothing": float("nan") if sigma is None else sigma}
    if mf is not None:
        out["mass_fraction"] = mf
    return out
