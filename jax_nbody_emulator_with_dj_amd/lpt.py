"""The emulator's input, on the GPU: a linear density field brought to the particle grid and turned into the first-order
LPT displacement that `process_box` reads.

The reference's pipeline does this before `process_box` with DISCO-DJ, JAX and Pylians (`scripts/core.py:302-409`:
`resize_density_grid`, `scripts/utils.py:186-234`, `:261-425`, `:531-592`; `dj.evaluate_lpt_psi_at_a(n_order=1)`).

    from jax_nbody_emulator_with_dj_amd.lpt import zeldovich_displacement, resize_density, gaussian_smooth, divergence

    delta512 = resize_density(delta256, 512, boxsize=1000.0, upsample_method="fourier")
    psi = zeldovich_displacement(delta512, boxsize=1000.0)                 # (3, 512, 512, 512), process_box's input
    delta128 = resize_density(delta256, 128, boxsize=1000.0, upsample_method="fourier", downsample_method="gaussian")
    smooth = gaussian_smooth(delta256, boxsize=1000.0, sigma=8.0)
    theta = divergence(vmesh, boxsize=1000.0)                              # (3, n, n, n) -> (n, n, n)

Conventions:

- Fields are cubic (n, n, n) float32 in a cubic periodic box of side `boxsize`, 2 <= n <= 2048.  Transforms are rocFFT's
  through torch.fft (unnormalised forward); a mode has the integer wave vector m, k = 2 pi m / L.
- `zeldovich_displacement` returns psi with psi_k = scale i k / |k|^2 delta_k, so that div psi = -scale delta: particles
  move towards overdensities, the sign of DISCO-DJ's and of the emulator's input.  psi_k is 0 at k = 0.  Where n is even,
  component c is 0 on the Nyquist row |m_c| = n/2, which has no sign.
- "fourier" resizing keeps every mode both grids hold, times (n_out / n_in)^3.  Upwards an even coarse Nyquist row is
  split evenly onto +-n_in/2; downwards a fine Nyquist component is the sum of the source at both signs.  So an upsampled
  field equals its input at the coarse nodes, and down(up(x)) = x.
- "mode_inject" keeps the modes inside the sphere |m| <= n_in/2 and draws the others from a tabulated P(k) with a
  counter-based generator: `inject_spectrum` has the definition.

- `gaussian_field`, `white_noise`, `colour_noise` and `linear_ics` make the linear field itself from a seed and a tabulated
  P(k), one seed being one universe at every resolution: `gaussian_spectrum` has the definition.

    delta, psi = linear_ics(512, 1000.0, k, pk, seed=7, scale=D)          # seed -> delta, process_box's input
    delta = gaussian_field(512, 1000.0, k, pk, seed=7)                    # the field alone: one draw pass, one irfftn
    delta = colour_noise(white, 1000.0, k, pk)                            # somebody else's white noise, coloured

- `lpt2_displacement` and `lpt2_source` add the second order: the initial condition of an N-body
  run and the stronger baseline beside an emulated box.  The emulator's own input stays first order.

    psi2lpt = lpt2_displacement(delta512, boxsize=1000.0, scale=D, growth2=3 / 7, dealias=True)
    delta, psi1, psi2lpt = linear_ics(512, 1000.0, k, pk, seed=7, scale=D, order=2)

Residency: NumPy in gives NumPy out; a CUDA torch tensor in gives a CUDA tensor on the same device, with no host copy,
enqueued on torch's current stream of that device.  There is no CPU fallback: without a device the first device call
raises NBEError.  Arguments are validated before any device work.
"""

import numbers

import numpy as np

from . import _lib
from . import density
from .density import _back, _bk_batch, _check_array, _cubic, _device_of, _ptr, _real, _stream, _to_device

try:
    import torch
except Exception:  # pragma: no cover
    torch = None

__all__ = ["zeldovich_displacement", "resize_density", "gaussian_smooth"]

MIN_N, MAX_N = 2, 2048                  # include/nbe.h: NBE_LPT_MIN_N, NBE_LPT_MAX_N
UPSAMPLE_METHODS = ("fourier", "linear", "mode_inject")
DOWNSAMPLE_METHODS = ("gaussian", "block_average", "fourier")
_TAIL_POINTS = 8                        # reference scripts/utils.py:307: the log-log tail is fitted to the last 8 points


def _field(delta, boxsize, what):
    return _cubic(delta, "delta", boxsize, what, "(n, n, n) field", MIN_N, MAX_N)


def _size(v, name):
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or not MIN_N <= int(v) <= MAX_N:
        raise ValueError("%s must be an int in %d .. %d, got %r" % (name, MIN_N, MAX_N, v))
    return int(v)


def _half_spectrum(x):
    return torch.fft.rfftn(x).contiguous()               # the kernels index the half spectrum row-major


def _real_field(spec, n):
    return torch.fft.irfftn(spec, s=(n, n, n)).contiguous()


def _empty_spectrum(n, dev, lead=()):
    return torch.empty(tuple(lead) + (n, n, n // 2 + 1), dtype=torch.complex64, device=dev)


# ---- first-order LPT -----------------------------------------------------------------------------------------------------

def zeldovich_displacement(delta, boxsize=1000.0, scale=1.0, _max_batch=None):
    """First-order LPT (Zel'dovich) displacement of a linear density field (reference scripts/core.py:396-397,
    dj.with_lpt(n_order=1) / dj.evaluate_lpt_psi_at_a(a, n_order=1), the order the reference uses; second order is
    `lpt2_displacement`).

    delta: cubic (n, n, n) float32, NumPy array or CUDA tensor, 2 <= n <= 2048.  boxsize: L (scalar, or a 3-tuple of equal
    values), the unit of the result.  Returns psi, (3, n, n, n) float32, channel c along array axis c: valid input to
    process_box as it stands.

    Sign convention: psi_k = scale i k / |k|^2 delta_k with k = 2 pi m / L, so that div psi = -scale delta and particles
    move towards overdensities.  `scale` carries the growth factor for a field given at another epoch: for delta
    normalised at a_0 and an emulator input at a, scale = D(a) / D(a_0) (cosmology.growth_factor); a negative or zero
    scale is taken as given.  DISCO-DJ cannot be imported where this library is developed, so its normalisation of the
    external field is not pinned; the definition above is what is computed.  psi_k = 0 at k = 0, and where n is even
    component c is 0 on the row |m_c| = n/2: a Nyquist row has no sign, so its derivative is set to zero and the field
    stays real.

    One rfftn, one pass that reads delta_k once and writes the three spectra, and one batched irfftn over the three
    components; where memory is short the components are transformed one at a time (the same bits)."""
    d, n, L = _field(delta, boxsize, "zeldovich_displacement")
    scale = _real(scale, "scale")
    dev = _device_of(d)
    with torch.cuda.device(dev):
        spec = _half_spectrum(_to_device(d, dev, (torch.float32,)))
        psi_k = _psi_spectrum(spec, n, L, scale)
        del spec
        psi = _inverse_components(psi_k, n, _max_batch)
    return _back(d, psi)


def _psi_spectrum(spec, n, L, scale):
    """nbe_zeldovich_spectrum on a contiguous complex64 half spectrum on the device: (3, n, n, n // 2 + 1)."""
    psi_k = _empty_spectrum(n, spec.device, (3,))
    _lib.check(_lib.lib().nbe_zeldovich_spectrum(_ptr(spec), n, L, scale, _ptr(psi_k), _stream(spec.device)))
    return psi_k


def _inverse_components(psi_k, n, max_batch):
    """The (3, n, n, n) float32 field of three half spectra: one batched irfftn, or one component at a time where
    `_bk_batch` finds memory short (the same bits)."""
    dev = psi_k.device
    if _bk_batch(dev, n, 3, max_batch) >= 3:
        return torch.fft.irfftn(psi_k, s=(n, n, n), dim=(1, 2, 3)).contiguous()
    psi = torch.empty((3, n, n, n), dtype=torch.float32, device=dev)
    # A batch of one through the same call: torch gives a transform with a leading batch axis to one 3-D
    # complex-to-real plan, and a bare 3-D tensor to a 2-D complex plan plus 1-D real ones, which rounds differently.
    for c in range(3):
        psi[c:c + 1] = torch.fft.irfftn(psi_k[c:c + 1], s=(n, n, n), dim=(1, 2, 3))
    return psi


def divergence(field, boxsize=1000.0):
    """theta = div v of a vector field on a periodic grid, by the spectral derivative: what turns the mass-weighted
    velocity mesh of density.paint_field into the field whose spectra P_theta-theta = power_spectrum(theta) and
    P_delta-theta = power_spectrum(delta, other=theta) check an emulated velocity (the reference's pipeline has no such
    step).

    field: (3, n, n, n) float32, component c along array axis c, NumPy array or CUDA tensor, 2 <= n <= 2048.  boxsize: L
    (scalar, or a 3-tuple of equal values); theta is in the field's unit per unit of L.  Returns (n, n, n) float32 of the
    input's kind.

    theta_k = i (2 pi / L) ((m_0 v_0 + m_1 v_1) + m_2 v_2), added in float64 in that order, each word rounded to float32
    once.  Where n is even, component c contributes nothing on its own Nyquist row |m_c| = n/2, as in
    `zeldovich_displacement`: the row has no sign, the field stays real and the axes are treated alike.  So
    divergence(zeldovich_displacement(x)) = -x for an x without power on those rows.

    One batched rfftn over the three components, one pass that reads them once, one irfftn."""
    f = _check_array(field, "field")
    if f.ndim != 4 or f.shape[0] != 3 or len(set(f.shape[1:])) != 1:
        raise ValueError("divergence needs a (3, n, n, n) field, got shape %s" % (tuple(f.shape),))
    _, n, L = _cubic(f[0], "field", boxsize, "divergence", "(3, n, n, n) field", MIN_N, MAX_N)
    dev = _device_of(f)
    with torch.cuda.device(dev):
        spec = torch.fft.rfftn(_to_device(f, dev, (torch.float32,)), dim=(1, 2, 3)).contiguous()
        theta_k = _empty_spectrum(n, dev)
        _lib.check(_lib.lib().nbe_divergence_spectrum(_ptr(spec), n, L, _ptr(theta_k), _stream(dev)))
        del spec
        theta = _real_field(theta_k, n)
    return _back(f, theta)


# ---- second-order LPT ------------------------------------------------------------------------------------------------------

COMPONENTS = 6                          # include/nbe.h: NBE_LPT2_COMPONENTS, the pairs (0,0) (1,1) (2,2) (0,1) (0,2) (1,2)
EDS_GROWTH2 = 3.0 / 7.0                 # -D_2 / D_1^2 in an Einstein-de Sitter universe


def _dealias_size(n, dealias, what):
    """The mesh the quadratic source is formed on: n, or 3 n / 2 with `dealias` (a bool), which needs an even n."""
    if not _flag(dealias, "dealias"):
        return n
    if n % 2 or 3 * n // 2 > MAX_N:
        raise ValueError("%s: dealias=True needs an even n with 3 n / 2 <= %d, got %d" % (what, MAX_N, n))
    return 3 * n // 2


def _validate_lpt2(delta, boxsize, scale, growth2, dealias, what):
    d, n, L = _field(delta, boxsize, what)
    return d, n, L, _real(scale, "scale"), _real(growth2, "growth2"), _dealias_size(n, dealias, what)


def _lpt2_budget(dev, n, p, what):
    """NBEError where the six real fields on the p^3 mesh, the source, one transform in flight and the spectra at n do not
    fit the free memory of the device."""
    need = (COMPONENTS + 1) * 4 * p ** 3 + 16 * (p ** 3 + 2 * p * p) + 5 * 4 * (n ** 3 + 2 * n * n)
    density._check_free_memory(dev, need, "%s: the six Hessian fields of %d^3" % (what, p),
                               "%d fields of 4 n^3 bytes and one transform" % (COMPONENTS + 1))


def _source_field(spec, n, p, max_batch, max_blocks=0):
    """The real source S (p, p, p) of the half spectrum `spec` of an n^3 field: the Hessian spectra `_bk_batch` at a time
    (nbe_lpt2_hessian_spectrum), each brought to p >= n by nbe_spectrum_resize, one batched irfftn per piece, and
    nbe_lpt2_source over the six real fields.  Pieces give the bits of the whole."""
    dev = spec.device
    l = _lib.lib()
    hess = torch.empty((COMPONENTS, p, p, p), dtype=torch.float32, device=dev)
    batch = _bk_batch(dev, p, COMPONENTS, max_batch)
    for first in range(0, COMPONENTS, batch):
        count = min(batch, COMPONENTS - first)
        hk = _empty_spectrum(n, dev, (count,))
        _lib.check(l.nbe_lpt2_hessian_spectrum(_ptr(spec), n, first, count, _ptr(hk), max_blocks, _stream(dev)))
        if p != n:
            up = _empty_spectrum(p, dev, (count,))
            for c in range(count):
                _lib.check(l.nbe_spectrum_resize(_ptr(hk[c]), n, _ptr(up[c]), p, 0, _stream(dev)))
            hk = up
            del up
        # a batch through dim=(1, 2, 3) whatever its length: see _inverse_components
        hess[first:first + count] = torch.fft.irfftn(hk, s=(p, p, p), dim=(1, 2, 3))
        del hk
    out = torch.empty((p, p, p), dtype=torch.float32, device=dev)
    _lib.check(l.nbe_lpt2_source(_ptr(hess), p, _ptr(out), max_blocks, _stream(dev)))
    return out


def _source_spectrum(spec, n, p, max_batch):
    """The half spectrum (n, n, n // 2 + 1) of the source of `spec`, formed on the p^3 mesh and brought back to n."""
    s_k = _half_spectrum(_source_field(spec, n, p, max_batch))
    return s_k if p == n else _resize_spectrum(s_k, p, n)


def _psi2_spectrum(spec, s_k, n, L, a, b, max_blocks=0):
    """nbe_lpt2_spectrum on two contiguous complex64 half spectra on the device: (3, n, n, n // 2 + 1)."""
    psi_k = _empty_spectrum(n, spec.device, (3,))
    _lib.check(_lib.lib().nbe_lpt2_spectrum(_ptr(spec), _ptr(s_k), n, L, a, b, _ptr(psi_k), max_blocks,
                                            _stream(spec.device)))
    return psi_k


def lpt2_source(delta, dealias=False, _max_batch=None):
    """The source of the second-order LPT displacement, S = sum over i < j of (phi,ii phi,jj - phi,ij^2) with
    nabla^2 phi = delta: the sum of the principal 2x2 minors of the Hessian of the first-order potential (DISCO-DJ's
    n_order=2).  S is dimensionless and does not depend on the box size.

    delta: cubic (n, n, n) float32, NumPy array or CUDA tensor, 2 <= n <= 2048.  Returns S, (n, n, n) float32 of the
    input's kind.

    phi,ij_k = d_i d_j / |m|^2 delta_k with d_c = m_c, or 0 where n is even and |m_c| = n/2 (the Nyquist rule of
    `zeldovich_displacement`, once per factor, so phi,ij = -d_j psi_i in this module's own derivative); 0 at m = 0.  S is
    formed per voxel in float64 as ((h0 h1 + h0 h2) + h1 h2) - ((h3^2 + h4^2) + h5^2) over the six fields in the order
    (0,0), (1,1), (2,2), (0,1), (0,2), (1,2), and rounded once.  A plane wave has S = 0, and the mean of S is 0.

    dealias=True (n even, 3 n / 2 <= 2048) forms the product on the mesh of 3 n / 2 points a side (the 3/2 rule): each
    Hessian spectrum is Fourier-interpolated upwards, S is formed there, transformed, and brought back to n by the
    "fourier" downsampling of `resize_density`.  Every mode of the result is then free of aliasing except those on the
    Nyquist rows |m_c| = n/2 of the (even) n, which the downsampling sums over both signs.

    One rfftn, six inverse transforms (batched as the free memory allows, the same bits), one real-space pass; with
    dealias two resizing passes per field and two more transforms."""
    d, n, L, _, _, p = _validate_lpt2(delta, 1.0, 1.0, EDS_GROWTH2, dealias, "lpt2_source")
    dev = _device_of(d)
    with torch.cuda.device(dev):
        _lpt2_budget(dev, n, p, "lpt2_source")
        spec = _half_spectrum(_to_device(d, dev, (torch.float32,)))
        if p == n:
            return _back(d, _source_field(spec, n, n, _max_batch))
        return _back(d, _real_field(_source_spectrum(spec, n, p, _max_batch), n))


def lpt2_displacement(delta, boxsize=1000.0, scale=1.0, growth2=EDS_GROWTH2, dealias=False, return_orders=False,
                      _max_batch=None):
    """Second-order LPT displacement of a linear density field: psi = psi1 + psi2, what DISCO-DJ's
    evaluate_lpt_psi_at_a(a, n_order=2) returns where the reference asks for n_order=1 (scripts/core.py:396-397).  The
    standard initial condition of an N-body run, and the stronger analytic baseline beside an emulated box; the emulator's
    own input stays `zeldovich_displacement`.

    delta, boxsize, and the result (3, n, n, n) float32 as in `zeldovich_displacement`.  With a = scale and
    b = growth2 scale^2,

        psi_k = i k / |k|^2 (a delta_k + b S_k),   S = lpt2_source(delta, dealias),

    so psi1 = `zeldovich_displacement(delta, boxsize, scale)` up to rounding and div psi2 = -b S: collapse speeds up where
    the three eigenvalues of phi,ij share a sign.  growth2 = -D_2 / D_1^2 at the epoch of the output: 3/7 in an
    Einstein-de Sitter universe (the default), and -cosmology.growth_factor_2(z, Om) / cosmology.growth_factor(z, Om)^2 in
    flat LambdaCDM, which stays within half a percent of 3/7.  Any finite value is taken as given; 0 leaves first order.

    The plain call is one pass that reads delta_k and S_k and writes the three spectra, and eleven transforms where
    first order has four.  return_orders=True returns (psi1, psi2) instead: two nbe_zeldovich_spectrum passes with the
    scales a and b, and six inverse transforms, so psi1 has the bits of `zeldovich_displacement`.  dealias as in
    `lpt2_source`.  2LPT velocities, 3LPT, glass pre-initial conditions and non-cubic boxes are not built."""
    d, n, L, scale, growth2, p = _validate_lpt2(delta, boxsize, scale, growth2, dealias, "lpt2_displacement")
    return_orders = _flag(return_orders, "return_orders")
    a, b = scale, growth2 * scale * scale
    dev = _device_of(d)
    with torch.cuda.device(dev):
        _lpt2_budget(dev, n, p, "lpt2_displacement")
        spec = _half_spectrum(_to_device(d, dev, (torch.float32,)))
        s_k = _source_spectrum(spec, n, p, _max_batch)
        if return_orders:
            psi1 = _inverse_components(_psi_spectrum(spec, n, L, a), n, _max_batch)
            del spec
            psi2 = _inverse_components(_psi_spectrum(s_k, n, L, b), n, _max_batch)
            return _back(d, psi1), _back(d, psi2)
        psi_k = _psi2_spectrum(spec, s_k, n, L, a, b)
        del spec, s_k
        psi = _inverse_components(psi_k, n, _max_batch)
    return _back(d, psi)


# ---- resizing --------------------------------------------------------------------------------------------------------------

def _resize_spectrum(spec, n_in, n_out, sphere=False):
    """nbe_spectrum_resize on a contiguous complex64 half spectrum on the device."""
    out = _empty_spectrum(n_out, spec.device)
    _lib.check(_lib.lib().nbe_spectrum_resize(_ptr(spec), n_in, _ptr(out), n_out, int(bool(sphere)),
                                              _stream(spec.device)))
    return out


def _validate_table(k_target, pk_target):
    """The tabulated P(k) of mode injection, checked as the reference checks it (scripts/utils.py:484-495) except that an
    unsorted table is an error here: (k, pk, slope, intercept) with the log-log tail fit."""
    if k_target is None or pk_target is None:
        raise ValueError("mode_inject needs a tabulated P(k): both k_target and pk_target (there is no default spectrum)")
    try:
        k = np.asarray(k_target, dtype=np.float64).ravel()
        pk = np.asarray(pk_target, dtype=np.float64).ravel()
    except (TypeError, ValueError):
        raise ValueError("k_target and pk_target must be numbers")
    if k.size < 2 or pk.size != k.size:
        raise ValueError("invalid tabulated P(k): need matching arrays with at least two points, got %d and %d"
                         % (k.size, pk.size))
    if not np.isfinite(k).all() or not np.isfinite(pk).all():
        raise ValueError("k_target and pk_target must be finite")
    if (np.diff(k) <= 0).any() or k[0] <= 0:
        raise ValueError("k_target values must be positive and strictly increasing")
    t = min(_TAIL_POINTS, k.size)
    if (pk[-t:] <= 0).any():
        raise ValueError("the last %d values of pk_target must be positive: the tail is fitted in log-log" % t)
    slope, intercept = np.polyfit(np.log(k[-t:]), np.log(pk[-t:]), 1)
    if not np.isfinite(slope) or not np.isfinite(intercept):
        raise ValueError("the log-log tail fit of the tabulated P(k) is not finite")
    return k, pk, float(slope), float(intercept)


def _seed(seed):
    if isinstance(seed, (bool, np.bool_)) or not isinstance(seed, numbers.Integral) or not 0 <= int(seed) < 2 ** 64:
        raise ValueError("seed must be an int in 0 .. 2^64 - 1, got %r" % (seed,))
    return int(seed)


def _inject_spectrum(spec, n_in, n_out, table, L, seed):
    """nbe_spectrum_inject on a contiguous complex64 half spectrum on the device; table from _validate_table."""
    k, pk, slope, intercept = table
    dev = spec.device
    kd, pd = torch.from_numpy(k).to(dev), torch.from_numpy(pk).to(dev)
    out = _empty_spectrum(n_out, dev)
    _lib.check(_lib.lib().nbe_spectrum_inject(_ptr(spec), n_in, _ptr(out), n_out, _ptr(kd), _ptr(pd), int(k.size), slope,
                                              intercept, L, seed, _stream(dev)))
    return out


def _validate_inject(delta, target_res, boxsize, k_target, pk_target, seed, what):
    d, n, L = _field(delta, boxsize, what)
    m = _size(target_res, "target_res")
    if m < n:
        raise ValueError("%s: target_res %d is below the input's %d" % (what, m, n))
    return d, n, L, m, _validate_table(k_target, pk_target), _seed(seed)


def inject_spectrum(delta, target_res, boxsize=1000.0, k_target=None, pk_target=None, seed=0):
    """The complex half spectrum (target_res, target_res, target_res // 2 + 1) of "mode_inject" before its inverse
    transform (reference scripts/utils.py:261-346, :349-425).

    Inside the sphere 4 |m|^2 <= n_in^2 the modes are those of "fourier" upsampling.  Outside, mode m is a Gaussian draw
    with E|F|^2 = sigma^2, sigma = n_out^3 sqrt(P(|k|) / L^3).  P is evaluated in float64: linear in k between the table's
    points (np.interp), pk_target[0] below them, exp(intercept + slope ln k) above k_target[-1], with the line fitted by
    np.polyfit to the last min(8, ntable) points in log-log as in the reference, and clamped at 0.

    The draw is counter-based, so it depends on the seed and the mode alone: Philox4x32-10 with key (seed low word, seed
    high word) and counter (r0, r1, i2, 0), where (r0, r1, i2) is the mode's index in the half spectrum.  On the planes
    i2 = 0 and (n_out even) i2 = n_out/2 the rows (i0, i1) and ((n - i0) % n, (n - i1) % n) form a pair: the one with the
    smaller i0 n + i1 supplies the counter and the other takes the complex conjugate.  U1 = (x0 + 1/2) 2^-32,
    U2 = (x1 + 1/2) 2^-32, g = sqrt(-2 ln U1) (cospi(2 U2) + i sinpi(2 U2)) in float64.  A mode that is its own mirror image
    gets F = sigma Re g, every other F = sigma g / sqrt(2); each word is rounded to float32 once.  The result is the half
    spectrum of a real field by construction, without the two extra transforms of the reference's projection.

    The 32-bit uniforms cut the Gaussian tail: |g| <= sqrt(-2 ln 2^-33) = 6.8, so no draw exceeds 6.8 sigma.  The random
    streams of NumPy or JAX are not matched (the reference's two backends do not match each other either).

    seed: an int in 0 .. 2^64 - 1.  Returns a complex64 array of the input's kind."""
    d, n, L, m, table, seed = _validate_inject(delta, target_res, boxsize, k_target, pk_target, seed, "inject_spectrum")
    dev = _device_of(d)
    with torch.cuda.device(dev):
        return _back(d, _inject_spectrum(_half_spectrum(_to_device(d, dev, (torch.float32,))), n, m, table, L, seed))


def _smooth(x, n, sigma_over_L):
    spec = _half_spectrum(x)
    _lib.check(_lib.lib().nbe_gaussian_filter(_ptr(spec), n, sigma_over_L, _stream(x.device)))
    return _real_field(spec, n)


def _real_pass(fn, x, n_in, n_out):
    """One of the real-space kernels (block average, trilinear interpolation) from n_in^3 to n_out^3."""
    out = torch.empty((n_out,) * 3, dtype=torch.float32, device=x.device)
    _lib.check(fn(_ptr(x), n_in, _ptr(out), n_out, _stream(x.device)))
    return out


def gaussian_smooth(delta, boxsize, sigma):
    """The field smoothed with a Gaussian of standard deviation sigma (the unit of boxsize): its spectrum times
    exp(-|k|^2 sigma^2 / 2), Pylians' FT_filter(boxsize, sigma, n, "Gaussian") and field_smoothing (reference
    scripts/utils.py:590-591).  delta: cubic (n, n, n) float32, NumPy array or CUDA tensor; returns the same kind."""
    d, n, L = _field(delta, boxsize, "gaussian_smooth")
    sigma = _real(sigma, "sigma", positive=True)
    dev = _device_of(d)
    with torch.cuda.device(dev):
        return _back(d, _smooth(_to_device(d, dev, (torch.float32,)), n, sigma / L))


_REQUIRED = object()


def _method(n, m, upsample_method, downsample_method):
    """The method that takes n^3 to m^3 (None for equal sizes), after checking both names and the ratio it needs."""
    if upsample_method is _REQUIRED or upsample_method not in UPSAMPLE_METHODS:
        raise ValueError("upsample_method must be one of %s, got %s"
                         % (UPSAMPLE_METHODS, "nothing" if upsample_method is _REQUIRED else repr(upsample_method)))
    if downsample_method not in DOWNSAMPLE_METHODS:
        raise ValueError("downsample_method must be one of %s, got %r" % (DOWNSAMPLE_METHODS, downsample_method))
    if m == n:
        return None
    method = upsample_method if m > n else downsample_method
    if method in ("linear", "gaussian", "block_average") and max(m, n) % min(m, n):
        raise ValueError("resize_density: %r needs an integer ratio, got %d -> %d" % (method, n, m))
    return method


def resize_density(delta, target_res, boxsize=1000.0, upsample_method=_REQUIRED, downsample_method="gaussian",
                   gaussian_sigma=None, k_target=None, pk_target=None, seed=0):
    """Resize a cubic periodic density field between resolutions (reference scripts/utils.py:595-655,
    resize_density_grid).

    delta: cubic (n, n, n) float32, NumPy array or CUDA tensor, 2 <= n <= 2048; target_res: 2 .. 2048.  Equal sizes return
    the input.  upsample_method has no default, as in the reference, and both method names are checked whichever way the
    call goes.

    Upwards: "fourier" (every mode of the coarse grid, an even Nyquist row split evenly onto +-n/2: the result equals the
    input at the coarse nodes), "linear" (periodic trilinear interpolation at the fine nodes) or "mode_inject" (the coarse
    modes inside the sphere |m| <= n/2, Gaussian draws from the table k_target / pk_target beyond it, reproducible from
    `seed`: see inject_spectrum; the table is required, there is no default spectrum here).
    Downwards: "gaussian" (gaussian_smooth with gaussian_sigma, default boxsize / target_res, then the block average),
    "block_average" (the mean of each block) or "fourier" (the exact inverse of "fourier" upsampling, which the reference
    does not have: a fine Nyquist component is the sum of the source at both signs).
    "linear", "gaussian" and "block_average" need an integer ratio of the sizes; "fourier" and "mode_inject" do not.

    Returns (target_res,) * 3 float32 of the input's kind."""
    d, n, L = _field(delta, boxsize, "resize_density")
    m = _size(target_res, "target_res")
    method = _method(n, m, upsample_method, downsample_method)
    if gaussian_sigma is not None:
        gaussian_sigma = _real(gaussian_sigma, "gaussian_sigma", positive=True)
    if method is None:
        return d
    table = seed_value = None
    if method == "mode_inject":
        table, seed_value = _validate_table(k_target, pk_target), _seed(seed)
    dev = _device_of(d)
    l = _lib.lib()
    with torch.cuda.device(dev):
        x = _to_device(d, dev, (torch.float32,))
        if method == "fourier":
            out = _real_field(_resize_spectrum(_half_spectrum(x), n, m), m)
        elif method == "mode_inject":
            out = _real_field(_inject_spectrum(_half_spectrum(x), n, m, table, L, seed_value), m)
        elif method == "linear":
            out = _real_pass(l.nbe_trilinear_upsample, x, n, m)
        else:
            if method == "gaussian":
                x = _smooth(x, n, (L / m if gaussian_sigma is None else gaussian_sigma) / L)
            out = _real_pass(l.nbe_block_average, x, n, m)
    return _back(d, out)


# ---- the linear field from a seed ------------------------------------------------------------------------------------------

FIXED_AMPLITUDE, INVERT_PHASE, WHITE_NOISE = 1, 2, 4      # include/nbe.h: NBE_IC_FIXED_AMPLITUDE, _INVERT_PHASE, _WHITE_NOISE


def _flag(v, name):
    if not isinstance(v, (bool, np.bool_)):
        raise ValueError("%s must be a bool, got %r" % (name, v))
    return bool(v)


def _flags(fixed_amplitude, invert_phase):
    return (FIXED_AMPLITUDE if _flag(fixed_amplitude, "fixed_amplitude") else 0) | \
        (INVERT_PHASE if _flag(invert_phase, "invert_phase") else 0)


def _cuda_device(device):
    """`device` as a torch.device of type cuda, or None for the current one (resolved when the device work starts)."""
    if device is None:
        return None
    try:
        dev = torch.device("cuda", device) if isinstance(device, numbers.Integral) and not isinstance(device, bool) \
            else torch.device(device)
    except (TypeError, RuntimeError, ValueError):
        raise ValueError("device must be a CUDA (HIP) device, got %r" % (device,))
    if dev.type != "cuda":
        raise ValueError("device must be a CUDA (HIP) device, got %r: there is no CPU fallback" % (device,))
    return dev


def _resolve(dev):
    cur = density._device()
    return cur if dev is None or dev.index is None else dev


def _out_kind(out):
    if out not in ("torch", "numpy"):
        raise ValueError("out must be 'torch' or 'numpy', got %r" % (out,))
    return out


def _max_blocks(v):
    if v is None:
        return 0
    if isinstance(v, (bool, np.bool_)) or not isinstance(v, numbers.Integral) or int(v) < 1:
        raise ValueError("_max_blocks must be a positive int, got %r" % (v,))
    return int(v)


def _validate_draw(n, boxsize, k_table, pk_table, seed, scale, fixed_amplitude, invert_phase, device, max_blocks, what):
    """Every argument of a draw, before any device work: (n, L, table, seed, scale, flags, device or None, max_blocks)."""
    n = _size(n, "n")
    L = density._triple(boxsize, "boxsize", "a length")
    if len(set(L)) != 1:
        raise ValueError("%s needs a cubic box, got boxsize %s" % (what, L))
    return (n, L[0], _validate_table(k_table, pk_table), _seed(seed), _real(scale, "scale", positive=True),
            _flags(fixed_amplitude, invert_phase), _cuda_device(device), _max_blocks(max_blocks))


def _draw_spectrum(n, L, table, seed, scale, flags, dev, max_blocks=0):
    """nbe_gaussian_spectrum on device `dev`; table from _validate_table, or None with the WHITE_NOISE flag."""
    out = _empty_spectrum(n, dev)
    if flags & WHITE_NOISE:
        kp = pp = None
        nt, slope, intercept = 0, 0.0, 0.0
    else:
        k, pk, slope, intercept = table
        kd, pd = torch.from_numpy(k).to(dev), torch.from_numpy(pk).to(dev)
        kp, pp, nt = _ptr(kd), _ptr(pd), int(k.size)
    _lib.check(_lib.lib().nbe_gaussian_spectrum(_ptr(out), n, kp, pp, nt, slope, intercept, L, scale, seed, flags,
                                                max_blocks, _stream(dev)))
    return out


def _colour_spectrum(spec, n, table, L, scale):
    """nbe_spectrum_colour, in place, on a contiguous complex64 half spectrum on the device."""
    k, pk, slope, intercept = table
    dev = spec.device
    kd, pd = torch.from_numpy(k).to(dev), torch.from_numpy(pk).to(dev)
    _lib.check(_lib.lib().nbe_spectrum_colour(_ptr(spec), n, _ptr(kd), _ptr(pd), int(k.size), slope, intercept, L, scale,
                                              _stream(dev)))
    return spec


def gaussian_spectrum(n, boxsize=1000.0, k_table=None, pk_table=None, seed=0, scale=1.0, fixed_amplitude=False,
                      invert_phase=False, device=None, _max_blocks=None):
    """The complex64 half spectrum (n, n, n // 2 + 1) of a Gaussian random field with the tabulated linear P(k), drawn on
    the device from a seed: the draw of the reference's run_lpt_emulator_pipeline(seed=...) (scripts/core.py:263-302, white
    noise coloured with a tabulated P(k)).  Returns a CUDA tensor on `device` (default: the current one).

    One seed is one universe at every resolution.  For a mesh of n^3, 2 <= n <= 2048, the half spectrum has index
    (i0, i1, i2), 0 <= i2 <= n/2, and signed wave numbers m_c = i_c for i_c <= n/2 and i_c - n above, so an even Nyquist
    row is +n/2.

    Pairing (that of `inject_spectrum`): on the planes i2 = 0 and (n even) i2 = n/2 the rows (i0, i1) and
    ((n - i0) % n, (n - i1) % n) form a pair; the row with the smaller i0 n + i1 draws, the other takes the complex
    conjugate, and a row that is its own mirror is a self mode.

    Counter: Philox4x32-10 with key (seed low word, seed high word) and counter ((uint32) m0, (uint32) m1, (uint32) m2, 1),
    where m0 and m1 are the two's-complement signed wave numbers of the drawing row.  `inject_spectrum` uses mesh indices
    and a last word of 0, so the two streams never share a counter, and this counter does not depend on n.

    Uniforms and the Gaussian (as in `inject_spectrum`): U1 = (x0 + 1/2) 2^-32, U2 = (x1 + 1/2) 2^-32,
    g = sqrt(-2 ln U1) (cospi(2 U2) + i sinpi(2 U2)) in float64; no draw exceeds 6.8 sigma.

    Amplitude: sigma = scale n^3 sqrt(P(|k|) / L^3), multiplied in that order, |k| = (2 pi / L) sqrt(|m|^2) with the integer
    |m|^2.  P is evaluated as `inject_spectrum` documents: np.interp inside the table, pk_table[0] below it, the fitted
    log-log tail above it, clamped at 0.  Only products follow, so sigma and every word for n and 2n differ by exactly 8.

    Modes: F(0) = +0; a self mode gets F = sigma Re g (imaginary word +0); every other mode F = sigma g / sqrt(2).  Each
    float32 word is rounded once.  `fixed_amplitude=True` (the Quijote "fixed" fields): a non-self mode gets
    F = sigma (cospi(2 U2) + i sinpi(2 U2)), a self mode +sigma if cospi(2 U2) >= 0 and -sigma otherwise.
    `invert_phase=True` (the "paired" partner): F -> -F for every mode; words that are +0 stay +0.

    What nesting covers: modes with every |m_c| < n/2 and i2 > 0 are the same draws at every n, and so are the drawing
    rows of the plane i2 = 0 (which row of a pair draws does not depend on n either).  Modes on a Nyquist row of an even n
    are not the same draws at other resolutions: at n such a mode is constrained (paired or self), at 2n it is an ordinary
    mode.

    `scale` (finite, > 0) multiplies the field, e.g. the growth factor D(a) / D(a_0) for a table given at a_0; the paired
    field is `invert_phase`, not a negative scale.  N-GenIC's own random stream is not matched, and DISCO-DJ cannot be
    imported where this library is developed; a reference run is reproduced through `colour_noise` from the two files it
    writes (white_noise_ngenic.npy and class_linear_pk_*_table.txt).  The table is required: CLASS is not available
    here, and the table is taken as given (no sigma_8 normalisation)."""
    n, L, table, seed, scale, flags, dev, mb = _validate_draw(n, boxsize, k_table, pk_table, seed, scale, fixed_amplitude,
                                                              invert_phase, device, _max_blocks, "gaussian_spectrum")
    dev = _resolve(dev)
    with torch.cuda.device(dev):
        return _draw_spectrum(n, L, table, seed, scale, flags, dev, mb)


def gaussian_field(n, boxsize=1000.0, k_table=None, pk_table=None, seed=0, scale=1.0, fixed_amplitude=False,
                   invert_phase=False, device=None, _max_blocks=None, out="torch"):
    """The (n, n, n) float32 linear density field of `gaussian_spectrum` (same arguments and definition; reference
    scripts/core.py:263-302): one draw pass and one irfftn.  out: "torch" (a CUDA tensor on `device`) or "numpy"."""
    n, L, table, seed, scale, flags, dev, mb = _validate_draw(n, boxsize, k_table, pk_table, seed, scale, fixed_amplitude,
                                                              invert_phase, device, _max_blocks, "gaussian_field")
    out = _out_kind(out)
    dev = _resolve(dev)
    with torch.cuda.device(dev):
        x = _real_field(_draw_spectrum(n, L, table, seed, scale, flags, dev, mb), n)
    return x if out == "torch" else x.cpu().numpy()


def white_noise(n, seed=0, fixed_amplitude=False, invert_phase=False, device=None, out="torch"):
    """A real (n, n, n) float32 white-noise field of unit variance: the draw of `gaussian_spectrum` with sigma = n^(3/2)
    under torch's unnormalised forward transform, so colour_noise(white_noise(n, seed), ...) is gaussian_field(n, ...,
    seed=seed) up to the rounding of the two extra transforms.  out: "torch" (a CUDA tensor on `device`) or "numpy"."""
    n, seed, flags, dev, out = _size(n, "n"), _seed(seed), _flags(fixed_amplitude, invert_phase), _cuda_device(device), \
        _out_kind(out)
    dev = _resolve(dev)
    with torch.cuda.device(dev):
        x = _real_field(_draw_spectrum(n, 1.0, None, seed, 1.0, flags | WHITE_NOISE, dev), n)
    return x if out == "torch" else x.cpu().numpy()


def colour_noise(white, boxsize, k_table, pk_table, scale=1.0):
    """The linear density field of somebody else's white noise (reference scripts/core.py:263-302, which colours N-GenIC's
    white noise with the CLASS table; both are written by a reference run as white_noise_ngenic.npy and
    class_linear_pk_*_table.txt).

    white: cubic (n, n, n) float32 of unit variance, NumPy array or CUDA tensor, 2 <= n <= 2048.  With w_k its unnormalised
    forward transform, delta_k = w_k scale sqrt(n^3 P(|k|) / L^3): the multiplier in float64, each word of the product
    rounded once, delta_0 = 0; P as `inject_spectrum` documents.  One rfftn, the colour pass in place, one irfftn.  Returns
    (n, n, n) float32 of the input's kind."""
    w, n, L = _cubic(white, "white", boxsize, "colour_noise", "(n, n, n) field", MIN_N, MAX_N)
    table, scale = _validate_table(k_table, pk_table), _real(scale, "scale", positive=True)
    dev = _device_of(w)
    with torch.cuda.device(dev):
        spec = _colour_spectrum(_half_spectrum(_to_device(w, dev, (torch.float32,))), n, table, L, scale)
        return _back(w, _real_field(spec, n))


def linear_ics(n, boxsize, k_table, pk_table, seed, scale=1.0, fixed_amplitude=False, invert_phase=False,
               return_delta=True, device=None, _max_batch=None, order=1, growth2=EDS_GROWTH2, dealias=False):
    """Initial conditions from a seed: (delta, psi) on the device, the linear field of `gaussian_spectrum` (reference
    scripts/core.py:263-302) and its first-order LPT displacement (scripts/core.py:396-397), without a forward transform.

    order=2 returns (delta, psi1, psi) instead: psi1 is what order=1 returns as psi, bit for bit, and psi is the
    second-order displacement of `lpt2_displacement` (growth2 and dealias are its arguments), for which the drawn spectrum
    goes straight into the Hessian pass.  `scale` rides in the field, so psi = psi1 + psi2 with a = 1 and b = growth2.

    The drawn spectrum goes straight into nbe_zeldovich_spectrum and through the inverse path of `zeldovich_displacement`
    (batched, or one component at a time where memory is short), so psi has the bits zeldovich_displacement's inverse path
    gives for that spectrum; delta does not pass through real space on its way to psi.  delta: (n, n, n) float32, or None
    with return_delta=False (three irfftn instead of four).  psi: (3, n, n, n) float32, psi_k = i k / |k|^2 delta_k, valid
    process_box input.  `scale` enters through the field: delta and psi both carry it.  Both are CUDA tensors."""
    n, L, table, seed, scale, flags, dev, _ = _validate_draw(n, boxsize, k_table, pk_table, seed, scale, fixed_amplitude,
                                                             invert_phase, device, None, "linear_ics")
    return_delta = _flag(return_delta, "return_delta")
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, numbers.Integral) or int(order) not in (1, 2):
        raise ValueError("order must be 1 or 2, got %r" % (order,))
    growth2 = _real(growth2, "growth2")
    p = _dealias_size(n, dealias, "linear_ics") if order == 2 else n
    dev = _resolve(dev)
    with torch.cuda.device(dev):
        if order == 2:
            _lpt2_budget(dev, n, p, "linear_ics")
        spec = _draw_spectrum(n, L, table, seed, scale, flags, dev)
        psi_k = _psi_spectrum(spec, n, L, 1.0)
        delta = _real_field(spec, n) if return_delta else None
        if order == 1:
            del spec
            return delta, _inverse_components(psi_k, n, _max_batch)
        psi1 = _inverse_components(psi_k, n, _max_batch)
        del psi_k
        psi_k = _psi2_spectrum(spec, _source_spectrum(spec, n, p, _max_batch), n, L, 1.0, growth2)
        del spec
        psi = _inverse_components(psi_k, n, _max_batch)
    return delta, psi1, psi
