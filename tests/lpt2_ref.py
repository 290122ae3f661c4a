"""Float64 NumPy restatement of second-order LPT: the definitions that nbe_lpt2_hessian_spectrum,
nbe_lpt2_source and nbe_lpt2_spectrum (csrc/nbe_lpt.hip), lpt.lpt2_source / lpt2_displacement and the second-order growth
of cosmology.py are held to.  Written from the definitions, not from the kernels.  Conventions are lpt_ref's: half
spectra (n, n, n//2+1) of the unnormalised forward transform, integer wave vectors m, k = 2 pi m / L.
"""

import numpy as np

from lpt_ref import mode_grid, red_field, spectrum_resize, zeldovich_spectrum  # noqa: F401  (red_field: for the tests)

PAIRS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))
EDS = 3.0 / 7.0


def derivative_numbers(n):
    """(d0, d1, d2, q): d_c = m_c, or 0 where n is even and |m_c| = n/2 (the Nyquist rule of the first derivative);
    q = |m|^2 is the true integer."""
    m0, m1, m2, q = mode_grid(n)
    d = [np.where((n % 2 == 0) & (np.abs(m) == n // 2), 0, m) for m in (m0, m1, m2)]
    return d[0], d[1], d[2], q


def hessian_spectrum(spec, n):
    """(6, n, n, h) complex128: phi,ij_k = d_i d_j / |m|^2 delta_k in the order PAIRS; 0 at m = 0."""
    spec = np.asarray(spec, dtype=np.complex128)
    d0, d1, d2, q = derivative_numbers(n)
    d = (d0, d1, d2)
    out = np.zeros((6,) + spec.shape, np.complex128)
    for p, (i, j) in enumerate(PAIRS):
        num = np.broadcast_to(d[i] * d[j], q.shape).astype(np.float64)
        out[p] = np.where(q > 0, num / np.maximum(q, 1).astype(np.float64), 0.0) * spec
    return out


def source(h):
    """S = ((h0 h1 + h0 h2) + h1 h2) - ((h3^2 + h4^2) + h5^2) of six real fields, float64, in that order."""
    h = [np.asarray(x, dtype=np.float64) for x in h]
    return ((h[0] * h[1] + h[0] * h[2]) + h[1] * h[2]) - ((h[3] * h[3] + h[4] * h[4]) + h[5] * h[5])


def hessian_fields(spec, n, p):
    """The six real fields on the p^3 mesh (p >= n: each spectrum Fourier-interpolated upwards first)."""
    hk = hessian_spectrum(spec, n)
    if p != n:
        hk = np.stack([spectrum_resize(hk[c], n, p) for c in range(6)])
    return np.fft.irfftn(hk, s=(p, p, p), axes=(1, 2, 3))


def source_spectrum(spec, n, dealias=False):
    """S_k at n: formed at n, or with `dealias` on the mesh of 3 n / 2 and brought back by Fourier downsampling."""
    p = 3 * n // 2 if dealias else n
    s_k = np.fft.rfftn(source(hessian_fields(spec, n, p)))
    return spectrum_resize(s_k, p, n) if p != n else s_k


def lpt2_source(delta, dealias=False):
    delta = np.asarray(delta, dtype=np.float64)
    n = delta.shape[0]
    if not dealias:
        return source(hessian_fields(np.fft.rfftn(delta), n, n))
    return np.fft.irfftn(source_spectrum(np.fft.rfftn(delta), n, True), s=(n, n, n), axes=(0, 1, 2))


def lpt2_spectrum(delta_k, source_k, n, boxsize, a, b):
    """(3, n, n, h) complex128: psi_c = i (L / 2 pi) d_c / |m|^2 (a delta_k + b S_k)."""
    return zeldovich_spectrum(a * np.asarray(delta_k, np.complex128) + b * np.asarray(source_k, np.complex128), n, boxsize)


def lpt2_orders(delta, boxsize=1000.0, scale=1.0, growth2=EDS, dealias=False):
    """(psi1, psi2), each (3, n, n, n) float64; psi = psi1 + psi2."""
    delta = np.asarray(delta, dtype=np.float64)
    n = delta.shape[0]
    spec = np.fft.rfftn(delta)
    s_k = source_spectrum(spec, n, dealias)
    inv = lambda x: np.fft.irfftn(x, s=(n, n, n), axes=(1, 2, 3))
    return inv(zeldovich_spectrum(spec, n, boxsize, scale)), inv(zeldovich_spectrum(s_k, n, boxsize, growth2 * scale * scale))


def lpt2_displacement(delta, boxsize=1000.0, scale=1.0, growth2=EDS, dealias=False):
    psi1, psi2 = lpt2_orders(delta, boxsize, scale, growth2, dealias)
    return psi1 + psi2


# ---- second-order growth ---------------------------------------------------------------------------------------------------

def growth2_ode(z, Om, steps=20000, a_start=1.0e-4):
    """(D1, D2, f2) of flat LambdaCDM at redshift z (arrays broadcast), D1(z = 0) = 1: the pair
        D1'' + (2 + dlnH/dlna) D1' - 1.5 Om(a) D1 = 0,   D2'' + (2 + dlnH/dlna) D2' - 1.5 Om(a) D2 = -1.5 Om(a) D1^2
    in x = ln a (primes d/dx), from D1 = a, D2 = -3/7 a^2 at a_start, by `steps` equal RK4 steps to a = 1 / (1 + z) and,
    for the normalisation, as many to a = 1."""
    z, Om = np.broadcast_arrays(np.asarray(z, np.float64), np.asarray(Om, np.float64))
    ends = np.stack([np.log(1.0 / (1.0 + z)), np.zeros(z.shape)])
    Om = np.broadcast_to(Om, ends.shape)

    def rhs(x, y):
        m = Om * np.exp(-3.0 * x)
        oma = m / (m + 1.0 - Om)
        dlnh = -1.5 * oma
        return np.stack([y[1], 1.5 * oma * y[0] - (2.0 + dlnh) * y[1],
                         y[3], 1.5 * oma * y[2] - (2.0 + dlnh) * y[3] - 1.5 * oma * y[0] * y[0]])

    x = np.full(ends.shape, np.log(a_start))
    h = (ends - x) / steps
    y = np.stack([np.full(ends.shape, v) for v in (a_start, a_start, -EDS * a_start ** 2, -2.0 * EDS * a_start ** 2)])
    for _ in range(steps):
        k1 = rhs(x, y)
        k2 = rhs(x + h / 2, y + h / 2 * k1)
        k3 = rhs(x + h / 2, y + h / 2 * k2)
        k4 = rhs(x + h, y + h * k3)
        y = y + h / 6 * (k1 + 2 * k2 + 2 * k3 + k4)
        x = x + h
    d1_today = y[0, 1]
    return y[0, 0] / d1_today, y[2, 0] / d1_today ** 2, y[3, 0] / y[2, 0]


def matter_fraction(z, Om):
    z, Om = np.asarray(z, np.float64), np.asarray(Om, np.float64)
    m = Om * (1.0 + z) ** 3
    return m / (m + 1.0 - Om)


# ---- test fields ----------------------------------------------------------------------------------------------------------

def phase(n, j, axis):
    """2 pi j i / n along `axis`, broadcastable to (n, n, n)."""
    shape = [1, 1, 1]
    shape[axis] = n
    return (2.0 * np.pi * j * np.arange(n) / n).reshape(shape)


def plane_wave(n, j, axis, amp=0.3):
    return np.broadcast_to(amp * np.cos(phase(n, j, axis)), (n, n, n)).copy()


def crossed_waves(n, j1, j2, A, B, phi):
    """delta = A cos(j1 x) + B cos(j2 y + phi) on axes 0 and 1, with (cx, sx, cy, sy) = the cosines and sines."""
    x, y = phase(n, j1, 0), phase(n, j2, 1) + phi
    full = lambda f: np.broadcast_to(f, (n, n, n)).copy()
    return full(A * np.cos(x) + B * np.cos(y)), full(np.cos(x)), full(np.sin(x)), full(np.cos(y)), full(np.sin(y))


def band_limited(n, seed, top):
    """A random real field with power only where every |m_c| <= top, unit variance."""
    w = np.fft.rfftn(np.random.default_rng(seed).standard_normal((n, n, n)))
    m0, m1, m2, _ = mode_grid(n)
    keep = (np.abs(m0) <= top) & (np.abs(m1) <= top) & (np.abs(m2) <= top)
    x = np.fft.irfftn(np.where(keep, w, 0.0), s=(n, n, n), axes=(0, 1, 2))
    return x / x.std()
