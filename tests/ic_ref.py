"""Float64 NumPy restatement of the linear field drawn from a seed (lpt.gaussian_spectrum has the
definition), built on lpt_ref's Philox, mode grid and P(k).  Written from the definition, not from the kernel.

A mesh of n^3 has the half spectrum (n, n, n//2+1); position i of an axis holds the signed wave number m = i for
i <= n//2 and i - n above.  On the planes i2 = 0 and (n even) i2 = n/2 the rows (i0, i1) and ((n-i0)%n, (n-i1)%n) form a
pair: the one with the smaller i0 n + i1 draws, the other takes the complex conjugate, a row that is its own mirror is a
self mode.  The Philox counter is the drawing row's signed wave vector (two's complement) and a last word of 1.
"""

import numpy as np

import lpt_ref as R

FIXED, INVERT, WHITE = 1, 2, 4


def pairing(n):
    """(second, own, d0, d1) on the half spectrum: whether a mode is the second of a pair, whether it is its own mirror,
    and the signed wave numbers (m0, m1) of the row that draws for it."""
    h = n // 2 + 1
    i0, i1, i2 = np.meshgrid(np.arange(n), np.arange(n), np.arange(h), indexing="ij")
    p0, p1 = (n - i0) % n, (n - i1) % n
    paired = (i2 == 0) | ((n % 2 == 0) & (i2 == n // 2))
    second = paired & (p0 * n + p1 < i0 * n + i1)
    own = paired & (p0 == i0) & (p1 == i1)
    m = R.wave_numbers(n)
    return second, own, m[np.where(second, p0, i0)], m[np.where(second, p1, i1)]


def uniforms(n, seed):
    """(U1, U2, second, own) on the half spectrum of an n^3 mesh."""
    second, own, d0, d1 = pairing(n)
    m2 = np.broadcast_to(np.arange(n // 2 + 1, dtype=np.int64)[None, None, :], d0.shape)
    seed = int(seed)
    x0, x1, _, _ = R.philox4x32_10(d0 & R.MASK, d1 & R.MASK, m2, np.ones_like(m2), seed & R.MASK, (seed >> 32) & R.MASK)
    u1 = (x0.astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (x1.astype(np.float64) + 0.5) * 2.0 ** -32
    return u1, u2, second, own


def phasor(u2):
    return np.cos(2.0 * np.pi * u2) + 1j * np.sin(2.0 * np.pi * u2)


def gaussian_draws(n, seed):
    """(g, second, own): the complex draw g = sqrt(-2 ln U1) (cospi(2 U2) + i sinpi(2 U2)) of the drawing row of every mode,
    before any conjugation."""
    u1, u2, second, own = uniforms(n, seed)
    return np.sqrt(-2.0 * np.log(u1)) * phasor(u2), second, own


def sigma(n, boxsize, k_table, pk_table, scale=1.0):
    """sigma = scale n^3 sqrt(P(|k|) / L^3) on the half spectrum, multiplied in that order."""
    _, _, _, q = R.mode_grid(n)
    k_table, pk_table = np.asarray(k_table, np.float64), np.asarray(pk_table, np.float64)
    slope, intercept = R.tail_fit(k_table, pk_table)
    k = (2.0 * np.pi / boxsize) * np.sqrt(q.astype(np.float64))
    return (float(scale) * float(n) ** 3) * np.sqrt(R.table_power(k, k_table, pk_table, slope, intercept) / float(boxsize) ** 3)


def gaussian_spectrum(n, boxsize=1000.0, k_table=None, pk_table=None, seed=0, scale=1.0, flags=0):
    """The complex128 half spectrum; flags: FIXED | INVERT | WHITE (sigma = n^(3/2), the table is not read)."""
    u1, u2, second, own = uniforms(n, seed)
    s = np.full(u1.shape, float(n) ** 1.5) if flags & WHITE else np.broadcast_to(sigma(n, boxsize, k_table, pk_table, scale),
                                                                                  u1.shape)
    e = phasor(u2)
    if flags & FIXED:
        F = np.where(own, np.where(e.real >= 0, s, -s), s * e)
    else:
        g = np.sqrt(-2.0 * np.log(u1)) * e
        F = np.where(own, s * g.real, s * g / np.sqrt(2.0))
    F = np.where(second, np.conj(F), F)
    if flags & INVERT:
        F = -F
    F[0, 0, 0] = 0.0
    return F


def gaussian_field(n, *args, **kw):
    return np.fft.irfftn(gaussian_spectrum(n, *args, **kw), s=(n, n, n), axes=(0, 1, 2))


def colour_spectrum(w_k, n, boxsize, k_table, pk_table, scale=1.0):
    """delta_k = w_k scale sqrt(n^3 P(|k|) / L^3), delta_0 = 0."""
    _, _, _, q = R.mode_grid(n)
    k_table, pk_table = np.asarray(k_table, np.float64), np.asarray(pk_table, np.float64)
    slope, intercept = R.tail_fit(k_table, pk_table)
    k = (2.0 * np.pi / boxsize) * np.sqrt(q.astype(np.float64))
    mult = float(scale) * np.sqrt(float(n) ** 3 * R.table_power(k, k_table, pk_table, slope, intercept) / float(boxsize) ** 3)
    out = np.asarray(w_k, np.complex128) * mult
    out[0, 0, 0] = 0.0
    return out


def colour_noise(white, boxsize, k_table, pk_table, scale=1.0):
    white = np.asarray(white, np.float64)
    n = white.shape[0]
    return np.fft.irfftn(colour_spectrum(np.fft.rfftn(white), n, boxsize, k_table, pk_table, scale), s=(n, n, n),
                         axes=(0, 1, 2))


def independent(n):
    """The modes that carry a draw of their own: not the second of a pair, not self, not DC."""
    second, own, _, _ = pairing(n)
    _, _, _, q = R.mode_grid(n)
    return ~second & ~own & (q > 0)
