"""Float64 NumPy restatement of jax_nbody_emulator_with_dj_amd.lpt: the definitions the HIP
kernels of csrc/nbe_lpt.hip are held to, Philox included.  Written from the definitions, not from the kernels.

Spectra are half spectra (n, n, n//2+1) of the unnormalised forward transform (np.fft.rfftn); position i of an axis of n
points holds the integer wave number m = i for i <= n//2 and i - n above, so an even axis stores its Nyquist row as +n/2.
"""

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57          # Philox4x32 multipliers and key increments (Salmon et al. 2011)
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK = 0xFFFFFFFF


def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on arrays (or ints) of counter words; returns four uint64 arrays of 32-bit values."""
    c0, c1, c2, c3 = (np.asarray(c, dtype=np.uint64) & np.uint64(MASK) for c in (c0, c1, c2, c3))
    k0, k1 = int(k0) & MASK, int(k1) & MASK
    for _ in range(10):
        p0 = np.uint64(M0) * c0
        p1 = np.uint64(M1) * c2
        n0 = (p1 >> np.uint64(32)) ^ c1 ^ np.uint64(k0)
        n2 = (p0 >> np.uint64(32)) ^ c3 ^ np.uint64(k1)
        c0, c1, c2, c3 = n0, p1 & np.uint64(MASK), n2, p0 & np.uint64(MASK)
        k0, k1 = (k0 + W0) & MASK, (k1 + W1) & MASK
    return c0, c1, c2, c3


def wave_numbers(n):
    i = np.arange(n, dtype=np.int64)
    return np.where(i <= n // 2, i, i - n)


def mode_grid(n):
    """(m0, m1, m2, q) of the half spectrum of an n^3 mesh, broadcastable int64 arrays; q = |m|^2."""
    m = wave_numbers(n)
    m0, m1, m2 = m[:, None, None], m[None, :, None], np.arange(n // 2 + 1, dtype=np.int64)[None, None, :]
    return m0, m1, m2, m0 * m0 + m1 * m1 + m2 * m2


def full_grid_weight(n):
    """How many modes of the full grid a mode of the half spectrum stands for: (1, 1, n//2+1) ints."""
    i2 = np.arange(n // 2 + 1)
    return np.where((i2 == 0) | ((n % 2 == 0) & (i2 == n // 2)), 1, 2)[None, None, :]


# ---- first-order LPT -----------------------------------------------------------------------------------------------------

def zeldovich_spectrum(spec, n, boxsize=1000.0, scale=1.0):
    """(3, n, n, h) complex128: psi_c = scale i k_c / |k|^2 delta_k, k = 2 pi m / L; 0 at m = 0, and component c is 0
    where n is even and |m_c| = n/2."""
    spec = np.asarray(spec, dtype=np.complex128)
    m0, m1, m2, q = mode_grid(n)
    out = np.zeros((3,) + spec.shape, np.complex128)
    inv = np.where(q > 0, 1.0 / np.maximum(q, 1), 0.0)
    for c, m in enumerate((m0, m1, m2)):
        mc = np.where((n % 2 == 0) & (np.abs(m) == n // 2), 0, m)
        out[c] = 1j * (scale * boxsize / (2.0 * np.pi)) * mc * inv * spec
    return out


def zeldovich_displacement(delta, boxsize=1000.0, scale=1.0):
    delta = np.asarray(delta, dtype=np.float64)
    n = delta.shape[0]
    psi = zeldovich_spectrum(np.fft.rfftn(delta), n, boxsize, scale)
    return np.fft.irfftn(psi, s=(n, n, n), axes=(1, 2, 3))


# ---- Fourier interpolation ----------------------------------------------------------------------------------------------

def source_value(src, n, a, b, c):
    """The source spectrum at the signed integer wave vectors (a, b, c) (arrays), |.| <= n/2: the stored mode for c >= 0,
    the conjugate of the stored mirror mode for c < 0."""
    neg = c < 0
    a, b, c = np.where(neg, -a, a), np.where(neg, -b, b), np.where(neg, -c, c)
    v = src[np.mod(a, n), np.mod(b, n), c]
    return np.where(neg, np.conj(v), v)


def axis_terms(m, n_in, n_out):
    """Per destination wave number m of one axis: (alive[2], source m[2], weight)."""
    a = np.abs(m)
    one = np.ones_like(m, dtype=bool)
    if n_out > n_in:
        return (a * 2 <= n_in, ~one), (m, -m), np.where(a * 2 == n_in, 0.5, 1.0)
    if n_out < n_in:
        return (one, a * 2 == n_out), (m, -m), np.ones(m.shape)
    return (one, ~one), (m, -m), np.ones(m.shape)


def spectrum_resize(src, n_in, n_out, sphere=False):
    """Fourier interpolation of a half spectrum to n_out, larger or smaller: (n_out / n_in)^3 times the source value at
    the same integer wave vector; zero beyond the source band and half weight per axis on an even source's Nyquist row
    (up); the sum over both signs of each destination Nyquist component (down); with `sphere`, zero where
    4 |m|^2 > n_in^2."""
    src = np.asarray(src, dtype=np.complex128)
    m0, m1, m2, q = mode_grid(n_out)
    shape = (n_out, n_out, n_out // 2 + 1)
    t = [axis_terms(m, n_in, n_out) for m in (m0, m1, m2)]
    acc = np.zeros(shape, np.complex128)
    for s0 in (0, 1):
        for s1 in (0, 1):
            for s2 in (0, 1):
                alive = np.broadcast_to(t[0][0][s0] & t[1][0][s1] & t[2][0][s2], shape)
                a, b, c = (np.broadcast_to(np.where(alive, t[x][1][s], 0), shape) for x, s in ((0, s0), (1, s1), (2, s2)))
                acc += np.where(alive, source_value(src, n_in, a, b, c), 0.0)
    r = float(n_out) / float(n_in)
    out = acc * ((r * r * r) * (t[0][2] * t[1][2] * t[2][2]))
    if sphere:
        out = np.where(4 * q <= n_in * n_in, out, 0.0)
    return out


def fourier_resize(delta, n_out):
    """The real field resized by Fourier interpolation, float64."""
    delta = np.asarray(delta, dtype=np.float64)
    n_in = delta.shape[0]
    return np.fft.irfftn(spectrum_resize(np.fft.rfftn(delta), n_in, n_out), s=(n_out,) * 3, axes=(0, 1, 2))


def full_spectrum(half, n):
    """The (n, n, n) complex spectrum whose half is `half`, completed by F(-m) = conj F(m) for the planes the half leaves
    out.  The planes i2 = 0 and n/2 are taken as they are: a half spectrum that is not Hermitian there shows as an
    imaginary part of np.fft.ifftn."""
    h = n // 2 + 1
    full = np.zeros((n, n, n), np.complex128)
    full[:, :, :h] = half
    i = (-np.arange(n)) % n
    for i2 in range(h, n):
        full[:, :, i2] = np.conj(half[i][:, i][:, :, n - i2])
    return full


# ---- mode injection ------------------------------------------------------------------------------------------------------

def tail_fit(k_table, pk_table):
    """(slope, intercept) of the log-log line through the last min(8, ntable) points, as the reference fits it."""
    t = min(8, len(k_table))
    slope, intercept = np.polyfit(np.log(k_table[-t:]), np.log(pk_table[-t:]), 1)
    return float(slope), float(intercept)


def table_power(k, k_table, pk_table, slope, intercept):
    k = np.asarray(k, dtype=np.float64)
    p = np.interp(k, k_table, pk_table, left=pk_table[0], right=pk_table[-1])
    hi = k > k_table[-1]
    with np.errstate(divide="ignore"):
        p = np.where(hi, np.exp(intercept + slope * np.log(np.where(hi, k, 1.0))), p)
    return np.maximum(p, 0.0)


def inject_sigma(n_out, boxsize, k_table, pk_table):
    """sigma = n_out^3 sqrt(P(|k|) / L^3) on the half spectrum."""
    _, _, _, q = mode_grid(n_out)
    slope, intercept = tail_fit(k_table, pk_table)
    k = (2.0 * np.pi / boxsize) * np.sqrt(q.astype(np.float64))
    return float(n_out) ** 3 * np.sqrt(table_power(k, k_table, pk_table, slope, intercept) / float(boxsize) ** 3)


def gaussian_draws(n, seed):
    """(g, own_mirror) on the half spectrum of an n^3 mesh: the complex draw of every mode (conjugated where the mode is
    the second of a pair) and whether the mode is its own mirror image."""
    h = n // 2 + 1
    i0, i1, i2 = np.meshgrid(np.arange(n), np.arange(n), np.arange(h), indexing="ij")
    p0, p1 = (n - i0) % n, (n - i1) % n
    paired = (i2 == 0) | ((n % 2 == 0) & (i2 == n // 2))
    second = paired & (p0 * n + p1 < i0 * n + i1)
    own = paired & (p0 == i0) & (p1 == i1)
    r0, r1 = np.where(second, p0, i0), np.where(second, p1, i1)
    seed = int(seed)
    x0, x1, _, _ = philox4x32_10(r0, r1, i2, np.zeros_like(i2), seed & MASK, (seed >> 32) & MASK)
    u1 = (x0.astype(np.float64) + 0.5) * 2.0 ** -32
    u2 = (x1.astype(np.float64) + 0.5) * 2.0 ** -32
    g = np.sqrt(-2.0 * np.log(u1)) * (np.cos(2.0 * np.pi * u2) + 1j * np.sin(2.0 * np.pi * u2))
    return np.where(second, np.conj(g), g), own


def spectrum_inject(src, n_in, n_out, k_table, pk_table, boxsize=1000.0, seed=0):
    """The resized spectrum inside the sphere 4 |m|^2 <= n_in^2, Gaussian draws with E|F|^2 = sigma^2 outside."""
    _, _, _, q = mode_grid(n_out)
    sigma = inject_sigma(n_out, boxsize, np.asarray(k_table, np.float64), np.asarray(pk_table, np.float64))
    g, own = gaussian_draws(n_out, seed)
    draw = np.where(own, sigma * g.real, sigma * g / np.sqrt(2.0))
    return np.where(4 * q <= n_in * n_in, spectrum_resize(src, n_in, n_out, sphere=True), draw)


# ---- real-space passes and the filter -----------------------------------------------------------------------------------------

def gaussian_filter(spec, n, sigma_over_L):
    _, _, _, q = mode_grid(n)
    return np.asarray(spec, np.complex128) * np.exp(-2.0 * np.pi ** 2 * q * float(sigma_over_L) ** 2)


def gaussian_smooth(delta, boxsize, sigma):
    delta = np.asarray(delta, dtype=np.float64)
    n = delta.shape[0]
    return np.fft.irfftn(gaussian_filter(np.fft.rfftn(delta), n, sigma / boxsize), s=(n,) * 3, axes=(0, 1, 2))


def block_average(x, n_out):
    x = np.asarray(x, dtype=np.float64)
    r = x.shape[0] // n_out
    return x.reshape(n_out, r, n_out, r, n_out, r).mean(axis=(1, 3, 5))


def trilinear(x, n_out):
    """Periodic trilinear interpolation at the fine nodes i n_in / n_out, n_out a multiple of n_in."""
    x = np.asarray(x, dtype=np.float64)
    n_in = x.shape[0]
    r = n_out // n_in
    i = np.arange(n_out)
    j, t = i // r, (i % r) / float(r)
    jp = (j + 1) % n_in

    def lerp(a, b, w):
        return (1.0 - w) * a + w * b

    def along2(a):                                        # a: (n_out, n_out, n_in) -> (n_out,) * 3
        return lerp(a[:, :, j], a[:, :, jp], t[None, None, :])

    def along1(a):                                        # a: (n_out, n_in, n_in)
        return lerp(along2(a[:, j, :]), along2(a[:, jp, :]), t[None, :, None])

    return lerp(along1(x[j]), along1(x[jp]), t[:, None, None])


def resize_density(delta, target_res, boxsize=1000.0, upsample_method=None, downsample_method="gaussian",
                   gaussian_sigma=None, k_target=None, pk_target=None, seed=0):
    delta = np.asarray(delta, dtype=np.float64)
    n = delta.shape[0]
    if target_res == n:
        return delta
    if target_res > n:
        if upsample_method == "fourier":
            return fourier_resize(delta, target_res)
        if upsample_method == "linear":
            return trilinear(delta, target_res)
        spec = spectrum_inject(np.fft.rfftn(delta), n, target_res, k_target, pk_target, boxsize, seed)
        return np.fft.irfftn(spec, s=(target_res,) * 3, axes=(0, 1, 2))
    if downsample_method == "fourier":
        return fourier_resize(delta, target_res)
    if downsample_method == "block_average":
        return block_average(delta, target_res)
    sigma = boxsize / target_res if gaussian_sigma is None else gaussian_sigma
    return block_average(gaussian_smooth(delta, boxsize, sigma), target_res)


# ---- test fields ----------------------------------------------------------------------------------------------------------

def red_field(n, seed, dtype=np.float64):
    """A real field with a red spectrum (|delta_k| ~ 1 / |m|), unit variance."""
    w = np.fft.rfftn(np.random.default_rng(seed).standard_normal((n, n, n)))
    _, _, _, q = mode_grid(n)
    x = np.fft.irfftn(w / np.sqrt(np.maximum(q, 1)), s=(n, n, n), axes=(0, 1, 2))
    return (x / x.std()).astype(dtype)


def power_law_table(n_out, boxsize, points=16):
    """A power law of 16 points that ends below the fine Nyquist: the interpolation and the tail are both used."""
    k_nyq = np.pi * n_out / boxsize
    k = np.geomspace(0.5 * 2.0 * np.pi / boxsize, 0.7 * k_nyq, points)
    return k, 2.0e4 * (k / 0.1) ** -1.7
