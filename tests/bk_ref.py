"""Float64 NumPy restatements of density.bispectrum, written from its definition (include/nbe.h, "Reduced bispectrum").

Two independent forms:
(a) `direct`: enumerates the modes of shells 1 and 2, forms m3 = -(m1 + m2) for every pair and, per theta, sums
    Re(delta_m1 delta_m2 delta_m3) and counts the pairs whose m3 lies in the third shell.  No transform of a filtered
    field, nothing shared with the device path.
(b) `fft_form`: F_S = irfftn(delta I_S), G_S = irfftn(I_S); n^6 sum_x F1 F2 F3 is the sum over the triangles and
    n^6 sum_x G1 G2 G3 their number.  Reaches sizes that (a) cannot; with dtype=float32 (scipy.fft keeps float32) it is
    the yardstick for the rounding of a single-precision pipeline.

Conventions: kappa = k / k_F, k_F = 2 pi / L; m runs over the full complex grid, each component in (-n/2, n/2]; delta_m is
the unnormalised forward FFT."""

import numpy as np


def kappa3(kappa1, kappa2, theta):
    theta = np.asarray(theta, dtype=np.float64)
    return np.sqrt((kappa2 * np.sin(theta)) ** 2 + (kappa2 * np.cos(theta) + kappa1) ** 2)


def in_shell(q, kappa, dk):
    """Whether the integer |m|^2 = q lies in S(kappa): lo^2 <= q < hi^2 in float64, and never the DC mode."""
    lo = max(kappa - 0.5 * dk, 0.0)
    hi = kappa + 0.5 * dk
    q = np.asarray(q)
    return (q.astype(np.float64) >= lo * lo) & (q.astype(np.float64) < hi * hi) & (q > 0)


def grid_modes(n):
    """Frequencies of the full grid along one axis, in FFT order: components in (-n/2, n/2]."""
    f = np.arange(n)
    return np.where(f <= n // 2, f, f - n)


def shell_modes(n, kappa, dk):
    """(count, 3) int64 wave vectors of S(kappa) on the full n^3 grid."""
    f = grid_modes(n)
    mx, my, mz = np.meshgrid(f, f, f, indexing="ij")
    sel = in_shell(mx * mx + my * my + mz * mz, kappa, dk)
    return np.stack([mx[sel], my[sel], mz[sel]], axis=1).astype(np.int64)


def shell_stats(x, boxsize, kappas, dk):
    """Per shell over the full grid: mean |k|, mean P = |delta_m|^2 L^3 / n^6, mode count (NaN, NaN, 0 when empty)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    d = np.fft.fftn(x)
    f = grid_modes(n)
    mx, my, mz = np.meshgrid(f, f, f, indexing="ij")
    q = mx * mx + my * my + mz * mz
    p = (d.real ** 2 + d.imag ** 2) * (boxsize ** 3 / float(n) ** 6)
    kk = np.sqrt(q.astype(np.float64)) * (2.0 * np.pi / boxsize)
    k, pk, nm = [], [], []
    for ka in kappas:
        sel = in_shell(q, ka, dk)
        c = int(sel.sum())
        nm.append(c)
        k.append(kk[sel].mean() if c else np.nan)
        pk.append(p[sel].mean() if c else np.nan)
    return np.array(k), np.array(pk), np.array(nm, dtype=np.int64)


def direct(x, kappa1, kappa2, theta, dk):
    """(sums, counts) per theta by enumeration: sums = sum over the triangles of Re(delta_m1 delta_m2 delta_m3) (float64),
    counts = N_tri (int64)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    d = np.fft.fftn(x)
    m1, m2 = shell_modes(n, kappa1, dk), shell_modes(n, kappa2, dk)
    m3 = -(m1[:, None, :] + m2[None, :, :])                          # closes exactly; inside the grid for valid arguments
    assert (np.abs(m3) < n / 2).all(), "a closing vector leaves the grid: the arguments violate the closure condition"
    q3 = (m3 * m3).sum(axis=2)
    d1 = d[m1[:, 0] % n, m1[:, 1] % n, m1[:, 2] % n]
    d2 = d[m2[:, 0] % n, m2[:, 1] % n, m2[:, 2] % n]
    d3 = d[m3[..., 0] % n, m3[..., 1] % n, m3[..., 2] % n]
    term = ((d1[:, None] * d2[None, :]) * d3).real
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    sums, counts = np.zeros(theta.size), np.zeros(theta.size, np.int64)
    for t, ka in enumerate(kappa3(kappa1, kappa2, theta)):
        sel = in_shell(q3, ka, dk)
        counts[t] = sel.sum()
        sums[t] = term[sel].sum()
    return sums, counts


def fft_form(x, kappa1, kappa2, theta, dk, dtype=np.float64):
    """(sums, counts, A) per theta by the FFT estimator in `dtype`: sums = n^6 sum_x F1 F2 F3, counts = n^6 sum_x G1 G2 G3
    (floats; round them), A = n^6 sum_x |F1 F2 F3|, the scale of the rounding error of the sums.  The products of the
    real fields are always accumulated in float64; the transforms run in `dtype`."""
    import scipy.fft as sf
    dtype = np.dtype(dtype)
    x = np.asarray(x, dtype=dtype)
    n = x.shape[0]
    d = sf.rfftn(x)
    assert d.dtype == (np.complex64 if dtype == np.float32 else np.complex128)
    f = grid_modes(n)
    mx, my, mz = np.meshgrid(f, f, np.arange(n // 2 + 1), indexing="ij")
    q = mx * mx + my * my + mz * mz

    def pair(ka):
        ind = in_shell(q, ka, dk)
        F = sf.irfftn(np.where(ind, d, 0).astype(d.dtype), s=(n, n, n))
        G = sf.irfftn(ind.astype(d.dtype), s=(n, n, n))
        return F.astype(np.float64), G.astype(np.float64)

    F1, G1 = pair(kappa1)
    F2, G2 = pair(kappa2)
    F12, G12 = F1 * F2, G1 * G2
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    sums, counts, A = np.zeros(theta.size), np.zeros(theta.size), np.zeros(theta.size)
    n6 = float(n) ** 6
    for t, ka in enumerate(kappa3(kappa1, kappa2, theta)):
        F3, G3 = pair(ka)
        sums[t] = n6 * (F12 * F3).sum()
        A[t] = n6 * np.abs(F12 * F3).sum()
        counts[t] = n6 * (G12 * G3).sum()
    return sums, counts, A


def bispectrum(x, boxsize, k1, k2, theta, dk, sums=None, counts=None):
    """The dict of density.bispectrum from the direct form (or from given sums and counts)."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    kF = 2.0 * np.pi / boxsize
    ka1, ka2 = k1 / kF, k2 / kF
    theta = np.atleast_1d(np.asarray(theta, dtype=np.float64))
    if sums is None:
        sums, counts = direct(x, ka1, ka2, theta, dk)
    ka3 = kappa3(ka1, ka2, theta)
    k, pk, nm = shell_stats(x, boxsize, np.concatenate([[ka1, ka2], ka3]), dk)
    with np.errstate(invalid="ignore", divide="ignore"):
        B = np.where(counts > 0, sums * (boxsize ** 6 / float(n) ** 9) / counts, np.nan)
        Q = B / (pk[0] * pk[1] + pk[1] * pk[2:] + pk[2:] * pk[0])
    return {"theta": theta, "k3": ka3 * kF, "B": B, "Q": Q, "ntriangles": np.asarray(counts, np.int64), "pk": pk, "k": k,
            "nmodes": nm}


def quadratic_field(n, seed):
    """g + 0.3 (g^2 - 1) of white noise g: non-Gaussian, so that B != 0.  float32."""
    g = np.random.default_rng(seed).standard_normal((n, n, n))
    return (g + 0.3 * (g * g - 1.0)).astype(np.float32)
