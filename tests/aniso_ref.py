"""Float64 NumPy restatement of the anisotropic two-point calls: the multipoles and (k, mu) wedges
of jax_nbody_emulator_with_dj_amd.density, the integer scheme their kernels carry the sums in, and lpt.divergence.
Written from the definitions, not from the kernels.  Shells, weights and the isotropic sums are mas_ref.power's; wave
numbers are lpt_ref.mode_grid's."""

import numpy as np

import mas_ref
from lpt_ref import full_grid_weight, mode_grid, red_field

KEXP = 36                                   # |k| and |mu| sums are in units of 2^-36


def legendre(mu2):
    """(L_0, L_2, L_4) of mu, from mu^2."""
    return np.ones_like(mu2), (3.0 * mu2 - 1.0) / 2.0, (35.0 * (mu2 * mu2) - 30.0 * mu2 + 3.0) / 8.0


def mu_bin(m_los, q, nmu):
    """The wedge of a mode by the integer rule: min(nmu - 1, #{ j in 1 .. nmu-1 : j^2 q <= nmu^2 m_los^2 })."""
    m_los, q = np.asarray(m_los, dtype=np.int64), np.asarray(q, dtype=np.int64)
    t = nmu * nmu * m_los * m_los
    count = np.zeros(np.broadcast(m_los, q).shape, np.int64)
    for j in range(1, nmu):
        count += j * j * q <= t
    return np.minimum(nmu - 1, count)


def modes(n, los):
    """Per mode of the half spectrum, flattened and restricted to the binned shells 1 .. n//2: (index into the flattened
    half spectrum, shell, full-grid weight, |m|, m_los, q)."""
    m = mode_grid(n)
    shape = (n, n, n // 2 + 1)
    q = np.broadcast_to(m[3], shape).ravel()
    m_los = np.broadcast_to(m[los], shape).ravel()
    w = np.broadcast_to(full_grid_weight(n), shape).ravel()
    kk = np.sqrt(q.astype(np.float64))
    shell = np.floor(kk + 0.5).astype(np.int64)
    idx = np.flatnonzero((shell >= 1) & (shell <= n // 2))
    return idx, shell[idx], w[idx], kk[idx], m_los[idx], q[idx]


def _term(a, boxsize, b):
    """Re(a_k b_k*) L^3 / n^6 on the flattened half spectrum of the float64 fields."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    A = np.fft.rfftn(a)
    B = A if b is None else np.fft.rfftn(np.asarray(b, dtype=np.float64))
    return n, ((A * np.conj(B)).real * boxsize ** 3 / float(n) ** 6).ravel()


def multipoles(a, boxsize, los, b=None):
    """dict(k, p0, p2, p4, nmodes): P_l = (2 l + 1) sum(w P L_l(mu)) / sum(w) over the shells of mas_ref.power."""
    n, P = _term(a, boxsize, b)
    k, p0, cnt = mas_ref.power(a, boxsize, b)
    idx, shell, w, kk, m_los, q = modes(n, los)
    L = legendre((m_los * m_los).astype(np.float64) / q.astype(np.float64))
    out = dict(k=k, p0=p0, nmodes=cnt)
    for ell in (2, 4):
        s = np.bincount(shell, weights=w * P[idx] * L[ell // 2], minlength=n // 2 + 1)[1:]
        out["p%d" % ell] = (2 * ell + 1) * s / cnt
    return out


def wedges(a, boxsize, los, nmu, b=None):
    """dict(k, mu, pk, nmodes, mu_edges): the means over the modes of each (mu bin, shell), (nmu, n // 2); NaN where a bin
    holds no mode."""
    n, P = _term(a, boxsize, b)
    idx, shell, w, kk, m_los, q = modes(n, los)
    nb = n // 2 + 1
    cell = mu_bin(m_los, q, nmu) * nb + shell
    mu = np.abs(m_los) / kk

    def total(x):
        return np.bincount(cell, weights=w * x, minlength=nmu * nb).reshape(nmu, nb)[:, 1:]

    cnt = total(np.ones(len(idx)))
    with np.errstate(invalid="ignore", divide="ignore"):
        return dict(k=total(kk) / cnt * (2.0 * np.pi / boxsize), mu=total(mu) / cnt, pk=total(P[idx]) / cnt, nmodes=cnt,
                    mu_edges=np.arange(nmu + 1) / nmu)


def integer_sums(spec, n, los, b=None, nmu=None):
    """The integer scheme for a complex64 half spectrum `spec` (and `b`): dict(binmax, multipoles[, wedges]).

    binmax: (n//2+1) uint32, the float32 bits of each shell's largest |p|, p = Re(spec b*) formed in float64 from the
    float32 parts.  With e the binary exponent of that word (m 2^e, m in [0.5, 1); 0 for an empty word), a power term of
    the shell is rint(ldexp(p L, 32 - e)), and 0 in a shell whose word is not finite.  multipoles: (5, n//2+1) int64, the
    sums of w, w rint((|m| - s) 2^36) and w times the terms for L_0, L_2, L_4.  wedges (with nmu): (4, nmu, n//2+1) int64,
    the sums of w, the same k word, w rint(|mu| 2^36) and w times the term."""
    spec = np.asarray(spec, dtype=np.complex64).reshape(-1)
    other = spec if b is None else np.asarray(b, dtype=np.complex64).reshape(-1)
    idx, shell, w, kk, m_los, q = modes(n, los)
    x, y = spec[idx], other[idx]
    p = x.real.astype(np.float64) * y.real.astype(np.float64) + x.imag.astype(np.float64) * y.imag.astype(np.float64)
    nb = n // 2 + 1
    binmax = np.zeros(nb, np.float32)
    np.maximum.at(binmax, shell, np.abs(p).astype(np.float32))     # a NaN term makes the word NaN, as it must
    finite = np.isfinite(binmax)
    _, e = np.frexp(np.where(finite & (binmax > 0), binmax, 1.0).astype(np.float64))
    e = np.where(finite & (binmax > 0), e, 0)

    def units(term):
        with np.errstate(invalid="ignore", over="ignore"):
            u = np.rint(np.ldexp(term, 32 - e[shell]))
        return np.where(finite[shell], u, 0.0).astype(np.int64)

    def total(cell, cells, value):
        out = np.zeros(cells, np.int64)
        np.add.at(out, cell, w * value)
        return out

    kq = np.rint((kk - shell) * 2.0 ** KEXP).astype(np.int64)
    L = legendre((m_los * m_los).astype(np.float64) / q.astype(np.float64))
    one = np.ones(len(idx), np.int64)
    out = dict(binmax=binmax.view(np.uint32),
               multipoles=np.stack([total(shell, nb, v) for v in (one, kq, units(p), units(p * L[1]), units(p * L[2]))]))
    if nmu is not None:
        cell = mu_bin(m_los, q, nmu) * nb + shell
        muq = np.rint(np.abs(m_los) / kk * 2.0 ** KEXP).astype(np.int64)
        out["wedges"] = np.stack([total(cell, nmu * nb, v) for v in (one, kq, muq, units(p))]).reshape(4, nmu, nb)
    return out


def divergence(field, boxsize):
    """div v of a (3, n, n, n) field by the spectral derivative, float64: theta_k = i (2 pi / L) sum_c m_c v_c, where
    component c is left out on its own Nyquist row (n even, |m_c| = n/2)."""
    field = np.asarray(field, dtype=np.float64)
    n = field.shape[1]
    spec = np.fft.rfftn(field, axes=(1, 2, 3))
    m = mode_grid(n)
    mc = [np.where((n % 2 == 0) & (np.abs(m[c]) == n // 2), 0, m[c]) for c in range(3)]
    theta = 1j * (2.0 * np.pi / boxsize) * ((mc[0] * spec[0] + mc[1] * spec[1]) + mc[2] * spec[2])
    return np.fft.irfftn(theta, s=(n, n, n), axes=(0, 1, 2))


# ---- test fields ----------------------------------------------------------------------------------------------------------

def anisotropic_field(n, seed, los, dtype=np.float32):
    """lpt_ref.red_field times (1 + mu^2 / 2) about `los` in Fourier space: a field whose l = 2, 4 are not noise."""
    m = mode_grid(n)
    mu2 = (m[los] * m[los]) / np.maximum(m[3], 1).astype(np.float64)
    x = np.fft.irfftn(np.fft.rfftn(red_field(n, seed)) * (1.0 + 0.5 * mu2), s=(n, n, n), axes=(0, 1, 2))
    return x.astype(dtype)


def plane_wave(n, m, amplitude=1.0):
    """amplitude cos(2 pi m . x / n) on an n^3 grid, float64."""
    i = np.arange(n)
    phase = m[0] * i[:, None, None] + m[1] * i[None, :, None] + m[2] * i[None, None, :]
    return amplitude * np.cos(2.0 * np.pi * phase / n)
