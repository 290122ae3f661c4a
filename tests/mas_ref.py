"""NumPy float64 reference of jax_nbody_emulator_with_dj_amd.density (mass assignment, window deconvolution, shell-binned
power spectra) with the conventions of the module docstring.  np.add.at on the CPU: small meshes only."""

import numpy as np


def window(x, p):
    """B-spline of order p (1 NGP, 2 CIC, 3 TSC, 4 PCS) at signed distance x, in mesh spacings."""
    a = np.abs(np.asarray(x, dtype=np.float64))
    if p == 1:
        return np.where(a < 0.5, 1.0, np.where(a == 0.5, 0.5, 0.0))
    if p == 2:
        return np.where(a < 1.0, 1.0 - a, 0.0)
    if p == 3:
        return np.where(a < 0.5, 0.75 - a * a, np.where(a < 1.5, 0.5 * (1.5 - a) ** 2, 0.0))
    if p == 4:
        return np.where(a < 1.0, (4.0 - 6.0 * a * a + 3.0 * a ** 3) / 6.0,
                        np.where(a < 2.0, (2.0 - a) ** 3 / 6.0, 0.0))
    raise ValueError(p)


def nodes(u, p):
    """First node and the p weights of the nodes j0 .. j0+p-1 for positions u (mesh units).  NGP takes the node at
    floor(u + 1/2) with weight 1 (half-way points go up, as in the kernel)."""
    u = np.asarray(u, dtype=np.float64)
    j0 = np.floor(u + 1.0 - 0.5 * p).astype(np.int64)
    if p == 1:
        return j0, np.ones(u.shape + (1,))
    w = np.stack([window(u - (j0 + t), p) for t in range(p)], axis=-1)
    return j0, w


def positions(disp, boxsize, res):
    """(3, Np) particle positions in mesh units: lattice q = i L / N plus the displacement, times res / L."""
    disp = np.asarray(disp, dtype=np.float64)
    n = disp.shape[1:]
    L = np.broadcast_to(np.asarray(boxsize, dtype=np.float64), (3,))
    r = np.broadcast_to(np.asarray(res, dtype=np.int64), (3,))
    idx = np.indices(n).reshape(3, -1).astype(np.float64)
    return np.stack([idx[c] * (r[c] / n[c]) + disp[c].reshape(-1) * (r[c] / L[c]) for c in range(3)])


def paint(disp, boxsize, res, worder):
    """(mass, contributors): mass per cell in particle masses (float64) and the number of particles with a non-zero
    weight in each cell."""
    r = tuple(int(v) for v in np.broadcast_to(np.asarray(res, dtype=np.int64), (3,)))
    u = positions(disp, boxsize, r)
    js, ws = zip(*[nodes(u[c], worder) for c in range(3)])
    mass = np.zeros(r)
    count = np.zeros(r, np.int64)
    p = worder
    for a in range(p):
        for b in range(p):
            for c in range(p):
                w = ws[0][:, a] * ws[1][:, b] * ws[2][:, c]
                g = (np.mod(js[0] + a, r[0]), np.mod(js[1] + b, r[1]), np.mod(js[2] + c, r[2]))
                np.add.at(mass, g, w)
                np.add.at(count, g, (w > 0).astype(np.int64))
    return mass, count


def delta_from_mass(mass, nparticles):
    return mass * (mass.size / float(nparticles)) - 1.0


def mas_window(shape, worder):
    """prod_c sinc(pi f_c / res_c)^worder on the rfft grid of a mesh of `shape`."""
    f = [np.fft.fftfreq(shape[0]) , np.fft.fftfreq(shape[1]), np.fft.rfftfreq(shape[2])]
    w = [np.sinc(fc) ** worder for fc in f]               # np.sinc(x) = sin(pi x) / (pi x), f = f_c / res_c
    return w[0][:, None, None] * w[1][None, :, None] * w[2][None, None, :]


def deconvolve(delta, worder):
    d = np.asarray(delta, dtype=np.float64)
    return np.fft.irfftn(np.fft.rfftn(d) / mas_window(d.shape, worder), s=d.shape, axes=(0, 1, 2))


def power(a, boxsize, b=None):
    """(k, P, nmodes) in shells 1 .. n/2 of |k| / k_F, modes of the full grid, P = Re(a_k b_k*) L^3 / n^6."""
    a = np.asarray(a, dtype=np.float64)
    n = a.shape[0]
    A = np.fft.rfftn(a)
    B = A if b is None else np.fft.rfftn(np.asarray(b, dtype=np.float64))
    P = (A * np.conj(B)).real * boxsize ** 3 / float(n) ** 6
    f = np.fft.fftfreq(n) * n
    fz = np.arange(n // 2 + 1, dtype=np.float64)
    kk = np.sqrt(f[:, None, None] ** 2 + f[None, :, None] ** 2 + fz[None, None, :] ** 2)
    shell = np.floor(kk + 0.5).astype(np.int64)
    w = np.full(fz.shape, 2.0)
    w[0] = 1.0
    if n % 2 == 0:
        w[-1] = 1.0
    w = np.broadcast_to(w[None, None, :], kk.shape)
    nb = n // 2
    sel = (shell >= 1) & (shell <= nb)
    cnt = np.bincount(shell[sel], weights=w[sel], minlength=nb + 1)[1:]
    ks = np.bincount(shell[sel], weights=(w * kk)[sel], minlength=nb + 1)[1:]
    ps = np.bincount(shell[sel], weights=(w * P)[sel], minlength=nb + 1)[1:]
    kF = 2.0 * np.pi / boxsize
    return ks / cnt * kF, ps / cnt, cnt


def full_grid_modes(n, shell):
    """Modes of the full n^3 grid in shell `shell`, counted directly (no half-spectrum weights)."""
    f = np.fft.fftfreq(n) * n
    kk = np.sqrt(f[:, None, None] ** 2 + f[None, :, None] ** 2 + f[None, None, :] ** 2)
    return int(np.count_nonzero(np.floor(kk + 0.5) == shell))
