"""NumPy float64 reference of density.paint_field: weighted mass assignment with the weights of mas_ref (np.add.at on the
CPU: small meshes only), the error bounds of the integer scheme, and the checks the CPU and GPU tests share."""

import numpy as np

import mas_ref as R

UNIT = 2.0 ** -22


def paint(disp, quantity, boxsize, res, worder):
    """(num, mass, count, absq) per cell.  disp: (3, N0, N1, N2) or None (the undisplaced lattice); quantity: (C, N0, N1, N2)
    or (N0, N1, N2).  num[c] = sum of w q_c, mass = sum of w (particle masses), count = particles with a non-zero weight,
    absq[c] = sum of |q_c| over those particles; all float64 (count int64), num and absq of shape (C,) + res."""
    q = np.asarray(quantity, dtype=np.float64)
    if q.ndim == 3:
        q = q[None]
    n = q.shape[1:]
    if disp is None:
        disp = np.zeros((3,) + n)
    r = tuple(int(v) for v in np.broadcast_to(np.asarray(res, dtype=np.int64), (3,)))
    u = R.positions(disp, boxsize, r)
    js, ws = zip(*[R.nodes(u[c], worder) for c in range(3)])
    qf = q.reshape(q.shape[0], -1)
    num = np.zeros((q.shape[0],) + r)
    absq = np.zeros((q.shape[0],) + r)
    mass = np.zeros(r)
    count = np.zeros(r, np.int64)
    p = worder
    for a in range(p):
        for b in range(p):
            for c in range(p):
                w = ws[0][:, a] * ws[1][:, b] * ws[2][:, c]
                g = (np.mod(js[0] + a, r[0]), np.mod(js[1] + b, r[1]), np.mod(js[2] + c, r[2]))
                hit = w > 0
                np.add.at(mass, g, w)
                np.add.at(count, g, hit.astype(np.int64))
                for ch in range(q.shape[0]):
                    np.add.at(num[ch], g, w * qf[ch])
                    np.add.at(absq[ch], g, hit * np.abs(qf[ch]))
    return num, mass, count, absq


def exponents(quantity):
    """(A_c, e_c) per channel: the largest magnitude and the binary exponent with A_c < 2^e_c (0 for a zero channel)."""
    q = np.asarray(quantity)
    if q.ndim == 3:
        q = q[None]
    A = np.abs(q.reshape(q.shape[0], -1).astype(np.float64)).max(axis=1)
    return A, np.frexp(A)[1].astype(np.int64)


def numerator_bound(A, e, mass, count):
    """The tests' bound on a cell's numerator before the float32 rounding: 4 2^-22 A count + m 2^(e - 24).  (The scheme's
    own bound is 2^-22 sum |q_p| + m 2^(e - 25): a weight is within 2^-22 of exact and |q| <= A; a value is rounded at
    2^(e - 25) and the weights of a cell sum to m.)"""
    return 4 * UNIT * A * count + mass * 2.0 ** (e - 24)


def check_mean(field, quantity, ref, nparticles):
    """normalize="mean": every cell of every channel within the numerator bound + 2e-7 |ref| (the float32 rounding)."""
    num, mass, count, _ = ref
    A, e = exponents(quantity)
    f = np.asarray(field)
    f = f[None] if f.ndim == 3 else f
    assert f.dtype == np.float32 and f.shape == num.shape
    g = f.astype(np.float64) * (nparticles / mass.size)
    worst = 0.0
    for c in range(num.shape[0]):
        err = np.abs(g[c] - num[c])
        bound = numerator_bound(A[c], e[c], mass, count) + 2e-7 * np.abs(num[c])
        assert (err <= bound + 1e-300).all(), (c, err.max(), np.unravel_index(np.argmax(err - bound), err.shape))
        worst = max(worst, float((err / np.maximum(bound, 1e-300)).max()))
    return worst


def check_density(field, quantity, ref):
    """normalize="density" with fill = 0, cross-multiplied so that no cell is left out (a cell whose mass is below the
    weights' resolution has no meaningful ratio, but g m is still bounded): |g m - num| <= E_num + |g| 4 2^-22 count +
    2e-7 |g| m, and |g| <= 2^e."""
    num, mass, count, _ = ref
    A, e = exponents(quantity)
    f = np.asarray(field)
    f = f[None] if f.ndim == 3 else f
    assert f.dtype == np.float32 and f.shape == num.shape
    g = f.astype(np.float64)
    for c in range(num.shape[0]):
        ga = np.abs(g[c])
        err = np.abs(g[c] * mass - num[c])
        bound = numerator_bound(A[c], e[c], mass, count) + ga * 4 * UNIT * count + 2e-7 * ga * mass
        assert (err <= bound + 1e-300).all(), (c, (err - bound).max(), np.unravel_index(np.argmax(err - bound), err.shape))
        assert (ga <= 2.0 ** e[c]).all()
        assert (f[c][count == 0] == 0).all()


def emulate(disp, quantity, boxsize, res, worder, normalize="density", fill=0.0):
    """The integer scheme of paint_field restated in NumPy (int64 sums, float64 conversion, one rounding to float32), for
    CPU tests of the bounds above: (field (C,) + res float32, integer mass mesh)."""
    q = np.asarray(quantity, dtype=np.float64)
    q = q[None] if q.ndim == 3 else q
    n = q.shape[1:]
    if disp is None:
        disp = np.zeros((3,) + n)
    r = tuple(int(v) for v in np.broadcast_to(np.asarray(res, dtype=np.int64), (3,)))
    u = R.positions(disp, boxsize, r)
    js, ws = zip(*[R.nodes(u[c], worder) for c in range(3)])
    _, e = exponents(q)
    V = [np.rint(np.ldexp(q[c].reshape(-1), 24 - int(e[c]))).astype(np.int64) for c in range(q.shape[0])]
    mass = np.zeros(r, np.int64)
    S = np.zeros((q.shape[0],) + r, np.int64)
    acc = np.zeros(u.shape[1])
    prev = np.zeros(u.shape[1], np.int64)
    p = worder
    for a in range(p):
        for b in range(p):
            wab = ws[0][:, a] * ws[1][:, b]
            for c in range(p):
                acc = acc + wab * ws[2][:, c]
                cum = np.rint(acc * 2.0 ** 22).astype(np.int64)
                wi, prev = cum - prev, cum
                g = (np.mod(js[0] + a, r[0]), np.mod(js[1] + b, r[1]), np.mod(js[2] + c, r[2]))
                np.add.at(mass, g, wi)
                for ch in range(q.shape[0]):
                    np.add.at(S[ch], g, wi * V[ch])
    out = np.empty(S.shape, np.float32)
    for ch in range(q.shape[0]):
        if normalize == "mean":
            out[ch] = np.ldexp(S[ch].astype(np.float64), int(e[ch]) - 46) * (mass.size / float(u.shape[1]))
        else:
            with np.errstate(invalid="ignore", divide="ignore"):
                out[ch] = np.where(mass == 0, fill, np.ldexp(S[ch].astype(np.float64), int(e[ch]) - 24) / mass)
    return out, mass
