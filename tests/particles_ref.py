"""NumPy float64 reference of density.paint_particles: mass assignment of explicit positions with the weights of mas_ref
(np.add.at on the CPU: small meshes only), and the integer scheme restated for CPU tests of its order independence."""

import numpy as np

import field_ref as F
import mas_ref as R


def lattice_positions(disp, boxsize):
    """(count, 3) float64 positions q + psi of a (3, N0, N1, N2) displacement, rows in lattice order."""
    disp = np.asarray(disp, dtype=np.float64)
    n = disp.shape[1:]
    L = np.broadcast_to(np.asarray(boxsize, dtype=np.float64), (3,))
    idx = np.indices(n).reshape(3, -1).astype(np.float64)
    return np.stack([idx[c] * (L[c] / n[c]) + disp[c].reshape(-1) for c in range(3)], axis=1)


def mesh_coordinates(pos, boxsize, res, shift=None):
    """(3, count) positions in mesh units, u_c = x_c res_c / L_c; shift = (axis, values, scale) adds values * scale *
    res / L along that axis."""
    pos = np.asarray(pos, dtype=np.float64)
    L = np.broadcast_to(np.asarray(boxsize, dtype=np.float64), (3,))
    r = np.broadcast_to(np.asarray(res, dtype=np.int64), (3,))
    u = np.stack([pos[:, c] * (r[c] / L[c]) for c in range(3)])
    if shift is not None:
        axis, values, scale = shift
        u[axis] = u[axis] + np.asarray(values, dtype=np.float64) * (scale * (r[axis] / L[axis]))
    return u


def _channels(count, weights, quantity):
    if weights is not None and quantity is not None:
        raise ValueError("weights or a quantity, not both")
    q = weights if weights is not None else quantity
    if q is None:
        return np.zeros((0, count))
    q = np.asarray(q, dtype=np.float64)
    return q[None] if q.ndim == 1 else q


def paint(pos, boxsize, res, worder, weights=None, quantity=None, shift=None):
    """(num, mass, count, absq) per cell, as field_ref.paint: num[c] = sum of w q_c with the weights (channel 0) or the
    (C, count) quantity as q, mass = sum of w (particle masses), count = particles with a non-zero weight, absq[c] = sum
    of |q_c| over those; float64 (count int64), num and absq of shape (C,) + res with C = 0 without weights or quantity."""
    r = tuple(int(v) for v in np.broadcast_to(np.asarray(res, dtype=np.int64), (3,)))
    u = mesh_coordinates(pos, boxsize, r, shift)
    q = _channels(u.shape[1], weights, quantity)
    js, ws = zip(*[R.nodes(u[c], worder) for c in range(3)])
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
                    np.add.at(num[ch], g, w * q[ch])
                    np.add.at(absq[ch], g, hit * np.abs(q[ch]))
    return num, mass, count, absq


def emulate(pos, boxsize, res, worder, weights=None, quantity=None, shift=None):
    """The integer meshes of nbe_paint_particles restated in NumPy: (mass, S), int64, mass in units of 2^-22 particle
    masses and S[c] = sum of w V with V = rint(q 2^(24 - e_c)) (field_ref.exponents)."""
    r = tuple(int(v) for v in np.broadcast_to(np.asarray(res, dtype=np.int64), (3,)))
    u = mesh_coordinates(pos, boxsize, r, shift)
    q = _channels(u.shape[1], weights, quantity)
    js, ws = zip(*[R.nodes(u[c], worder) for c in range(3)])
    e = F.exponents(q[:, :, None, None])[1] if q.shape[0] else []
    V = [np.rint(np.ldexp(q[c], 24 - int(e[c]))).astype(np.int64) for c in range(q.shape[0])]
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
    return mass, S


def weighted_delta(S0):
    """sum(w m) / mean - 1 from the integer mesh of the weight channel: float64, one rounding to float32."""
    total = int(np.sum(S0.astype(object)))
    return (S0.astype(np.float64) * (S0.size / float(total)) - 1.0).astype(np.float32)
