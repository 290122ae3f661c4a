"""Float64 NumPy restatement of the cosmic-web classification and of the mesh readout: the
definitions that nbe_shear_spectrum, nbe_tensor_eigenvalues, nbe_web_classify and nbe_mesh_read, and web.py,
density.read_mesh and halos.halo_environment above them, are held to.  Written from the definitions, not from the kernels:
np.fft with the derivative numbers of lpt2_ref, np.linalg.eigvalsh, counting, and mas_ref's window weights.
"""

import numpy as np

import lpt_ref
import mas_ref
from lpt2_ref import PAIRS, derivative_numbers, hessian_spectrum

NO_TYPE = 255


# ---- tensors ---------------------------------------------------------------------------------------------------------------

def shear_spectrum(spectra, n, boxsize, scale=1.0):
    """(6, n, n, h) complex128: Sigma_ij_k = -scale (1/2) i (2 pi / L) (d_i v_j + d_j v_i) in the order PAIRS."""
    v = np.asarray(spectra, dtype=np.complex128)
    d = derivative_numbers(n)[:3]
    out = np.zeros((6,) + v.shape[1:], np.complex128)
    for p, (i, j) in enumerate(PAIRS):
        out[p] = (-scale * (2.0 * np.pi / boxsize)) * 1j * (0.5 * (d[i] * v[j] + d[j] * v[i]))
    return out


def _inverse(tk, n):
    return np.fft.irfftn(tk, s=(n, n, n), axes=(1, 2, 3))


def tidal_tensor(delta, boxsize=1000.0, smoothing=None):
    """(6, n, n, n) float64: phi,ij of nabla^2 phi = delta, of the Gaussian-smoothed field where `smoothing` is a length."""
    delta = np.asarray(delta, dtype=np.float64)
    n = delta.shape[0]
    spec = np.fft.rfftn(delta)
    if smoothing is not None:
        spec = lpt_ref.gaussian_filter(spec, n, smoothing / boxsize)
    return _inverse(hessian_spectrum(spec, n), n)


def velocity_shear(vmesh, boxsize=1000.0, scale=1.0, smoothing=None):
    v = np.asarray(vmesh, dtype=np.float64)
    n = v.shape[1]
    spec = np.fft.rfftn(v, axes=(1, 2, 3))
    if smoothing is not None:
        spec = np.stack([lpt_ref.gaussian_filter(spec[c], n, smoothing / boxsize) for c in range(3)])
    return _inverse(shear_spectrum(spec, n, boxsize, scale), n)


def divergence(vmesh, boxsize=1000.0):
    """div v with the same derivative: (n, n, n) float64."""
    v = np.asarray(vmesh, dtype=np.float64)
    n = v.shape[1]
    spec = np.fft.rfftn(v, axes=(1, 2, 3))
    d = derivative_numbers(n)[:3]
    theta = 1j * (2.0 * np.pi / boxsize) * (d[0] * spec[0] + d[1] * spec[1] + d[2] * spec[2])
    return np.fft.irfftn(theta, s=(n, n, n), axes=(0, 1, 2))


# ---- eigenvalues and types -------------------------------------------------------------------------------------------------

def matrices(tensor):
    """(..., 3, 3) float64 symmetric matrices of a (6, ...) tensor in the order PAIRS."""
    t = np.asarray(tensor, dtype=np.float64)
    m = np.empty(t.shape[1:] + (3, 3))
    for p, (i, j) in enumerate(PAIRS):
        m[..., i, j] = t[p]
        m[..., j, i] = t[p]
    return m


def frobenius(tensor):
    t = np.asarray(tensor, dtype=np.float64)
    return np.sqrt((t[:3] ** 2).sum(0) + 2.0 * (t[3:] ** 2).sum(0))


def eigenvalues(tensor):
    """(3, ...) float64, lambda_1 >= lambda_2 >= lambda_3 (LAPACK's symmetric solver); three NaNs for a voxel with a
    non-finite word."""
    m = matrices(tensor)
    bad = ~np.isfinite(m).all(axis=(-1, -2))
    lam = np.linalg.eigvalsh(np.where(bad[..., None, None], 0.0, m))[..., ::-1]
    lam = np.where(bad[..., None], np.nan, lam)
    return np.moveaxis(lam, -1, 0)


def web_types(eig, threshold):
    """uint8: the number of eigenvalues > threshold per voxel, NO_TYPE where one is NaN (in the dtype of eig)."""
    eig = np.asarray(eig)
    th = eig.dtype.type(threshold)
    with np.errstate(invalid="ignore"):
        m = (eig > th).sum(0).astype(np.uint8)
    return np.where(np.isnan(eig).any(0), np.uint8(NO_TYPE), m)


def web_counts(eig, thresholds):
    """(T, 5) int64: voxels of type 0 .. 3 and without a type."""
    out = np.zeros((len(thresholds), 5), np.int64)
    for t, th in enumerate(thresholds):
        ty = web_types(eig, th).ravel()
        out[t, :4] = np.bincount(ty[ty != NO_TYPE], minlength=4)
        out[t, 4] = np.count_nonzero(ty == NO_TYPE)
    return out


def mass_fraction(types, mass):
    """(4,) float64: the sum of 1 + mass over the voxels of each type over its sum over all voxels."""
    w = 1.0 + np.asarray(mass, dtype=np.float64)
    return np.array([w[types == m].sum() for m in range(4)]) / w.sum()


# the families whose off-diagonal words are 0: the result is the sorted diagonal itself
EXACT_FAMILIES = ("diagonal", "isotropic", "two equal on the diagonal")


def tensor_families(count, seed):
    """name -> (6, count) float32 tensors: the inputs an eigenvalue method can get wrong."""
    rng = np.random.default_rng(seed)
    normal = lambda *shape: rng.standard_normal(shape)
    out = {"random": normal(6, count)}
    h = normal(6, count); h[3:] = 0.0
    out["diagonal"] = h
    h = np.zeros((6, count)); h[:3] = normal(count)
    out["isotropic"] = h
    v, lam = normal(3, count), normal(count)
    out["rank one"] = np.stack([lam * v[i] * v[j] for i, j in PAIRS])
    # two equal eigenvalues in a rotated frame: a I + b v v^T
    v, a, b = normal(3, count), normal(count), normal(count)
    out["two equal"] = np.stack([a * (i == j) + b * v[i] * v[j] for i, j in PAIRS])
    h = normal(6, count); h[3:] = 0.0; h[1] = h[0]
    out["two equal on the diagonal"] = h
    h = normal(6, count); h[3:] *= 1e-6
    out["nearly diagonal"] = h
    h = np.zeros((6, count)); h[:3] = 1.0; h[3:] = 1e-4 * normal(3, count)
    out["isotropic plus small"] = h
    out["wide range"] = normal(6, count) * 10.0 ** rng.uniform(-6.0, 0.0, (6, count))
    h = normal(6, count)
    h[np.arange(count) % 6, np.arange(count)] = np.where(np.arange(count) % 3 == 0, np.inf, np.nan)
    h[:, ::2] = normal(6, (count + 1) // 2)                # every other voxel stays finite
    out["nan"] = h
    return {k: v.astype(np.float32) for k, v in out.items()}


EIG_BOUND = 2.0 ** -23      # |lambda - exact| <= EIG_BOUND |A|_F: one float32 rounding (2^-24 |A|_F, since |lambda| <= |A|_F)
                            # plus the float64 method's own error, measured at 0.14 of that (csrc/nbe_web.h)


def check_eigenvalues(name, h, eig):
    """Hold float32 eigenvalues `eig` (3, ...) of the float32 tensors `h` (6, ...) to the reference: the bound, the order
    on the bits returned, NaN in exactly where a word is not finite, and == on the families whose off-diagonal words are 0.
    Returns the worst error over the bound."""
    h, eig = np.asarray(h), np.asarray(eig)
    assert eig.dtype == np.float32 and eig.shape == (3,) + h.shape[1:], (name, eig.dtype, eig.shape)
    ref = eigenvalues(h)
    bad = np.isnan(ref[0])
    assert np.array_equal(np.isnan(eig), np.broadcast_to(bad, eig.shape)), name
    assert np.array_equal(bad, ~np.isfinite(h).all(0)), name
    ok = ~bad
    assert (eig[0][ok] >= eig[1][ok]).all() and (eig[1][ok] >= eig[2][ok]).all(), name
    err = np.abs(eig.astype(np.float64) - ref)[:, ok].max(0) if ok.any() else np.zeros(0)
    bound = EIG_BOUND * frobenius(h)[ok]
    assert (err <= bound).all(), (name, float((err / np.maximum(bound, 1e-300)).max()))
    if not np.any(h[3:]):
        assert np.array_equal(eig, np.sort(h[:3], axis=0)[::-1]), name
    return float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0


def plane_wave(n, m, amp=0.3):
    """delta = amp cos(2 pi m.x / L) on the mesh, for an integer wave vector m: its tidal tensor is delta m_i m_j / |m|^2,
    with the eigenvalues (delta, 0, 0) sorted."""
    i = np.indices((n, n, n)).astype(np.float64)
    return amp * np.cos(2.0 * np.pi * (m[0] * i[0] + m[1] * i[1] + m[2] * i[2]) / n)


# ---- the mesh readout ------------------------------------------------------------------------------------------------------

def read_mesh(field, u, worder):
    """(C, count) float64: sum over the worder^3 nodes of the window weights times the field, at positions u (count, 3) in
    mesh units on a periodic mesh."""
    f = np.asarray(field, dtype=np.float64)
    f = f.reshape((-1,) + f.shape[-3:])
    r = f.shape[1:]
    u = np.asarray(u, dtype=np.float64)
    js, ws = zip(*[mas_ref.nodes(u[:, c], worder) for c in range(3)])
    out = np.zeros((f.shape[0], u.shape[0]))
    for a in range(worder):
        for b in range(worder):
            for c in range(worder):
                w = ws[0][:, a] * ws[1][:, b] * ws[2][:, c]
                g = (np.mod(js[0] + a, r[0]), np.mod(js[1] + b, r[1]), np.mod(js[2] + c, r[2]))
                out += w[None, :] * f[:, g[0], g[1], g[2]]
    return out
