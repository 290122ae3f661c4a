"""The cosmic-web classification on the MI355X (web.py and the entry points nbe_shear_spectrum, nbe_tensor_eigenvalues and
nbe_web_classify behind it) against the float64 restatement tests/web_ref.py.

Bounds.  Eigenvalues: |lambda - exact| <= 2^-23 |A|_F per voxel (one float32 rounding of at most 2^-24 |A|_F plus the float64
method's own error, 0.14 of that on the host walk of tests/test_web_host_walk.py), the order on the bits returned, == where
the off-diagonal words are 0.  Types and counts: exact integers from the returned float32 words.  The shear pass: 2^-22 of the
float64 term per word, the bound of test_gpu_lpt2.py's Hessian pass.  Whole calls: test_gpu_lpt.py's relative L2 of 1e-5."""

import ctypes as C

import numpy as np
import pytest

import web_ref as W
from lpt2_ref import PAIRS, derivative_numbers
from lpt_ref import red_field

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = 250.0


def _torch():
    import torch
    return torch


def _web():
    from jax_nbody_emulator_with_dj_amd import web
    return web


def _abi():
    from jax_nbody_emulator_with_dj_amd import _lib
    return _lib


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def ptr(t):
    return C.c_void_p(t.data_ptr())


def mixed_tensor(n, seed):
    """(6, n, n, n) float32: voxel i takes family i % F of web_ref.tensor_families, so that every family meets every path."""
    fams = list(W.tensor_families(n ** 3, seed).values())
    i = np.arange(n ** 3)
    h = np.stack(fams)[i % len(fams), :, i].T
    return np.ascontiguousarray(h.reshape(6, n, n, n))


def eigenvalues_abi(t, n, max_blocks=0):
    torch = _torch()
    eig = torch.full((3, n, n, n), 7.0, dtype=torch.float32, device="cuda")
    _abi().check(_abi().lib().nbe_tensor_eigenvalues(ptr(t), n, ptr(eig), max_blocks, None))
    return eig.cpu().numpy()


def classify_abi(eig, n, th, which=0, want_types=True, max_blocks=0):
    torch = _torch()
    counts = torch.zeros((len(th), 5), dtype=torch.int64, device="cuda")
    types = torch.full((n, n, n), 9, dtype=torch.uint8, device="cuda") if want_types else None
    arr = (C.c_float * len(th))(*[float(v) for v in th])
    _abi().check(_abi().lib().nbe_web_classify(ptr(eig), n, arr, len(th), which, ptr(types) if want_types else None,
                                               ptr(counts), max_blocks, None))
    return counts.cpu().numpy(), None if types is None else types.cpu().numpy()


# ---- eigenvalues -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 5, 8, 12, 33])
def test_eigenvalues_vs_reference(n):
    """2, 8, 12: the 16-byte path; 3, 5, 33: no aligned form (33: a ragged tail over 141 workgroups).  Every family of the
    host walk in one mesh; a capped grid makes the loop wrap and gives the same bits."""
    torch = _torch()
    h = mixed_tensor(n, 400 + n)
    t = torch.from_numpy(h).cuda()
    eig = eigenvalues_abi(t, n)
    worst = W.check_eigenvalues("mixed %d" % n, h.reshape(6, -1), eig.reshape(3, -1))
    print("n %d: worst error / bound %.3f" % (n, worst))
    for blocks in (1, 3):
        assert same_bits(eigenvalues_abi(t, n, blocks), eig)
    assert same_bits(_web().tensor_eigenvalues(h), eig) and same_bits(_web().tensor_eigenvalues(t).cpu().numpy(), eig)


@pytest.mark.parametrize("n", [5, 8])
def test_eigenvalues_exact_families_and_nan(n):
    torch = _torch()
    fams = W.tensor_families(n ** 3, 9)
    for name in W.EXACT_FAMILIES + ("nan",):
        h = fams[name]
        eig = eigenvalues_abi(torch.from_numpy(h).cuda(), n).reshape(3, -1)
        W.check_eigenvalues(name, h, eig)
        if name != "nan":
            assert np.array_equal(eig, np.sort(h[:3], axis=0)[::-1])
        else:
            assert np.isnan(eig).any() and not np.isnan(eig).all()


def test_eigenvalues_unaligned_pointers_take_the_narrow_path():
    """An even n whose tensor starts 4 bytes past a 16-byte boundary: the same bits as the aligned call."""
    torch = _torch()
    n = 8
    h = mixed_tensor(n, 77)
    big = torch.zeros(6 * n ** 3 + 1, dtype=torch.float32, device="cuda")
    big[1:] = torch.from_numpy(h).cuda().reshape(-1)
    shifted = big[1:]
    assert shifted.data_ptr() % 16 == 4
    eig = torch.empty((3, n, n, n), dtype=torch.float32, device="cuda")
    _abi().check(_abi().lib().nbe_tensor_eigenvalues(ptr(shifted), n, ptr(eig), 0, None))
    assert same_bits(eig.cpu().numpy(), eigenvalues_abi(torch.from_numpy(h).cuda(), n))


# ---- classification --------------------------------------------------------------------------------------------------------

def gaussian_tensor(n, seed):
    """The float32 tidal tensor of a smoothed red field (the reference's), with a few voxels made non-finite."""
    t = W.tidal_tensor(red_field(n, seed), L, smoothing=2.0 * L / n).astype(np.float32)
    flat = t.reshape(6, -1)
    flat[0, 5::997] = np.nan
    flat[4, 11::1499] = np.inf
    return t


@pytest.mark.parametrize("n, T", [(12, 1), (12, 3), (12, 64), (33, 1), (33, 3), (33, 64), (5, 8), (2, 9)])
def test_classification_is_exact(n, T):
    torch = _torch()
    h = gaussian_tensor(n, 30 + n)
    t = torch.from_numpy(h).cuda()
    eig_d = torch.empty((3, n, n, n), dtype=torch.float32, device="cuda")
    _abi().check(_abi().lib().nbe_tensor_eigenvalues(ptr(t), n, ptr(eig_d), 0, None))
    eig = eig_d.cpu().numpy()
    sd = float(np.nanstd(eig))
    th = np.linspace(-1.0, 1.5, T).astype(np.float32) * np.float32(sd) if T > 1 else np.array([0.0], np.float32)
    which = T // 2
    counts, types = classify_abi(eig_d, n, th, which)
    nan = np.isnan(eig).any(0)
    assert nan.sum() == np.count_nonzero(~np.isfinite(h).all(0)) > 0
    want = np.where(nan, 255, (eig > th[which]).sum(0)).astype(np.uint8)
    assert types.dtype == np.uint8 and np.array_equal(types, want)
    for t_i in range(T):
        ty = np.where(nan, 255, (eig > th[t_i]).sum(0))
        assert counts[t_i, :4].tolist() == np.bincount(ty[~nan], minlength=4).tolist()
        assert counts[t_i, 4] == nan.sum()
    assert np.array_equal(counts, W.web_counts(eig, th))
    for blocks in (1, 2):
        c2, t2 = classify_abi(eig_d, n, th, which, max_blocks=blocks)
        assert np.array_equal(c2, counts) and np.array_equal(t2, types)
    c3, t3 = classify_abi(eig_d, n, th, which, want_types=False)
    assert t3 is None and np.array_equal(c3, counts)
    out = _web().classify_web(eig, threshold=th, which=which)
    assert np.array_equal(out["counts"], counts) and np.array_equal(out["types"], types) and out["thresholds"].dtype == np.float32
    vf = out["volume_fraction"]
    assert vf.shape == (T, 4) and vf.dtype == np.float64
    assert np.abs(vf.sum(1) - (1.0 - nan.sum() / float(n) ** 3)).max() < 1e-15
    assert "types" not in _web().classify_web(eig_d, threshold=th, return_types=False)


def test_types_agree_with_the_float64_reference_away_from_the_threshold():
    """Every voxel whose reference eigenvalues all lie farther than the eigenvalue bound from the threshold must get the
    reference's type; for a Gaussian field at 33^3 about 1e-6 of the voxels lie closer, and at most 1e-3 may."""
    torch = _torch()
    n = 33
    h = gaussian_tensor(n, 63)
    ref = W.eigenvalues(h)
    eig_d = torch.empty((3, n, n, n), dtype=torch.float32, device="cuda")
    _abi().check(_abi().lib().nbe_tensor_eigenvalues(ptr(torch.from_numpy(h).cuda()), n, ptr(eig_d), 0, None))
    for th in (0.0, 0.3 * float(np.nanstd(ref))):
        th = float(np.float32(th))
        _, types = classify_abi(eig_d, n, [th])
        with np.errstate(invalid="ignore"):
            far = (np.abs(ref - th) > W.EIG_BOUND * W.frobenius(h)).all(0)
        far &= ~np.isnan(ref[0])
        left_out = 1.0 - far.sum() / float(np.count_nonzero(~np.isnan(ref[0])))
        print("threshold %g: %.2e of the voxels are within the bound of it" % (th, left_out))
        assert left_out <= 1e-3
        assert np.array_equal(types[far], W.web_types(ref, th)[far])


# ---- the shear pass --------------------------------------------------------------------------------------------------------

def device_spectra(n, seed):
    torch = _torch()
    v = np.stack([red_field(n, seed + c, np.float32) for c in range(3)])
    spec = torch.fft.rfftn(torch.from_numpy(v).cuda(), dim=(1, 2, 3)).contiguous()
    return v, spec, spec.cpu().numpy().astype(np.complex128)


def shear(spec, n, scale, first=0, count=6, max_blocks=0):
    torch = _torch()
    out = torch.full((count, n, n, n // 2 + 1), 5.0, dtype=torch.complex64, device="cuda")
    _abi().check(_abi().lib().nbe_shear_spectrum(ptr(spec), n, L, scale, first, count, ptr(out), max_blocks, None))
    return out.cpu().numpy()


@pytest.mark.parametrize("n", [2, 3, 12, 15, 40])
def test_shear_spectrum_vs_reference(n):
    _, spec, spec64 = device_spectra(n, 700 + n)
    scale = 0.37
    got = shear(spec, n, scale)
    ref = W.shear_spectrum(spec64, n, L, scale)
    assert got.dtype == np.complex64 and got.shape == ref.shape == (6, n, n, n // 2 + 1)
    err = np.abs(got.astype(np.complex128) - ref)
    bound = 2.0 ** -22 * np.abs(ref) + 1e-30
    print("n %d: worst error / bound %.3f" % (n, (err / bound).max()))
    assert (err <= bound).all()
    d = derivative_numbers(n)[:3]
    shape = ref.shape[1:]
    for p, (i, j) in enumerate(PAIRS):
        dead = np.broadcast_to((d[i] == 0) & (d[j] == 0), shape)     # m_i = m_j = 0 and the Nyquist rows of both factors
        assert np.all(got[p][dead] == 0) and dead[0, 0, 0]
    assert same_bits(shear(spec, n, scale, max_blocks=1), got)
    pieces = np.concatenate([shear(spec, n, scale, 0, 2), shear(spec, n, scale, 2, 1), shear(spec, n, scale, 3, 3, 3)])
    assert same_bits(pieces, got)


@pytest.mark.parametrize("n", [12, 15])
def test_shear_trace_is_minus_scale_times_the_divergence(n):
    from jax_nbody_emulator_with_dj_amd import lpt
    v, _, _ = device_spectra(n, 50 + n)
    scale = -1.9
    s = _web().velocity_shear(v, L, scale=scale)
    assert s.shape == (6, n, n, n) and s.dtype == np.float32
    err = rel_l2(s[:3].astype(np.float64).sum(0), -scale * lpt.divergence(v, L).astype(np.float64))
    print("n %d: trace against -scale div v, rel L2 %.3e" % (n, err))
    assert err <= TOL
    assert rel_l2(s, W.velocity_shear(v, L, scale)) <= TOL
    assert rel_l2(_web().velocity_shear(v, L, scale, smoothing=9.0), W.velocity_shear(v, L, scale, smoothing=9.0)) <= TOL


# ---- whole calls -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def boxes():
    """n -> (delta float32, the reference's tidal tensor and eigenvalues of the smoothed field), computed once."""
    out = {}
    for n in (12, 33):
        delta = red_field(n, 80 + n, np.float32)
        sm = 1.5 * L / n
        t = W.tidal_tensor(delta, L, smoothing=sm)
        out[n] = (delta, sm, t, W.eigenvalues(t))
    return out


@pytest.mark.parametrize("n", [12, 33])
def test_tidal_tensor_and_cosmic_web_vs_reference(boxes, n):
    torch = _torch()
    web = _web()
    delta, sm, t_ref, lam_ref = boxes[n]
    t = web.tidal_tensor(delta, L, smoothing=sm)
    assert isinstance(t, np.ndarray) and t.shape == (6, n, n, n) and t.dtype == np.float32
    e1, e0 = rel_l2(t, t_ref), rel_l2(web.tidal_tensor(delta, L), W.tidal_tensor(delta, L))
    print("n %d: tidal tensor rel L2 %.3e smoothed, %.3e plain" % (n, e1, e0))
    assert e1 <= TOL and e0 <= TOL
    assert same_bits(web.tidal_tensor(delta, L, smoothing=sm, _max_batch=1, _max_blocks=2), t)
    th = [0.0, 0.2 * float(lam_ref.std())]
    out = web.cosmic_web(delta, L, sm, threshold=th, mass=delta)
    e2 = rel_l2(out["eigenvalues"], lam_ref)
    print("n %d: eigenvalues rel L2 %.3e" % (n, e2))
    assert e2 <= TOL and out["smoothing"] == sm
    eig = out["eigenvalues"]
    assert same_bits(eig, web.tensor_eigenvalues(t))
    assert np.array_equal(out["types"], W.web_types(eig, np.float32(th[0])))
    assert np.array_equal(out["counts"], W.web_counts(eig, np.array(th, np.float32)))
    assert np.abs(out["volume_fraction"].sum(1) - 1.0).max() < 1e-15
    # the types against the reference's, away from the threshold by the whole-call error
    tol = TOL * np.abs(lam_ref).max()
    far = (np.abs(lam_ref - th[0]) > tol).all(0)
    assert far.mean() > 0.99 and np.array_equal(out["types"][far], W.web_types(lam_ref, th[0])[far])
    for t_i in range(2):
        want = W.mass_fraction(W.web_types(eig, np.float32(th[t_i])), delta)
        assert (np.abs(out["mass_fraction"][t_i] - want) <= 1e-12 * want).all() and want.min() > 0
    dev = web.cosmic_web(torch.from_numpy(delta).cuda(), L, sm, threshold=th)
    assert dev["types"].is_cuda and same_bits(dev["eigenvalues"].cpu().numpy(), eig) and "mass_fraction" not in dev


def test_cosmic_web_of_a_plane_wave():
    """delta = A cos(2 pi m.x / L): sheets where delta > threshold and voids elsewhere, no filament, no knot."""
    n, m, th = 12, (1, 2, -1), 0.1
    delta = W.plane_wave(n, m).astype(np.float32)
    out = _web().cosmic_web(delta, L, None, threshold=th)
    clear = np.abs(delta.astype(np.float64) - th) > 1e-5
    assert np.array_equal(out["types"][clear], (delta > th).astype(np.uint8)[clear]) and clear.mean() > 0.9
    assert out["counts"][0, 2] == 0 and out["counts"][0, 3] == 0 and out["counts"][0, 4] == 0
    assert np.isnan(out["smoothing"])
    lam = out["eigenvalues"].astype(np.float64)
    assert np.abs(lam[0] - np.maximum(delta, 0)).max() < 1e-5 and np.abs(lam[1]).max() < 1e-5


def test_shear_web_and_nan_share():
    web = _web()
    n = 12
    v, _, _ = device_spectra(n, 21)
    delta = red_field(n, 3, np.float32)
    out = web.cosmic_web(delta, L, 30.0, threshold=0.0, kind="shear", vmesh=v, scale=2.0)
    lam_ref = W.eigenvalues(W.velocity_shear(v, L, 2.0, smoothing=30.0))
    assert rel_l2(out["eigenvalues"], lam_ref) <= TOL
    assert np.array_equal(out["types"], W.web_types(out["eigenvalues"], np.float32(0.0)))
    bad = delta.copy()
    bad[0, 0, 0] = np.nan                                  # a NaN voxel spoils every mode: no voxel has a type
    out = web.cosmic_web(bad, L, 30.0)
    assert out["counts"][0].tolist() == [0, 0, 0, 0, n ** 3] and np.all(out["types"] == 255)
    assert out["volume_fraction"].sum() == 0.0
