"""Anisotropic two-point statistics on the MI355X: power_spectrum_multipoles,
power_spectrum_wedges and lpt.divergence against the float64 restatement of tests/aniso_ref.py, the integer scheme of the
two entry points word for word, and the identities that hold bit for bit (the monopole is power_spectrum; chunking, a
second call and the kind of the input change nothing)."""

import ctypes as C
import functools

import numpy as np
import pytest

import aniso_ref as A
import mas_ref
from lpt_ref import mode_grid, red_field

pytestmark = pytest.mark.gpu

TOL = 1e-5                                  # the project's float32-FFT bound (test_gpu_density.py, test_gpu_lpt.py)
L = 500.0
CASES = [(n, los) for n in (15, 30, 64) for los in (0, 1, 2)] + [(128, 2)]   # 128: 4160 blocks' worth on a 2048-block grid
KINDS = ("auto", "correlated", "independent")


def _density():
    from jax_nbody_emulator_with_dj_amd import density
    return density


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.sqrt(((a - b) ** 2).sum() / (b ** 2).sum())


@functools.lru_cache(maxsize=None)
def fields(n, los):
    """(a, {kind: other}): float32 fields with a quadrupole about los; `correlated` is a + 0.3 c, `independent` is c, as
    test_power_spectrum_vs_reference builds them."""
    a, c = A.anisotropic_field(n, 300 + n, los), A.anisotropic_field(n, 400 + n, los)
    b = (a + 0.3 * c).astype(np.float32)
    return a, {"auto": None, "correlated": b, "independent": c}


@functools.lru_cache(maxsize=None)
def auto_power(n, los, kind):
    """mas_ref.power's P of one of the fields: the scale of a cross spectrum's error."""
    a, others = fields(n, los)
    return mas_ref.power(a if kind == "auto" else others[kind], L)[1]


def check_power(got, want, scale, cross, what):
    """|got - want| <= TOL * scale where the reference holds a value; NaN in the same places."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got - want)[ok] / scale[ok]
    print("%s: worst error %.3e of its scale (%s)" % (what, err.max() if err.size else 0.0, "cross" if cross else "auto"))
    assert (err <= TOL).all(), what


# ---- against the reference ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n, los", CASES)
def test_multipoles_vs_reference(n, los):
    a, others = fields(n, los)
    for kind in KINDS:
        got = _density().power_spectrum_multipoles(a, L, los=los, other=others[kind])
        ref = A.multipoles(a, L, los, others[kind])
        assert sorted(got) == ["k", "nmodes", "p0", "p2", "p4"]
        assert all(v.dtype == np.float64 and v.shape == (n // 2,) for v in got.values())
        assert np.array_equal(got["nmodes"], ref["nmodes"])
        np.testing.assert_allclose(got["k"], ref["k"], rtol=1e-10, atol=0)
        # a cross spectrum may cancel: its float32-FFT error is relative to sqrt(Pa Pb); so may l = 2, 4 of any spectrum
        cross = np.sqrt(auto_power(n, los, "auto") * auto_power(n, los, kind))
        if kind == "independent":
            check_power(got["p0"], ref["p0"], cross, True, "n %d los %d %s p0" % (n, los, kind))
        else:
            np.testing.assert_allclose(got["p0"], ref["p0"], rtol=TOL, atol=0)
        scale = np.abs(ref["p0"]) if kind == "auto" else cross
        for ell in (2, 4):
            check_power(got["p%d" % ell], ref["p%d" % ell], (2 * ell + 1) * scale, kind != "auto",
                        "n %d los %d %s p%d" % (n, los, kind, ell))
        assert np.abs(got["p2"]).max() > 100 * TOL * np.abs(got["p0"]).max()        # the quadrupole is not noise


@pytest.mark.parametrize("n, los", CASES)
def test_wedges_vs_reference(n, los):
    a, others = fields(n, los)
    for nmu in (1, 5, 64):
        autos = {kind: A.wedges(a if kind == "auto" else others[kind], L, los, nmu)["pk"] for kind in KINDS}
        for kind in KINDS:
            got = _density().power_spectrum_wedges(a, L, los=los, nmu=nmu, other=others[kind])
            ref = A.wedges(a, L, los, nmu, others[kind])
            assert sorted(got) == ["k", "mu", "mu_edges", "nmodes", "pk"]
            assert all(got[key].dtype == np.float64 and got[key].shape == (nmu, n // 2) for key in ("k", "mu", "pk", "nmodes"))
            assert np.array_equal(got["mu_edges"], np.arange(nmu + 1) / nmu)
            assert np.array_equal(got["nmodes"], ref["nmodes"])
            empty = ref["nmodes"] == 0
            for key in ("k", "mu", "pk"):
                assert np.array_equal(np.isnan(got[key]), empty), key
            np.testing.assert_allclose(got["k"][~empty], ref["k"][~empty], rtol=1e-10, atol=0)
            np.testing.assert_allclose(got["mu"][~empty], ref["mu"][~empty], rtol=1e-10, atol=1e-10)
            scale = np.abs(ref["pk"]) if kind == "auto" else np.sqrt(autos["auto"] * autos[kind])
            check_power(got["pk"], ref["pk"], scale, kind != "auto", "n %d los %d nmu %d %s" % (n, los, nmu, kind))
        if nmu == 64 and n >= 30:
            assert empty.any() and not empty.all()


# ---- the integer scheme itself ----------------------------------------------------------------------------------------------

def _spectrum(n, seed):
    """A seeded complex64 half spectrum whose shells differ in scale, so that their exponents differ."""
    rng = np.random.default_rng(seed)
    shape = (n, n, n // 2 + 1)
    q = np.broadcast_to(mode_grid(n)[3], shape)
    return ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * 37.0 / (1.0 + q)).astype(np.complex64)


def _entry_points(spec, other, n, los, nmu, max_bins=0):
    """(binmax, multipole sums (5, nb), binmax, wedge sums (4, nmu, nb)) of the two entry points, as NumPy."""
    import torch
    from jax_nbody_emulator_with_dj_amd import _lib
    l = _lib.lib()
    nb = n // 2 + 1
    a = torch.from_numpy(spec).cuda()
    b = None if other is None else torch.from_numpy(other).cuda()
    pb = None if b is None else C.c_void_p(b.data_ptr())
    stream = C.c_void_p(int(torch.cuda.current_stream().cuda_stream) or None)
    bm1, s1 = torch.zeros(nb, dtype=torch.int32, device="cuda"), torch.zeros(5 * nb, dtype=torch.int64, device="cuda")
    bm2, s2 = torch.zeros(nb, dtype=torch.int32, device="cuda"), torch.zeros(4 * nmu * nb, dtype=torch.int64, device="cuda")
    _lib.check(l.nbe_power_multipoles(C.c_void_p(a.data_ptr()), pb, n, los, C.c_void_p(bm1.data_ptr()),
                                      C.c_void_p(s1.data_ptr()), stream))
    _lib.check(l.nbe_power_wedges(C.c_void_p(a.data_ptr()), pb, n, los, nmu, max_bins, C.c_void_p(bm2.data_ptr()),
                                  C.c_void_p(s2.data_ptr()), stream))
    return (bm1.cpu().numpy().view(np.uint32), s1.cpu().numpy().reshape(5, nb), bm2.cpu().numpy().view(np.uint32),
            s2.cpu().numpy().reshape(4, nmu, nb))


@pytest.mark.parametrize("n", [30, 15])
def test_integer_sums_word_for_word(n):
    """Modes, k and |mu| words are equal.  Two float64 evaluations of one term p L_l differ by far less than a unit, so its
    rint moves by at most one: a power word is within (modes of its bin) units."""
    nmu = 5
    spec, other = _spectrum(n, 11 + n), _spectrum(n, 12 + n)
    for los in (0, 1, 2):
        for b in (None, other):
            ref = A.integer_sums(spec, n, los, b, nmu)
            bm1, mp, bm2, wd = _entry_points(spec, b, n, los, nmu)
            assert np.array_equal(bm1, ref["binmax"]) and np.array_equal(bm2, ref["binmax"])
            assert len(set(np.frexp(bm1[1:].view(np.float32))[1])) > 3         # the shells' exponents do differ
            assert np.array_equal(mp[:2], ref["multipoles"][:2])
            assert np.array_equal(wd[:3], ref["wedges"][:3])
            assert np.all(mp[:, 0] == 0) and np.all(wd[:, :, 0] == 0)            # shell 0 is not binned
            for word in (2, 3, 4):
                d = np.abs(mp[word] - ref["multipoles"][word])
                print("n %d los %d word %d: worst %d units" % (n, los, word, d.max()))
                assert (d <= mp[0]).all()
            d = np.abs(wd[3] - ref["wedges"][3])
            assert (d <= wd[0]).all()
            assert mp[2].any() and mp[3].any() and mp[4].any() and wd[3].any()


def test_entry_points_refuse_bad_arguments():
    import torch
    from jax_nbody_emulator_with_dj_amd import _lib
    l = _lib.lib()
    t = torch.zeros(4096, dtype=torch.int64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    q = C.c_void_p(t.data_ptr() + 8)
    for call, name in ((lambda: l.nbe_power_multipoles(None, None, 8, 0, p, p, None), "nbe_power_multipoles"),
                       (lambda: l.nbe_power_multipoles(p, None, 1, 0, p, p, None), "nbe_power_multipoles"),
                       (lambda: l.nbe_power_multipoles(p, None, 4096, 0, p, p, None), "nbe_power_multipoles"),
                       (lambda: l.nbe_power_multipoles(p, None, 8, 3, p, p, None), "nbe_power_multipoles"),
                       (lambda: l.nbe_power_wedges(p, None, 8, 0, 5, 0, None, p, None), "nbe_power_wedges"),
                       (lambda: l.nbe_power_wedges(p, None, 2049, 0, 5, 0, p, p, None), "nbe_power_wedges"),
                       (lambda: l.nbe_power_wedges(p, None, 8, -1, 5, 0, p, p, None), "nbe_power_wedges"),
                       (lambda: l.nbe_power_wedges(p, None, 8, 0, 0, 0, p, p, None), "nbe_power_wedges"),
                       (lambda: l.nbe_power_wedges(p, None, 8, 0, 65, 0, p, p, None), "nbe_power_wedges"),
                       (lambda: l.nbe_power_wedges(p, None, 8, 0, 5, 4, p, p, None), "nbe_power_wedges"),    # 5 shells, 4 bins
                       (lambda: l.nbe_power_wedges(p, None, 8, 0, 5, -1, p, p, None), "nbe_power_wedges"),
                       (lambda: l.nbe_divergence_spectrum(None, 8, 1.0, p, None), "nbe_divergence_spectrum"),
                       (lambda: l.nbe_divergence_spectrum(p, 8, 1.0, p, None), "nbe_divergence_spectrum"),
                       (lambda: l.nbe_divergence_spectrum(p, 1, 1.0, q, None), "nbe_divergence_spectrum"),
                       (lambda: l.nbe_divergence_spectrum(p, 8, 0.0, q, None), "nbe_divergence_spectrum")):
        rc = call()
        assert rc != 0
        with pytest.raises(_lib.NBEError, match=name):
            _lib.check(rc)
    torch.cuda.synchronize()
    assert not t.any()


# ---- identities that hold bit for bit -----------------------------------------------------------------------------------------

def same(x, y):
    return all(np.array_equal(x[key], y[key], equal_nan=True) and x[key].tobytes() == y[key].tobytes() for key in x) \
        and sorted(x) == sorted(y)


@pytest.mark.parametrize("kind", ["auto", "correlated"])
def test_monopole_is_power_spectrum(kind):
    """The same binmax, the same integers, the same conversion."""
    D = _density()
    for n in (30, 15):
        a, others = fields(n, 0)
        k, pk, nm = D.power_spectrum(a, L, other=others[kind])
        for los in (0, 1, 2):
            mp = D.power_spectrum_multipoles(a, L, los=los, other=others[kind])
            assert np.array_equal(mp["k"], k) and np.array_equal(mp["p0"], pk) and np.array_equal(mp["nmodes"], nm)
            wd = D.power_spectrum_wedges(a, L, los=los, nmu=1, other=others[kind])
            assert np.array_equal(wd["k"][0], k) and np.array_equal(wd["pk"][0], pk) and np.array_equal(wd["nmodes"][0], nm)
            assert np.array_equal(wd["mu_edges"], [0.0, 1.0])


def test_chunking_repetition_and_residency():
    """n = 30, nmu = 5: 80 (mu, s) bins.  32 bins per launch hold two mu bins: launches of 2, 2 and 1; 16 hold one: five
    launches; 47 hold two again.  Integer sums: every chunking gives the same bits."""
    import torch
    D = _density()
    a, others = fields(30, 1)
    for other in (None, others["correlated"]):
        whole = D.power_spectrum_wedges(a, L, los=1, nmu=5, other=other)
        assert np.isnan(whole["pk"]).any() and np.isfinite(whole["pk"]).sum() > 40
        for cap in (32, 16, 47, 80, 10 ** 6):
            assert same(D.power_spectrum_wedges(a, L, los=1, nmu=5, other=other, _max_bins=cap), whole), cap
        assert same(D.power_spectrum_wedges(a, L, los=1, nmu=5, other=other), whole)
        to = None if other is None else torch.from_numpy(other).cuda()
        assert same(D.power_spectrum_wedges(torch.from_numpy(a).cuda(), L, los=1, nmu=5, other=to), whole)
        mp = D.power_spectrum_multipoles(a, L, los=1, other=other)
        assert same(D.power_spectrum_multipoles(a, L, los=1, other=other), mp)
        assert same(D.power_spectrum_multipoles(torch.from_numpy(a).cuda(), L, los=1, other=to), mp)
    from jax_nbody_emulator_with_dj_amd._lib import NBEError
    with pytest.raises(NBEError, match="max_bins"):
        D.power_spectrum_wedges(a, L, los=1, nmu=5, _max_bins=15)            # 16 shells do not fit


# ---- edges ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3])
def test_one_shell(n):
    D = _density()
    a = np.random.default_rng(n).standard_normal((n, n, n)).astype(np.float32)
    b = np.random.default_rng(n + 10).standard_normal((n, n, n)).astype(np.float32)
    pa, pb = mas_ref.power(a, L)[1], mas_ref.power(b, L)[1]
    for los in (0, 1, 2):
        for other, scale in ((None, pa), (b, np.sqrt(pa * pb))):
            got, ref = D.power_spectrum_multipoles(a, L, los=los, other=other), A.multipoles(a, L, los, other)
            assert got["nmodes"].shape == (1,) and np.array_equal(got["nmodes"], ref["nmodes"])
            np.testing.assert_allclose(got["k"], ref["k"], rtol=1e-10, atol=0)
            for ell in (0, 2, 4):
                check_power(got["p%d" % ell], ref["p%d" % ell], (2 * ell + 1) * scale, other is not None, "n %d p%d" % (n, ell))
            for nmu in (1, 5):
                got, ref = D.power_spectrum_wedges(a, L, los=los, nmu=nmu, other=other), A.wedges(a, L, los, nmu, other)
                assert np.array_equal(got["nmodes"], ref["nmodes"])
                np.testing.assert_allclose(got["mu"], ref["mu"], rtol=1e-10, atol=1e-10)
                check_power(got["pk"], ref["pk"], np.broadcast_to(scale, ref["pk"].shape), other is not None, "n %d wedges" % n)


def test_non_finite_values():
    """One infinite mode: the entry points mark its shell (a binmax word that is not finite, power words 0) and leave every
    other word as it is without it, and the conversion turns a marked shell into NaN.  One infinite voxel reaches every
    mode of the transform, so the public calls return NaN power in every shell, with the counts and k of a finite field."""
    D = _density()
    n, nmu, los = 15, 5, 2
    spec = _spectrum(n, 3)
    bad = spec.copy()
    bad[2, 1, 2] = np.complex64(complex(np.inf, 1.0))                       # |m|^2 = 9: shell 3
    bm, mp, bm_w, wd = _entry_points(spec, None, n, los, nmu)
    bm_b, mp_b, bm_wb, wd_b = _entry_points(bad, None, n, los, nmu)
    assert np.array_equal(bm_b, bm_wb) and not np.isfinite(bm_b.view(np.float32)[3])
    keep = np.arange(n // 2 + 1) != 3
    assert np.array_equal(bm_b[keep], bm[keep])
    assert np.array_equal(mp_b[:, keep], mp[:, keep]) and np.array_equal(wd_b[:, :, keep], wd[:, :, keep])
    assert np.array_equal(mp_b[:2, 3], mp[:2, 3]) and not mp_b[2:, 3].any()
    assert np.array_equal(wd_b[:3, :, 3], wd[:3, :, 3]) and not wd_b[3, :, 3].any()
    k, pk, cnt = D._shell_means(bm_b[1:].view(np.int32), mp_b[0, 1:], mp_b[1, 1:], mp_b[2, 1:], np.arange(1.0, 8.0), 36, L, n)
    assert np.isnan(pk[2]) and np.isfinite(np.delete(pk, 2)).all() and np.isfinite(k).all()

    a, _ = fields(n, los)
    x = a.copy()
    x[1, 2, 3] = np.inf
    good, got = D.power_spectrum_multipoles(a, L, los=los), D.power_spectrum_multipoles(x, L, los=los)
    assert all(np.isnan(got[key]).all() for key in ("p0", "p2", "p4"))
    assert np.array_equal(got["nmodes"], good["nmodes"]) and np.array_equal(got["k"], good["k"])
    good, got = D.power_spectrum_wedges(a, L, los=los, nmu=nmu), D.power_spectrum_wedges(x, L, los=los, nmu=nmu)
    assert np.isnan(got["pk"]).all() and np.array_equal(got["nmodes"], good["nmodes"])
    assert np.array_equal(got["k"], good["k"], equal_nan=True) and np.array_equal(got["mu"], good["mu"], equal_nan=True)


@pytest.mark.parametrize("los", [0, 1, 2])
def test_plane_wave_on_the_card(los):
    D = _density()
    n, box, amp, m, nmu = 16, 100.0, 0.3, (1, 2, 2), 5
    x = A.plane_wave(n, m, amp).astype(np.float32)
    mp = D.power_spectrum_multipoles(x, box, los=los)
    _, l2, l4 = A.legendre(np.float64(m[los] ** 2 / 9.0))
    np.testing.assert_allclose(mp["p0"][2], amp * amp * box ** 3 / 2.0 / mp["nmodes"][2], rtol=TOL)
    np.testing.assert_allclose(mp["p2"][2] / mp["p0"][2], 5.0 * l2, rtol=TOL)
    np.testing.assert_allclose(mp["p4"][2] / mp["p0"][2], 9.0 * l4, rtol=TOL)
    assert np.abs(np.delete(mp["p0"], 2)).max() < 1e-9 * mp["p0"][2]
    wd = D.power_spectrum_wedges(x, box, los=los, nmu=nmu)
    j = int(A.mu_bin(m[los], 9, nmu))
    power = wd["nmodes"] * np.nan_to_num(wd["pk"])
    np.testing.assert_allclose(power[j, 2], mp["p0"][2] * mp["nmodes"][2], rtol=TOL)
    power[j, 2] = 0.0
    assert np.abs(power).max() < 1e-9 * mp["p0"][2] * mp["nmodes"][2]
    np.testing.assert_allclose(wd["mu"][j, 2], A.wedges(x, box, los, nmu)["mu"][j, 2], rtol=1e-10)


# ---- divergence ---------------------------------------------------------------------------------------------------------------

def _vector_field(n, seed):
    return np.stack([red_field(n, seed + c, np.float32) for c in range(3)])


@pytest.mark.parametrize("n", [12, 15, 40])
def test_divergence_vs_reference(n):
    """Even, odd, and (40) more than one pass of the grid with a ragged tail: 1600 rows of 21 modes."""
    from jax_nbody_emulator_with_dj_amd import lpt
    v = _vector_field(n, 500 + n)
    theta = lpt.divergence(v, boxsize=250.0)
    assert isinstance(theta, np.ndarray) and theta.dtype == np.float32 and theta.shape == (n, n, n)
    err = rel_l2(theta, A.divergence(v, 250.0))
    print("n %d: rel L2 %.3e" % (n, err))
    assert err <= TOL


@pytest.mark.parametrize("n", [12, 15])
def test_divergence_undoes_zeldovich(n):
    """div psi = -delta for a delta with zero mean and nothing on the rows |m_c| = n/2, which both calls leave out."""
    from jax_nbody_emulator_with_dj_amd import lpt
    m0, m1, m2, q = mode_grid(n)
    spec = np.fft.rfftn(red_field(n, 600 + n))
    keep = (2 * np.abs(m0) < n) & (2 * np.abs(m1) < n) & (2 * m2 < n) & (q > 0)
    x = np.fft.irfftn(np.where(keep, spec, 0.0), s=(n, n, n), axes=(0, 1, 2)).astype(np.float32)
    theta = lpt.divergence(lpt.zeldovich_displacement(x, boxsize=250.0, scale=1.0), boxsize=250.0)
    err = rel_l2(theta, -x)
    print("n %d: rel L2 %.3e" % (n, err))
    assert err <= TOL


def test_divergence_residency_repetition_and_spectra():
    import torch
    from jax_nbody_emulator_with_dj_amd import lpt
    D = _density()
    n = 24
    v = _vector_field(n, 77)
    one = lpt.divergence(v, boxsize=L)
    assert one.tobytes() == lpt.divergence(v, boxsize=L).tobytes()
    vt = torch.from_numpy(v).cuda()
    tt = lpt.divergence(vt, boxsize=L)
    assert isinstance(tt, torch.Tensor) and tt.device == vt.device and tt.dtype == torch.float32 and tt.shape == (n, n, n)
    assert tt.cpu().numpy().tobytes() == one.tobytes()
    assert np.array_equal(lpt.divergence(v, boxsize=(L, L, L)), one)
    # P_theta-theta and P_delta-theta, and the multipoles of the pair
    delta = red_field(n, 78, np.float32)
    ref = A.divergence(v, L)
    np.testing.assert_allclose(D.power_spectrum(one, L)[1], mas_ref.power(ref, L)[1], rtol=TOL)
    got, want = D.power_spectrum(delta, L, other=one)[1], mas_ref.power(delta, L, ref)[1]
    assert (np.abs(got - want) <= TOL * np.sqrt(mas_ref.power(delta, L)[1] * mas_ref.power(ref, L)[1])).all()
    mp = D.power_spectrum_multipoles(delta, L, los=0, other=one)
    assert np.array_equal(mp["p0"], got) and np.isfinite(mp["p2"]).all() and np.isfinite(mp["p4"]).all()
