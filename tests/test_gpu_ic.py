"""The linear field drawn from a seed on the MI355X (lpt.gaussian_spectrum, gaussian_field, white_noise, colour_noise,
linear_ics) against the float64 restatement tests/ic_ref.py.

Spectra are held to 2^-22 |ref| + 1e-30 per mode, the bound test_inject_spectrum_vs_reference holds the same arithmetic to
(float64 draws rounded once, four half-ulps for the separate roundings of the two words and for libm differences); fields
that pass through a float32 transform to a relative L2 error of 1e-5, the module's bound for that path."""

import numpy as np
import pytest

import ic_ref as I
import lpt_ref as R
from lpt_ref import power_law_table, red_field

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = 1000.0
SEED = 12345
K, PK = power_law_table(32, L)            # one table for every size (nesting compares sizes): 0.5 to 11.2 k_F, so that the
#                                           small meshes interpolate and the larger ones also use the fitted tail
FLAGS = {"plain": 0, "fixed": I.FIXED, "inverted": I.INVERT, "fixed+inverted": I.FIXED | I.INVERT, "white": I.WHITE}


def _torch():
    import torch
    return torch


def _lpt():
    from jax_nbody_emulator_with_dj_amd import lpt
    return lpt


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def device_spectrum(n, flags=0, seed=SEED, scale=0.8, **kw):
    """The device's half spectrum as a NumPy array, through the public function (the white flag through the private one:
    the public white_noise returns the field)."""
    lpt = _lpt()
    if flags & I.WHITE:
        dev = _torch().device("cuda", _torch().cuda.current_device())
        return lpt._draw_spectrum(n, 1.0, None, seed, 1.0, flags, dev).cpu().numpy()
    return lpt.gaussian_spectrum(n, L, K, PK, seed=seed, scale=scale, fixed_amplitude=bool(flags & I.FIXED),
                                 invert_phase=bool(flags & I.INVERT), **kw).cpu().numpy()


def reference_spectrum(n, flags=0, seed=SEED, scale=0.8):
    return I.gaussian_spectrum(n, L, K, PK, seed, scale, flags)


def assert_within_bound(got, ref, what):
    assert got.dtype == np.complex64 and got.shape == ref.shape
    err = np.abs(got.astype(np.complex128) - ref)
    bound = 2.0 ** -22 * np.abs(ref) + 1e-30
    print("%s: worst error / bound %.3f" % (what, (err / bound).max()))
    assert (err <= bound).all()


# ---- the spectrum ---------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def plain():
    """The plain draw on the device, once per size."""
    return {n: device_spectrum(n) for n in (3, 4, 9, 16, 32, 130)}


@pytest.mark.parametrize("n", [3, 4, 9, 16, 130])
def test_spectrum_vs_restatement(plain, n):
    """3: no Nyquist plane, the smallest size with a complex mode; 4: the smallest even size; 130: a half row of 66 modes,
    more than the 64 lanes, so the lane loop strides."""
    ref = reference_spectrum(n)
    assert_within_bound(plain[n], ref, "n %d" % n)
    assert (np.abs(ref).ravel()[1:] > 0).all()


@pytest.mark.parametrize("n", [9, 16])
@pytest.mark.parametrize("name", ["fixed", "inverted", "fixed+inverted", "white"])
def test_flag_combinations_vs_restatement(n, name):
    assert_within_bound(device_spectrum(n, FLAGS[name]), reference_spectrum(n, FLAGS[name]), "n %d %s" % (n, name))


@pytest.mark.parametrize("n", [3, 4, 9, 16, 130])
def test_paired_planes_are_hermitian_bit_for_bit(plain, n):
    S = plain[n]
    mirror = (-np.arange(n)) % n
    own = I.pairing(n)[1]
    for i2 in sorted({0, n // 2} if n % 2 == 0 else {0}):
        plane = S[:, :, i2]
        assert np.array_equal(bits(plane[mirror][:, mirror].real), bits(plane.real))
        moving = ~own[:, :, i2]
        assert np.array_equal(bits(plane[mirror][:, mirror].imag)[moving], bits(-plane.imag)[moving])
    assert np.all(bits(S.imag)[own] == 0)                                    # +0, not -0
    assert np.all(bits(S[0, 0, 0:1].real) == 0) and np.all(bits(S[0, 0, 0:1].imag) == 0)


@pytest.mark.parametrize("max_blocks", [1, 3])
def test_launch_geometry_does_not_change_the_bits(plain, max_blocks):
    """n = 16 has 256 rows, 64 workgroups of four: capped at 1 and at 3 workgroups the row loop wraps (3 does not divide
    64, so the last round is ragged)."""
    got = device_spectrum(16, _max_blocks=max_blocks)
    assert np.array_equal(bits(got), bits(plain[16]))


def eight(x):
    """8 x, word by word (a power of two: exact)."""
    return (np.float32(8) * np.ascontiguousarray(x).view(np.float32)).view(np.complex64)


def test_nesting_on_the_device(plain):
    """One seed is one universe: a mode with every |m_c| < 8 has at n = 32 exactly 8 times its words at n = 16 (sigma
    carries n^3 and only products follow).  i2 > 0: every such mode.  i2 = 0: the drawing rows, and the conjugate rows
    after conjugation."""
    a, b = plain[16], plain[32]
    m16, m32 = R.wave_numbers(16), R.wave_numbers(32)
    i16, i32 = np.flatnonzero(np.abs(m16) < 8), np.flatnonzero(np.abs(m32) < 8)
    assert np.array_equal(m16[i16], m32[i32])
    sub16, sub32 = a[np.ix_(i16, i16, np.arange(8))], b[np.ix_(i32, i32, np.arange(8))]
    assert np.array_equal(bits(sub32[:, :, 1:]), bits(eight(sub16[:, :, 1:])))
    second16 = I.pairing(16)[0][np.ix_(i16, i16, [0])][:, :, 0]
    second32 = I.pairing(32)[0][np.ix_(i32, i32, [0])][:, :, 0]
    assert np.array_equal(second16, second32)
    p16, p32 = sub16[:, :, 0], sub32[:, :, 0]
    assert np.array_equal(bits(p32[~second32]), bits(eight(p16[~second16])))
    assert np.array_equal(bits(np.conj(p32[second32])), bits(eight(np.conj(p16[second16]))))
    assert (np.abs(sub16) > 0).sum() == sub16.size - 1                       # every mode but F(0) is compared on a value


@pytest.mark.parametrize("n", [9, 16])
def test_fixed_amplitude(n):
    sigma = np.broadcast_to(I.sigma(n, L, K, PK, 0.8), (n, n, n // 2 + 1))
    got = np.abs(device_spectrum(n, I.FIXED).astype(np.complex128))
    live = R.mode_grid(n)[3] > 0
    worst = float(np.abs(got[live] / sigma[live] - 1.0).max())
    print("n %d: worst | |F| / sigma - 1 | = %.3e (2^-22 = %.3e)" % (n, worst, 2.0 ** -22))
    assert worst <= 2.0 ** -22 and got[0, 0, 0] == 0


@pytest.mark.parametrize("n", [9, 16])
def test_paired_field_is_the_negation(plain, n):
    """invert_phase flips the sign bit of every non-zero word; the words that are +0 (F(0), the imaginary word of a self
    mode) stay +0."""
    got, ref = device_spectrum(n, I.INVERT), plain[n]
    zero = bits(ref.view(np.float32)) == 0
    assert np.array_equal(bits(got.view(np.float32))[~zero], bits(-ref.view(np.float32))[~zero])
    assert np.all(bits(got.view(np.float32))[zero] == 0)
    assert zero.sum() == 1 + I.pairing(n)[1].sum()


def test_seeds(plain):
    other = device_spectrum(16, seed=SEED + (1 << 32))
    assert not np.any(other.ravel()[1:] == plain[16].ravel()[1:])
    assert not np.any(device_spectrum(16, seed=SEED + 1).ravel()[1:] == plain[16].ravel()[1:])
    assert np.array_equal(bits(device_spectrum(16)), bits(plain[16]))
    assert_within_bound(device_spectrum(9, seed=2 ** 64 - 1), reference_spectrum(9, seed=2 ** 64 - 1), "seed 2^64 - 1")


# ---- fields ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [16, 15])
def test_gaussian_field(n):
    torch, lpt = _torch(), _lpt()
    k, pk = power_law_table(n, L)
    dev = torch.device("cuda", torch.cuda.current_device())
    x = lpt.gaussian_field(n, L, k, pk, seed=SEED, scale=0.8, device=dev)
    assert isinstance(x, torch.Tensor) and x.device == dev and x.dtype == torch.float32 and x.shape == (n, n, n)
    assert x.is_contiguous()
    ref = I.gaussian_field(n, L, k, pk, SEED, 0.8)
    err = rel_l2(x.cpu().numpy(), ref)
    mean = abs(float(x.double().mean())) / float(np.abs(ref).max())
    print("n %d: rel L2 %.3e, |mean| / max %.3e" % (n, err, mean))
    assert err <= TOL and mean <= 1e-6
    y = lpt.gaussian_field(n, L, k, pk, seed=SEED, scale=0.8, out="numpy")
    assert isinstance(y, np.ndarray) and y.dtype == np.float32 and np.array_equal(bits(y), bits(x.cpu().numpy()))


@pytest.mark.parametrize("n", [12, 15])
def test_colour_noise_vs_restatement(n):
    torch, lpt = _torch(), _lpt()
    k, pk = power_law_table(n, L)
    w = np.random.default_rng(n).standard_normal((n, n, n)).astype(np.float32)
    out = lpt.colour_noise(w, L, k, pk, scale=0.8)
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.shape == (n, n, n)
    err = rel_l2(out, I.colour_noise(w, L, k, pk, 0.8))
    print("n %d: rel L2 %.3e" % (n, err))
    assert err <= TOL
    wt = torch.from_numpy(w).cuda()
    t = lpt.colour_noise(wt, L, k, pk, scale=0.8)
    assert isinstance(t, torch.Tensor) and t.device == wt.device and np.array_equal(bits(t.cpu().numpy()), bits(out))
    assert np.array_equal(wt.cpu().numpy(), w)                              # the input is not written


def test_coloured_white_noise_is_the_gaussian_field():
    lpt = _lpt()
    n = 16
    k, pk = power_law_table(n, L)
    w = lpt.white_noise(n, seed=SEED)
    assert w.dtype == _torch().float32 and w.shape == (n, n, n)
    assert rel_l2(w.cpu().numpy(), I.gaussian_field(n, seed=SEED, flags=I.WHITE)) <= TOL
    err = rel_l2(lpt.colour_noise(w, L, k, pk, scale=0.8).cpu().numpy(),
                 lpt.gaussian_field(n, L, k, pk, seed=SEED, scale=0.8).cpu().numpy())
    print("rel L2 %.3e" % err)
    assert err <= TOL
    assert isinstance(lpt.white_noise(n, seed=SEED, out="numpy"), np.ndarray)


# ---- initial conditions ---------------------------------------------------------------------------------------------------------

def test_linear_ics_is_the_spectrum_route_of_zeldovich_displacement():
    torch, lpt = _torch(), _lpt()
    n = 16
    k, pk = power_law_table(n, L)
    delta, psi = lpt.linear_ics(n, L, k, pk, SEED, scale=0.8)
    assert psi.dtype == torch.float32 and psi.shape == (3, n, n, n) and psi.is_contiguous() and psi.is_cuda
    spec = lpt.gaussian_spectrum(n, L, k, pk, seed=SEED, scale=0.8)
    want = lpt._inverse_components(lpt._psi_spectrum(spec, n, L, 1.0), n, None)
    assert np.array_equal(bits(psi.cpu().numpy()), bits(want.cpu().numpy()))
    assert np.array_equal(bits(delta.cpu().numpy()), bits(lpt._real_field(spec, n).cpu().numpy()))
    one, psi1 = lpt.linear_ics(n, L, k, pk, SEED, scale=0.8, return_delta=False, _max_batch=1)
    assert one is None and np.array_equal(bits(psi1.cpu().numpy()), bits(psi.cpu().numpy()))
    ref = np.fft.irfftn(R.zeldovich_spectrum(I.gaussian_spectrum(n, L, k, pk, SEED, 0.8), n, L), s=(n,) * 3, axes=(1, 2, 3))
    assert rel_l2(psi.cpu().numpy(), ref) <= TOL
    _, paired = lpt.linear_ics(n, L, k, pk, SEED, scale=0.8, invert_phase=True, return_delta=False)
    assert np.array_equal(paired.cpu().numpy(), -psi.cpu().numpy())


def test_linear_ics_divergence_is_minus_delta():
    """Odd n = 15 has no Nyquist rows, so div psi = -delta holds for every mode."""
    lpt = _lpt()
    n = 15
    k, pk = power_law_table(n, L)
    delta, psi = lpt.linear_ics(n, L, k, pk, SEED, scale=0.8)
    err = rel_l2(lpt.divergence(psi, boxsize=L).cpu().numpy(), -delta.cpu().numpy())
    print("rel L2 %.3e" % err)
    assert err <= TOL
    assert rel_l2(delta.cpu().numpy(), I.gaussian_field(n, L, k, pk, SEED, 0.8)) <= TOL


def test_linear_ics_feeds_process_box():
    lpt = _lpt()
    import jax_nbody_emulator_with_dj_amd as J
    from oracle import params as P
    n = 32
    cfg = J.SubboxConfig(size=(n, n, n), ndiv=(1, 1, 1), output_dtype=np.float32)
    emu = J.create_emulator(load_params=False, processor_config=cfg, mid_chan=8)
    emu.processor.params = P.synthetic_params(seed=71, mid_chan=8)
    k, pk = power_law_table(n, L)
    _, psi = lpt.linear_ics(n, L, k, pk, SEED, scale=0.05, return_delta=False)
    d_t, v_t = emu.process_box(psi, 0.5, 0.3, show_progress=False)
    d_n, v_n = emu.process_box(psi.cpu().numpy(), 0.5, 0.3, show_progress=False)
    assert np.array_equal(d_t.cpu().numpy(), np.asarray(d_n)) and np.array_equal(v_t.cpu().numpy(), np.asarray(v_n))
    assert np.isfinite(np.asarray(d_n)).all() and np.asarray(d_n).shape == (3, n, n, n)


# ---- end to end -------------------------------------------------------------------------------------------------------------------

def shell_ratio_cap(nmodes):
    """power_spectrum returns per shell the mean of |delta_k|^2 L^3 / n^6 over the modes of the full complex grid and
    their number nmodes.  Of those, 2 N_p are mirror pairs that share one draw, |F|^2 / sigma^2 exponential with variance 1,
    and N_s are self modes, chi^2_1 with variance 2: the variance of the sum is 4 N_p + 2 N_s = 2 nmodes, so the mean has
    the standard deviation sqrt(2 / nmodes) and the factor on 4 sqrt(2 / nmodes) is 1."""
    return 4.0 * np.sqrt(2.0 / nmodes)


def end_to_end_table():
    k = np.geomspace(0.5 * 2.0 * np.pi / L, 2.0 * np.pi * 32 / L, 64)         # covers every shell: np.interp throughout
    return k, 2.0e4 * (k / 0.1) ** -1.7


def test_power_spectrum_of_the_drawn_field():
    """n = 32, seed 12345: every shell with at least 10 modes has P_measured / P_table(mean k of the shell) within
    4 sqrt(2 / nmodes) of 1 (shell_ratio_cap).  The restatement passes with this seed (worst shell 0.47 of the cap)."""
    lpt = _lpt()
    from jax_nbody_emulator_with_dj_amd.density import power_spectrum
    n = 32
    k, pk = end_to_end_table()
    kk, pp, nmodes = power_spectrum(lpt.gaussian_field(n, L, k, pk, seed=SEED), boxsize=L)
    slope, intercept = R.tail_fit(k, pk)
    ratio = pp / R.table_power(kk, k, pk, slope, intercept)
    checked = nmodes >= 10
    worst = np.abs(ratio - 1.0)[checked] / shell_ratio_cap(nmodes[checked])
    print("shells checked %d of %d, worst |ratio - 1| / cap %.3f" % (checked.sum(), nmodes.size, worst.max()))
    assert checked.sum() >= 15 and (worst <= 1.0).all()
