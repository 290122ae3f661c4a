"""Second-order LPT on the MI355X (lpt.lpt2_source, lpt2_displacement, linear_ics(order=2) and the three entry points of
csrc/nbe_lpt.hip behind them) against the float64 restatement tests/lpt2_ref.py.

The kernels are held per word: the two spectral passes to 2^-22 of the float64 term(s) (the bound of
test_inject_spectrum_vs_reference: a float64 factor, one rounding per word), the real-space pass to the bits of the NumPy
float64 expression.  Whole calls are held to test_gpu_lpt.py's relative L2 of 1e-5; a CPU emulation of the float32 path
gives 2.1e-7 to 4.2e-7 for psi2 at these sizes."""

import ctypes as C

import numpy as np
import pytest

import lpt2_ref as R2
from lpt_ref import red_field

pytestmark = pytest.mark.gpu

TOL = 1e-5
L = 1000.0
K = np.geomspace(0.003, 0.3, 24)
PK = 2.0e4 * (K / 0.1) ** -1.7


def _torch():
    import torch
    return torch


def _lpt():
    from jax_nbody_emulator_with_dj_amd import lpt
    return lpt


def _abi():
    from jax_nbody_emulator_with_dj_amd import _lib
    return _lib


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def ptr(t):
    return C.c_void_p(t.data_ptr())


def device_spectrum(n, seed):
    """The device's own half spectrum of a red field, as a CUDA tensor and as complex128."""
    spec = _lpt()._half_spectrum(_torch().from_numpy(red_field(n, seed, np.float32)).cuda())
    return spec, spec.cpu().numpy().astype(np.complex128)


def hessian(spec, n, first=0, count=6, max_blocks=0):
    out = _lpt()._empty_spectrum(n, spec.device, (count,))
    _abi().check(_abi().lib().nbe_lpt2_hessian_spectrum(ptr(spec), n, first, count, ptr(out), max_blocks, None))
    return out.cpu().numpy()


# ---- the Hessian pass ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 12, 15, 40, 130])
def test_hessian_spectrum_vs_reference(n):
    """Even and odd, one row of workgroups and many (40: 1600 rows of 21), and rows of 66 modes (130), which take the
    lane loop twice with a ragged tail."""
    spec, spec64 = device_spectrum(n, 900 + n)
    got = hessian(spec, n)
    ref = R2.hessian_spectrum(spec64, n)
    assert got.dtype == np.complex64 and got.shape == ref.shape == (6, n, n, n // 2 + 1)
    err = np.abs(got.astype(np.complex128) - ref)
    bound = 2.0 ** -22 * np.abs(ref) + 1e-30
    print("n %d: worst error / bound %.3f" % (n, (err / bound).max()))
    assert (err <= bound).all()
    d0, d1, d2, q = R2.derivative_numbers(n)
    d = (d0, d1, d2)
    for p, (i, j) in enumerate(R2.PAIRS):
        dead = np.broadcast_to(d[i] * d[j] == 0, q.shape)           # m = 0 and the Nyquist rows of either factor
        assert np.all(got[p][dead] == 0) and dead[0, 0, 0]
        if n > 3:
            assert np.all(got[p][~dead] != 0)


def test_hessian_pieces_and_capped_grid_give_the_same_bits():
    n = 12
    spec, _ = device_spectrum(n, 77)
    whole = hessian(spec, n)
    assert same_bits(hessian(spec, n, max_blocks=1).view(np.float32), whole.view(np.float32))
    pieces = np.concatenate([hessian(spec, n, 0, 2), hessian(spec, n, 2, 1), hessian(spec, n, 3, 3, max_blocks=3)])
    assert same_bits(pieces.view(np.float32), whole.view(np.float32))


# ---- the real-space pass ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [2, 3, 15, 16, 40])
def test_source_kernel_bit_for_bit(n):
    """Odd n takes the 4-byte path (component c starts at byte 4 c n^3), even n the 16-byte one; max_blocks 1 and 3 make
    the grid-stride loop wrap.  Six independent normal fields, and six equal ones (S = +0 everywhere)."""
    torch, lib = _torch(), _abi()
    rng = np.random.default_rng(1200 + n)
    h = rng.standard_normal((6, n, n, n)).astype(np.float32)
    same = np.broadcast_to(h[0], h.shape).copy()
    for fields in (h, same):
        ref = R2.source(fields).astype(np.float32)
        assert np.all((ref == 0) | (np.abs(ref) >= np.finfo(np.float32).tiny))        # zero or normal: no flushing question
        if fields is same:
            assert same_bits(ref, np.zeros_like(ref))
        ht = torch.from_numpy(fields).cuda()
        for max_blocks in (0, 1, 3):
            out = torch.full((n, n, n), np.nan, dtype=torch.float32, device="cuda")
            lib.check(lib.lib().nbe_lpt2_source(ptr(ht), n, ptr(out), max_blocks, None))
            assert same_bits(out.cpu().numpy(), ref)


# ---- the displacement pass ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [12, 15, 40])
def test_displacement_spectrum_vs_reference(n):
    lpt, lib = _lpt(), _abi()
    box, a, b = 250.0, 0.8, 0.3
    dk, dk64 = device_spectrum(n, 1300 + n)
    sk, sk64 = device_spectrum(n, 1400 + n)
    out = lpt._empty_spectrum(n, dk.device, (3,))
    lib.check(lib.lib().nbe_lpt2_spectrum(ptr(dk), ptr(sk), n, box, a, b, ptr(out), 0, None))
    got = out.cpu().numpy().astype(np.complex128)
    t1, t2 = R2.zeldovich_spectrum(dk64, n, box, a), R2.zeldovich_spectrum(sk64, n, box, b)      # i f a delta, i f b S
    assert np.abs(R2.lpt2_spectrum(dk64, sk64, n, box, a, b) - (t1 + t2)).max() <= 1e-12 * np.abs(t1).max()
    worst = 0.0
    for part in (np.real, np.imag):
        err = np.abs(part(got) - part(t1 + t2))
        bound = 2.0 ** -22 * (np.abs(part(t1)) + np.abs(part(t2))) + 1e-30
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all()
    print("n %d: worst error / bound %.3f" % (n, worst))
    capped = lpt._empty_spectrum(n, dk.device, (3,))
    lib.check(lib.lib().nbe_lpt2_spectrum(ptr(dk), ptr(sk), n, box, a, b, ptr(capped), 1, None))
    assert same_bits(capped.cpu().numpy().view(np.float32), out.cpu().numpy().view(np.float32))


# ---- whole calls --------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module", params=[(12, False), (12, True), (15, False), (40, False), (40, True)],
                ids=lambda p: "%d%s" % (p[0], "-dealias" if p[1] else ""))
def whole(request):
    """One field per case, its restatement once, and the device's three results."""
    n, dealias = request.param
    lpt = _lpt()
    box, scale, g = 250.0, 0.8, 0.41
    x = red_field(n, 1500 + n, np.float32)
    ref1, ref2 = R2.lpt2_orders(x, box, scale, g, dealias)
    psi = lpt.lpt2_displacement(x, boxsize=box, scale=scale, growth2=g, dealias=dealias)
    psi1, psi2 = lpt.lpt2_displacement(x, boxsize=box, scale=scale, growth2=g, dealias=dealias, return_orders=True)
    return dict(n=n, dealias=dealias, x=x, box=box, scale=scale, g=g, ref1=ref1, ref2=ref2, psi=psi, psi1=psi1, psi2=psi2)


def test_whole_calls_vs_reference(whole):
    W = whole
    n = W["n"]
    for got in (W["psi"], W["psi1"], W["psi2"]):
        assert isinstance(got, np.ndarray) and got.dtype == np.float32 and got.shape == (3, n, n, n)
    e, e1, e2 = rel_l2(W["psi"], W["ref1"] + W["ref2"]), rel_l2(W["psi1"], W["ref1"]), rel_l2(W["psi2"], W["ref2"])
    print("n %d dealias %s: rel L2 psi %.3e, psi1 %.3e, psi2 %.3e" % (n, W["dealias"], e, e1, e2))
    assert e <= TOL and e1 <= TOL and e2 <= TOL
    assert same_bits(W["psi1"], _lpt().zeldovich_displacement(W["x"], boxsize=W["box"], scale=W["scale"]))


def test_source_field_vs_reference(whole):
    W = whole
    s = _lpt().lpt2_source(W["x"], dealias=W["dealias"])
    assert s.dtype == np.float32 and s.shape == (W["n"],) * 3
    err = rel_l2(s, R2.lpt2_source(W["x"], W["dealias"]))
    print("n %d dealias %s: rel L2 %.3e, mean / rms %.3e" % (W["n"], W["dealias"], err, abs(s.mean()) / s.std()))
    assert err <= TOL


def test_crossed_waves_on_the_card():
    n, j1, j2, A, B, phi, box, scale, g = 16, 2, 3, 0.3, -0.2, 0.7, 100.0, 0.8, 0.43
    delta, cx, sx, cy, sy = R2.crossed_waves(n, j1, j2, A, B, phi)
    c = g * scale * scale * A * B * box / (2.0 * np.pi * (j1 * j1 + j2 * j2))
    want = np.stack([-c * j1 * sx * cy, -c * j2 * cx * sy, np.zeros((n, n, n))])
    for dealias in (False, True):
        _, psi2 = _lpt().lpt2_displacement(delta.astype(np.float32), boxsize=box, scale=scale, growth2=g, dealias=dealias,
                                           return_orders=True)
        err = rel_l2(psi2, want)
        print("dealias %s: rel L2 %.3e" % (dealias, err))
        assert err <= TOL


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_plane_wave_on_the_card(axis):
    psi1, psi2 = _lpt().lpt2_displacement(R2.plane_wave(16, 2, axis).astype(np.float32), boxsize=100.0, return_orders=True)
    rms1 = float(np.sqrt(np.mean(psi1[axis].astype(np.float64) ** 2)))
    print("axis %d: max |psi2| / rms psi1 %.3e" % (axis, np.abs(psi2).max() / rms1))
    assert rms1 > 0 and np.abs(psi2).max() <= TOL * rms1


def test_exact_zeros():
    lpt = _lpt()
    two = np.random.default_rng(2).standard_normal((2, 2, 2)).astype(np.float32)
    flat = np.full((8, 8, 8), 0.75, np.float32)
    for x in (two, flat):
        for dealias in (False, True):
            assert np.all(lpt.lpt2_source(x, dealias=dealias) == 0)
            assert np.all(lpt.lpt2_displacement(x, boxsize=L, dealias=dealias) == 0)


def test_orders_scale_exactly():
    lpt = _lpt()
    x = red_field(24, 7, np.float32)
    one1, one2 = lpt.lpt2_displacement(x, boxsize=L, return_orders=True)
    two1, two2 = lpt.lpt2_displacement(x, boxsize=L, scale=2.0, return_orders=True)
    assert np.array_equal(two1, 2.0 * one1) and np.array_equal(two2, 4.0 * one2) and np.abs(one2).max() > 0
    assert np.all(lpt.lpt2_displacement(x, boxsize=L, growth2=0.0, return_orders=True)[1] == 0)


def test_residency_batches_and_reproducibility():
    torch, lpt = _torch(), _lpt()
    x = red_field(24, 8, np.float32)
    xt = torch.from_numpy(x).cuda()
    for dealias in (False, True):
        one = lpt.lpt2_displacement(x, boxsize=L, scale=0.9, dealias=dealias)
        t = lpt.lpt2_displacement(xt, boxsize=L, scale=0.9, dealias=dealias)
        assert isinstance(t, torch.Tensor) and t.device == xt.device and t.dtype == torch.float32 and t.is_contiguous()
        assert same_bits(t.cpu().numpy(), one)
        assert same_bits(lpt.lpt2_displacement(xt, boxsize=L, scale=0.9, dealias=dealias).cpu().numpy(), one)
        assert same_bits(lpt.lpt2_displacement(xt, boxsize=L, scale=0.9, dealias=dealias, _max_batch=1).cpu().numpy(), one)
        s = lpt.lpt2_source(x, dealias=dealias)
        st = lpt.lpt2_source(xt, dealias=dealias, _max_batch=1)
        assert isinstance(st, torch.Tensor) and same_bits(st.cpu().numpy(), s)
        o1, o2 = lpt.lpt2_displacement(xt, boxsize=L, scale=0.9, dealias=dealias, return_orders=True)
        p1, p2 = lpt.lpt2_displacement(x, boxsize=L, scale=0.9, dealias=dealias, return_orders=True, _max_batch=1)
        assert same_bits(o1.cpu().numpy(), p1) and same_bits(o2.cpu().numpy(), p2)


@pytest.mark.parametrize("dealias", [False, True])
def test_linear_ics_second_order(dealias):
    lpt = _lpt()
    n, g = 24, 0.42
    delta1, psi_first = lpt.linear_ics(n, 500.0, K, PK, 11, scale=0.05)
    delta, psi1, psi = lpt.linear_ics(n, 500.0, K, PK, 11, scale=0.05, order=2, growth2=g, dealias=dealias)
    assert same_bits(delta.cpu().numpy(), delta1.cpu().numpy()) and same_bits(psi1.cpu().numpy(), psi_first.cpu().numpy())
    assert psi.shape == (3, n, n, n) and psi.is_cuda and psi.dtype == _torch().float32
    err = rel_l2(psi.cpu().numpy(), lpt.lpt2_displacement(delta, boxsize=500.0, growth2=g, dealias=dealias).cpu().numpy())
    print("dealias %s: rel L2 against lpt2_displacement of its own delta %.3e" % (dealias, err))
    assert err <= TOL
    assert not np.array_equal(psi.cpu().numpy(), psi1.cpu().numpy())
    none, p1, p = lpt.linear_ics(n, 500.0, K, PK, 11, scale=0.05, order=2, growth2=g, dealias=dealias, return_delta=False,
                                 _max_batch=1)
    assert none is None and same_bits(p1.cpu().numpy(), psi1.cpu().numpy()) and same_bits(p.cpu().numpy(), psi.cpu().numpy())


def test_result_is_finite_and_paints():
    torch, lpt = _torch(), _lpt()
    from jax_nbody_emulator_with_dj_amd import density
    x = torch.from_numpy(np.float32(0.05) * red_field(16, 16, np.float32)).cuda()
    psi = lpt.lpt2_displacement(x, boxsize=L, dealias=True)
    assert torch.isfinite(psi).all()
    mesh = density.paint_density(psi, boxsize=L, res=16)
    mesh = mesh.cpu().numpy() if isinstance(mesh, torch.Tensor) else np.asarray(mesh)
    assert mesh.shape == (16, 16, 16) and np.isfinite(mesh).all() and np.abs(mesh).max() > 0


# ---- error paths through the C ABI ----------------------------------------------------------------------------------------------

def test_entry_points_refuse_bad_arguments():
    torch, lib = _torch(), _abi()
    l = lib.lib()
    t = torch.zeros(8192, dtype=torch.int64, device="cuda")
    p = C.c_void_p(t.data_ptr())
    q = C.c_void_p(t.data_ptr() + 32768)                    # 8^3 spectra of 8 * 8 * 5 * 8 = 2560 bytes: clear of p
    inside = C.c_void_p(t.data_ptr() + 512)                 # inside the six fields / the spectrum that start at p
    for call, name in ((lambda: l.nbe_lpt2_hessian_spectrum(None, 8, 0, 6, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, 0, 6, None, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, 0, 1, p, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, 0, 1, inside, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 1, 0, 1, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 2049, 0, 1, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, 1, 6, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, 6, 1, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, -1, 2, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_hessian_spectrum(p, 8, 0, 0, q, 0, None), "nbe_lpt2_hessian_spectrum"),
                       (lambda: l.nbe_lpt2_source(None, 8, q, 0, None), "nbe_lpt2_source"),
                       (lambda: l.nbe_lpt2_source(p, 8, None, 0, None), "nbe_lpt2_source"),
                       (lambda: l.nbe_lpt2_source(p, 8, p, 0, None), "nbe_lpt2_source"),
                       (lambda: l.nbe_lpt2_source(p, 8, inside, 0, None), "nbe_lpt2_source"),
                       (lambda: l.nbe_lpt2_source(p, 1, q, 0, None), "nbe_lpt2_source"),
                       (lambda: l.nbe_lpt2_spectrum(None, p, 8, 1.0, 1.0, 1.0, q, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, None, 8, 1.0, 1.0, 1.0, q, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, p, 8, 1.0, 1.0, 1.0, None, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, q, 8, 1.0, 1.0, 1.0, p, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(q, p, 8, 1.0, 1.0, 1.0, inside, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, p, 1, 1.0, 1.0, 1.0, q, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, p, 8, 0.0, 1.0, 1.0, q, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, p, 8, 1.0, float("nan"), 1.0, q, 0, None), "nbe_lpt2_spectrum"),
                       (lambda: l.nbe_lpt2_spectrum(p, p, 8, 1.0, 1.0, float("inf"), q, 0, None), "nbe_lpt2_spectrum")):
        rc = call()
        assert rc != 0
        with pytest.raises(lib.NBEError, match=name):
            lib.check(rc)
    torch.cuda.synchronize()
    assert not t.any()
