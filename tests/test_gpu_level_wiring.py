"""The wiring between the U-Net levels of the one-tile periodic schedule: down_l0 and down_l1 write the
interior of the next level's input, whose halo is filled and whose z context is copied in place; level 1 computes exactly the
planes of its skip connection; a fused conv_r1 reads concat([skip, up]) from conv_l1's result and a tensor of the up-sampled
half; nothing fills the halo or zeroes the padding channel planes of conv_r01's result, which only the head reads.

Only data movement differs from the padded schedule (NBE_PERIODIC=0 at context creation: every tile carries 48 voxels of
periodic padding and all levels shrink), so on the direct kernels the two give the same bits.  Boxes: 48^3, the smallest
periodic extent (the level-1 and level-2 context planes wrap furthest: 6 of 24 and 10 of 12), and 64 x 48 x 56, whose unequal
extents catch swapped axes.  Shallow boxes (depth 8, 16, 32) have fewer own planes at levels 1 and 2 than planes of context: the
context then spans several periods.

What these tests cannot see is WHICH path conv_r1 took: level 0 sets the two-source bits of `paths` already, and there is no
query key for level 1 (none may be added).  A wrong choice between two sources and the copy would still give the right fields;
that the two-source path runs at the benchmark width is shown by the kernel trace (the 3.2 ms copy is gone)."""

import numpy as np
import pytest

import jax_nbody_emulator_with_dj_amd as J
from conftest import rel_l2, max_over_rms

pytestmark = pytest.mark.gpu

Z, OM = 0.5, 0.3
PAD = ((48, 48),) * 3
SIZES = [(48, 48, 48), (64, 48, 56)]
# the level-1 / level-2 inputs have 4 / 2, 8 / 4 and 16 / 8 own planes for 6 / 10 planes of z context on either side
SHALLOW = [(8, 48, 48), (16, 48, 48), (32, 48, 56)]

_ENGINES, _FIELDS = {}, {}


def _engine(engine_factory, monkeypatch, mid, prec, periodic):
    """One context per (width, arithmetic, schedule): NBE_PERIODIC is read when a context is created."""
    key = (mid, prec, periodic)
    if key not in _ENGINES:
        from oracle import params as P
        monkeypatch.setenv("NBE_PERIODIC", "1" if periodic else "0")
        e = engine_factory(mid_chan=mid, precision=prec)
        e.load_params(P.synthetic_params(seed=29, mid_chan=mid), False)
        e.set_cosmology(OM, float(J.growth_factor(Z, OM)))
        _ENGINES[key] = e
    return _ENGINES[key]


def _box(size):
    return np.random.default_rng(31).standard_normal((3,) + size).astype(np.float32)


def _run(e, box, size):
    d, v = e.process_box(box, size, (1, 1, 1), PAD, float(J.growth_factor(Z, OM)), float(J.vel_norm(Z, OM)))
    return np.array(d), np.array(v)


def _fields(engine_factory, monkeypatch, mid, prec, size, periodic, wino):
    """(disp, vel) of the seeded box: computed once per configuration and shared, never modified."""
    key = (mid, prec, size, periodic, wino)
    if key not in _FIELDS:
        e = _engine(engine_factory, monkeypatch, mid, prec, periodic)
        monkeypatch.setenv("NBE_WINO", "1" if wino else "0")
        d, v = _run(e, _box(size), size)
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(v))
        if periodic:                                            # the test cannot pass on another schedule
            assert e.query("periodic_yx") == 1.0 and e.query("periodic_z") == 1.0 and e.query("slab") > 0
        else:
            assert e.query("periodic_yx") == 0.0
        d.setflags(write=False); v.setflags(write=False)
        _FIELDS[key] = (d, v)
    return _FIELDS[key]


@pytest.mark.parametrize("size", SIZES + SHALLOW)
def test_copy_free_path_equals_padded_schedule_f16x3(engine_factory, monkeypatch, size):
    """f16x3, disp + vel, mid 16: the narrowest width at which conv_r1 reads two sources.  Direct kernels: bit for bit.  Default
    kernels (Winograd-z): the bounds of tests/test_gpu_api.py::test_winograd_schedules_agree_to_rounding, restated."""
    d0, v0 = _fields(engine_factory, monkeypatch, 16, "f16x3", size, False, False)
    d1, v1 = _fields(engine_factory, monkeypatch, 16, "f16x3", size, True, False)
    print("f16x3 mid 16 %s direct kernels: disp differs at %d voxels, vel at %d" % (size, int((d1 != d0).sum()), int((v1 != v0).sum())))
    assert np.array_equal(d1, d0) and np.array_equal(v1, v0)
    dr, vr = _fields(engine_factory, monkeypatch, 16, "f16x3", size, False, True)
    dw, vw = _fields(engine_factory, monkeypatch, 16, "f16x3", size, True, True)
    ed = rel_l2(dw, dr), max_over_rms(dw, dr)
    rms_v = np.sqrt(np.mean(vr.astype(np.float64) ** 2))
    e = np.abs(vw.astype(np.float64) - vr) / rms_v
    inl = e <= 1e-3
    ev = (float(np.median(e)), float(np.sqrt(np.sum(((vw - vr) ** 2)[inl])) / np.linalg.norm(vr)), float((~inl).mean()))
    print("f16x3 mid 16 %s default kernels: disp rel_l2 %.2e max/rms %.2e; vel median %.2e inlier rel_l2 %.2e outliers %.4f" % ((size,) + ed + ev))
    assert ed[0] <= 3e-6 and ed[1] <= 3e-5, ed
    assert ev[0] <= 5e-6 and ev[1] <= 1e-4 and ev[2] <= 0.05, ev


@pytest.mark.parametrize("size", SIZES)
def test_copy_free_path_equals_padded_schedule_float16_model(engine_factory, monkeypatch, size):
    """The float16 model at mid 32, its two-source width, with the fused skip in the Winograd-z form (default kernels).  Held to
    what tests/test_gpu_api.py::test_periodic_yx_mode_is_identical asks of the same comparison -- periodic against padded
    schedule of the float16 model -- : float32 sums may differ in the last bit before a float16 rounding."""
    d0, v0 = _fields(engine_factory, monkeypatch, 32, "f16", size, False, True)
    d1, v1 = _fields(engine_factory, monkeypatch, 32, "f16", size, True, True)
    e = rel_l2(d1, d0), rel_l2(v1, v0)
    print("float16 model mid 32 %s default kernels: disp rel_l2 %.2e vel rel_l2 %.2e" % ((size,) + e))
    assert e[0] <= 1e-3 and e[1] <= 1e-2, e


@pytest.mark.parametrize("mid,prec", [(8, "f16x3"), (16, "f32")])
def test_fallbacks_keep_the_concat_copy(engine_factory, monkeypatch, mid, prec):
    """mid 8 has no two-source width (a 16-channel chunk would straddle the tensors) and the strict float32 blocks do not fuse:
    both still copy the skip connection into the concat tensor, and equal their own padded schedule bit for bit -- on the
    direct kernels and on the default ones (both schedules start every launch of this box on an even plane of the tile, so the
    Winograd-z kernel pairs the same planes)."""
    size = SIZES[0]
    for wino in (False, True):
        d0, v0 = _fields(engine_factory, monkeypatch, mid, prec, size, False, wino)
        d1, v1 = _fields(engine_factory, monkeypatch, mid, prec, size, True, wino)
        print("%s mid %d NBE_WINO=%d: disp differs at %d voxels, vel at %d" % (prec, mid, wino, int((d1 != d0).sum()), int((v1 != v0).sum())))
        assert np.array_equal(d1, d0) and np.array_equal(v1, v0), wino


def test_stale_halo_and_padding_planes_of_the_head_input_are_never_read(engine_factory, monkeypatch):
    """A box of NaN leaves NaN wherever the workspace was written (NaN in, NaN out: no error).  conv_r01's result then sits on
    NaN in its y/x halo and in its padding channel planes, which nothing fills or zeroes any more; a finite box on the same
    context must give the fields of a context that never saw the NaN, bit for bit."""
    size = SIZES[0]
    want = _fields(engine_factory, monkeypatch, 16, "f16x3", size, True, True)
    from oracle import params as P
    monkeypatch.setenv("NBE_PERIODIC", "1")
    monkeypatch.setenv("NBE_WINO", "1")
    e = engine_factory(mid_chan=16, precision="f16x3")
    e.load_params(P.synthetic_params(seed=29, mid_chan=16), False)
    e.set_cosmology(OM, float(J.growth_factor(Z, OM)))
    dn, vn = _run(e, np.full((3,) + size, np.nan, np.float32), size)
    assert np.isnan(dn).all() and np.isnan(vn).all()
    d, v = _run(e, _box(size), size)
    assert e.query("periodic_z") == 1.0
    assert np.array_equal(d, want[0]) and np.array_equal(v, want[1])
