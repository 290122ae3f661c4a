"""The network above width 64 on the GPU: the fall-back kernels the planners choose there, against the float64 oracle.

nbe_create accepts every width that is a multiple of 8, and width 64 is where most of the fast paths stop: the one-pass head
kernel (4 chunks), the one-launch up-sampling (4 chunks), the Winograd-z kernel (128 input channels, a 128-channel skip; 256 in
float16), the group table of the gauged direct kernel (64 entries).  tests/wide_cases.py restates what decides the launches of a
block and names six widths, each for the limits it meets (WIDTHS); tests/test_wide_cases.py holds that table to the limits on
the CPU.  Here every (width, block, form) of the table runs through test_gpu_blocks.run_case with all of its checks -- both stages
against tests/block_ref.py at the per-layer classes of tests/layer_checks.py, unchanged, the branches behind the activations,
the gauge vectors, the two-source form against the concat form -- and on top of that the profile labels, the launch counts and
the exact path word are held to the table, so that a block which falls to another kernel fails instead of passing on that
kernel's merits.  The per-layer classes were stated for K <= 27 * 128 + 128 products per output; the decoders reach
27 * 352 + 352 here: the worst figure per stage and width is printed by the last test (DESIGN.md section 2c records them).

Then, where a whole launch form has never run on a GPU:
  * conv_h3g_kernel<NARROW> (the head from width 72 on; it shares label and path bit with conv_h3nz_kernel) on the case list
    of tests/test_gpu_head.py and on 17 planes of 17 x 33 (102 workgroups), and its position independence bit for bit;
  * the eight-launch up-sampling in half precision, into the second half of a concat tensor;
  * the masked rows, columns and cout groups of ragged tiles after a NaN run on the same workspace;
  * the whole network at width 72 against tests/golden/golden_v5.npz, and the one-tile periodic schedule against the padded
    one bit for bit at widths 72 (level 1 copies the skip connection) and 80 (level 1 reads two sources)."""

import os
import time

import numpy as np
import pytest

import block_ref as B
import test_gpu_blocks as TB
import wide_cases as W
from conftest import rel_l2, max_over_rms
from oracle import layers as L
from stream_cases import rand
from test_gpu_blocks import engines  # noqa: F401  (the module-scoped engine cache, as a fixture of this module)
from test_gpu_fused_blocks import counted, _embed
from test_gpu_head import ZRUN, _shape
from test_gpu_patch_layers import loaded, set_wino  # noqa: F401  (loaded: a fresh loaded context per call, as a fixture)

pytestmark = pytest.mark.gpu

X3V = W.FORMS["w"]
T0 = [None]


def _gauge_deviation(mid):
    """as test_gpu_blocks._gauge_deviation, for one width"""
    s32 = np.array([(np.float32(TB.OM) - np.float32(0.3)) * np.float32(5.0), np.float32(TB.DZ) - np.float32(1.0)], np.float32)
    return max(float(np.abs(B.alpha(lp, s32).astype(np.float64) - B.alpha(lp, TB.s64())).max())
               for bp in TB.params_of(mid)['params'].values() for lp in bp.values())


def tree(mid):
    """one kind of tree per width (its table of worst figures): style parameters, the fusing rule of tests/wide_cases.py, and
    whether wire_gauge keeps the gauge at this width"""
    name = "wide-%d" % mid
    if name not in TB.TREES:
        TB.TREES[name] = TB.Tree(lambda m, vel: TB.params_of(m), W.expect_fused, _gauge_deviation(mid),
                                 gauge_active=W.gauge_active(mid, X3V))
    return name


def run(e, block, mid, form, shape):
    """run_case on one shape with the table's expectations on top: labels, launch counts, the exact path word"""
    if T0[0] is None:
        T0[0] = time.time()
    f = W.FORMS[form]
    gauge = W.gauge_active(mid, f) if f.vel else True
    srcs = W.sources(block, mid, form, shape, gauge)
    with L.backend('torch'):
        out, ran = counted(e, lambda: TB.run_case(e, block, mid, f.prec, f.vel, shape, gauge=gauge, wino_on=f.wino, forms=srcs,
                                                  tree=tree(mid)))
    want = W.labels(block, mid, form, shape, gauge)
    assert ran == want, (block, mid, form, shape, ran, want)
    if block in W.RES:
        assert set(out) == set(srcs), (sorted(out), srcs)
        for src, r in out.items():
            assert r["paths"] == W.paths(block, mid, form, shape, src, gauge), (src, r["paths"])
    if f.vel and not gauge:                                      # the gauge is off: every vector the engine returns is zero
        for r in out.values():
            assert not r["gauge_in"].any() and not r["gauge_out"].any() and (r["gauge_hidden"] is None or not r["gauge_hidden"].any())
    return out


# ---- every block of the table against the oracle ---------------------------------------------------------------------------------
@pytest.mark.parametrize("mid,block,form", W.MATRIX, ids=["m%d-%s-%s" % c for c in W.MATRIX])
def test_block_against_the_oracle(engines, mid, block, form, monkeypatch):  # noqa: F811
    f = W.FORMS[form]
    set_wino(monkeypatch, f.wino)
    e = engines(mid, f.prec, f.vel, tree=tree(mid))              # asserts gauge_active: false at 176, true below
    print("  width %d: %s" % (mid, W.WIDTHS[mid]))
    for shape in W.shapes(block, form):
        run(e, block, mid, form, shape)


# ---- conv_h3g_kernel<NARROW> at its tile edges -----------------------------------------------------------------------------------
def _head_cases(j):
    """the case list of tests/test_gpu_head.py for the j-th width (its y / x extents alternate with the plane count and the
    width), and 17 planes of 17 x 33: 3 x 2 tiles per plane, 102 workgroups"""
    yx = ((9, 33), (5, 7))
    return [_shape(n, *yx[(i + j) % 2]) for i, n in enumerate((1, 2, 3, 5))] + [_shape(ZRUN + 5, 8, 32), (6, 48, 56, 1), _shape(17, 17, 33)]


HEAD = [(mid, s) for j, mid in enumerate((72, 128)) for s in _head_cases(j)]


@pytest.mark.parametrize("mid,shape", HEAD, ids=["mid%d-%dx%dx%d-pad%d" % ((m,) + s) for m, s in HEAD])
def test_narrow_head_against_the_oracle(engines, mid, shape):  # noqa: F811
    la = W.launches('conv_r01', mid, "w", shape)[-1]
    assert la.kernel == "h3g_narrow" and la.nskip == W.nchunk(mid) > W.HNZ_MAXCH
    if shape == _shape(17, 17, 33):
        assert W.tiles_of(17, 8) * W.tiles_of(33, 32) * 17 == 102
    out = run(engines(mid, "f16x3", True, tree=tree(mid)), 'conv_r01', mid, "w", shape)
    assert all("narrow" in r["paths"] for r in out.values())


def test_narrow_head_is_position_independent(engines, monkeypatch):  # noqa: F811
    """tests/test_gpu_head.py::test_head_is_position_independent at width 80 (five whole chunks, five skip groups): under
    NBE_WINO=0 the hidden tensors of a volume and of its sub-volumes agree bit for bit, and conv_h3g_kernel<NARROW>, which sums its
    groups in a fixed order, must give a voxel the same bits wherever its tile begins: offsets (1, 3, 5) and (3, 3, 5)."""
    mid = 80
    monkeypatch.setenv("NBE_WINO", "0")
    e = engines(mid, "f16x3", True, tree=tree(mid))
    rng = np.random.default_rng(mid)
    x = rng.standard_normal((mid, ZRUN + 9, 18, 42)).astype(np.float32)
    dx = rng.standard_normal(x.shape).astype(np.float32)
    want = W.paths('conv_r01', mid, "g", x.shape[1:] + (0,))
    assert want == {"skip_fused", "narrow"}
    full, ran = counted(e, lambda: e.test_block('conv_r01', x, dx=dx))
    assert full["paths"] == want and ran == W.labels('conv_r01', mid, "g", x.shape[1:] + (0,)), (full["paths"], ran)
    for a, b, c in ((1, 3, 5), (3, 3, 5)):
        sub = e.test_block('conv_r01', np.ascontiguousarray(x[:, a:, b:, c:]), dx=np.ascontiguousarray(dx[:, a:, b:, c:]))
        assert sub["paths"] == want
        for k in ("h", "dh"):
            assert np.array_equal(sub[k], full[k][:, a:, b:, c:]), "hidden tensors differ in %s at offset %s" % (k, (a, b, c))
        for k in ("y", "dy"):
            assert sub[k].shape == full[k][:, a:, b:, c:].shape and np.abs(sub[k]).max() > 0
            assert np.array_equal(sub[k], full[k][:, a:, b:, c:]), "%s depends on where the volume begins (offset %s)" % (k, (a, b, c))


# ---- eight launches per up-sampling ----------------------------------------------------------------------------------------------
UP = [("up_r0", (2, 8, 12, 1)), ("up_r1", (2, 6, 10, 0))]


@pytest.mark.parametrize("form", ["w", "h", "n"])
@pytest.mark.parametrize("block,shape", UP, ids=["up_r0-periodic", "up_r1"])
def test_eight_parity_upsampling_into_a_concat_tensor(engines, block, shape, form):  # noqa: F811
    """Width 72 (five chunks: no up_h3_kernel): eight conv_h3_kernel<FLAT1> launches, one per parity, write the second half of
    a concat tensor.  The skip half must come back bit for bit; output voxel 2 i + parity depends on input voxel i alone, so the
    result of an input embedded in a larger one (lead (1, 2, 3): every voxel at another place of its 256-voxel tile) must equal
    the small one bit for bit.  (Against the oracle: test_block_against_the_oracle, on the same blocks.)"""
    mid, f = 72, W.FORMS[form]
    D, H, W_, pad = shape
    e = engines(mid, f.prec, f.vel, tree=tree(mid))
    rng = np.random.default_rng(72)
    x, dx = rand(rng, mid, D, H, W_), (rand(rng, mid, D, H, W_) if f.vel else None)
    q = lambda: (np.round(rng.standard_normal((mid, 2 * D, 2 * H, 2 * W_)) * 64).clip(-256, 256) / 64).astype(np.float32)
    sk, dsk = q(), (q() if f.vel else None)
    lead, trail = (1, 2, 3), (1, 1, 1)
    X, DX = _embed(x, lead, trail), _embed(dx, lead, trail)
    SK, DSK = (_embed(a, [2 * n for n in lead], [2 * n for n in trail]) for a in (sk, dsk))
    assert np.abs(X).max() == np.abs(x).max() and np.abs(SK).max() == np.abs(sk).max()
    label = W.launches(block, mid, form, shape)[0].label
    assert W.labels(block, mid, form, shape) == {label: 16} and "FLAT1" in label and W.paths(block, mid, form, shape) == set()
    small, ran = counted(e, lambda: e.test_block(block, x, dx=dx, x2=sk, dx2=dsk, pad=pad))
    assert ran == {label: 8} and small["paths"] == set(), (ran, small["paths"])
    large, ran = counted(e, lambda: e.test_block(block, X, dx=DX, x2=SK, dx2=DSK, pad=pad))
    assert ran == {label: 8} and large["paths"] == set(), (ran, large["paths"])
    dz, dy, dx_ = (2 * n for n in lead)
    for k, half_, big in (("y", sk, SK), ("dy", dsk, DSK)):
        if small[k] is None:
            continue
        assert np.array_equal(small[k][:mid], half_) and np.array_equal(large[k][:mid], big), "the skip half of the concat tensor changed (%s)" % k
        up = small[k][mid:]
        assert up.shape == (mid, 2 * D, 2 * H, 2 * W_) and np.all(np.isfinite(up)) and np.abs(up).max() > 0
        common = large[k][mid:, dz:dz + 2 * D, dy:dy + 2 * H, dx_:dx_ + 2 * W_]
        assert np.array_equal(common, up), "%s %s: %d of %d values differ after the shift by %s" % (block, k, int((common != up).sum()), up.size, lead)


# ---- masked stores ---------------------------------------------------------------------------------------------------------------
HALO = [('conv_r01', 80), ('conv_r00', 72)]


@pytest.mark.parametrize("form", ["w", "g"])
@pytest.mark.parametrize("block,mid", HALO, ids=["r01-m80", "r00-m72"])
def test_masked_stores_after_a_nan_run(loaded, block, mid, form, monkeypatch):  # noqa: F811
    """tests/test_gpu_fused_blocks.py's method at a result of 4 x 9 x 33 (2 x 2 tiles whose last ones hold one row, one column).
    conv_r01 at width 80: conv_h3g_kernel<NARROW> stores 3 of its 16 couts.  conv_r00 at width 72: 144 -> 144 -> 72 on
    conv_h3g_kernel<false>, three cout tiles of which the last holds 16 of 64 channels, then two with 8 of 64.  After a NaN run
    of the same shape the workspace holds NaN wherever a tensor lay; the finite case on it must give finite results with the
    bits of a context that never saw the NaN."""
    f = W.FORMS[form]
    set_wino(monkeypatch, f.wino)
    dv = (4, 9, 33)
    shape = (dv[0] + 4, dv[1] + 4, dv[2] + 4, 0)
    c0, c1 = W.launches(block, mid, form, shape)
    assert c1.nskip > 0 and c1.kernel == ("h3g_narrow" if block == 'conv_r01' else "h3g_wide")
    if block == 'conv_r00':
        assert (W.nct(c0.cout), W.nct(c1.cout), c0.cout % 64, c1.cout % 64) == (3, 2, 16, 8)
    cin = B.channels(block, mid)[0]
    rng = np.random.default_rng(47)
    x, dx = rand(rng, cin, *shape[:3]), rand(rng, cin, *shape[:3])
    want = loaded(f.prec, mid, f.vel).test_block(block, x, dx=dx)
    e = loaded(f.prec, mid, f.vel)
    nan = np.full_like(x, np.nan)
    out = e.test_block(block, nan, dx=nan)
    assert out["y"].shape == (c1.cout,) + dv and np.isnan(out["y"]).all() and np.isnan(out["dy"]).all()
    got, ran = counted(e, lambda: e.test_block(block, x, dx=dx))
    assert ran == W.labels(block, mid, form, shape), ran
    assert got["paths"] == want["paths"] == W.paths(block, mid, form, shape), (got["paths"], want["paths"])
    for k in ("y", "dy", "h", "dh"):
        assert np.all(np.isfinite(want[k])) and np.all(np.isfinite(got[k])) and np.abs(want[k]).max() > 0
        assert np.array_equal(got[k], want[k]), "%s differs after a NaN run on the same workspace" % k


# ---- the whole network -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    from oracle import params as P
    g = np.load(os.path.join(os.path.dirname(__file__), "golden", "golden_v5.npz"))
    seed_p, seed_x, mid, d0, d1, d2 = (int(t) for t in g["net72_meta"])
    x = np.random.default_rng(seed_x).standard_normal((1, 3, d0, d1, d2)).astype(np.float32)[0]
    return P.synthetic_params(seed=seed_p, mid_chan=mid), mid, x, g["net72_disp"], g["net72_vel"]


@pytest.mark.parametrize("prec", ["f32", "f16x3", "f16"])
def test_whole_network_at_width_72(engine_factory, golden, prec):
    """104^3 -> 8^3 against the float64 oracle (tests/golden/make_golden_v5.py): f32 and f16x3 at the bounds of
    tests/test_gpu_model.py::_check (2e-5 / 2e-4 and 5e-5 / 2e-4), the float16 model at that module's float16 bounds
    (2e-3 / 4e-2) against the fixture.

    The fixture's velocity follows the oracle's own branches at every LeakyReLU, and this input has activations in the
    level-0 and level-1 encoder blocks whose pre-activation is zero to within 3e-6 RMS of their tensor: the library takes the
    other branch at 34 (f16x3) and 47 (f32) of 3.0e8 activations, the largest of them at 9.5e-7 and 2.8e-6 RMS (kink.FLIP_TOL is
    2e-5), and its velocity then differs from the fixture's by rel-L2 3.28e-4, max/RMS 3.26e-3 in both arithmetics -- outside
    _check -- while the displacement, which does not depend on the branches, agrees to 3.9e-7 / 7.8e-7.  So the velocity of f32
    and f16x3 is held to the same bounds causally, the way tests/test_gpu_kink.py::test_config1_velocity_is_exact_given_the_branches
    does at width 64: the float64 oracle of the same input with the library's own branch decisions (kink.oracle_cone; the cone of
    the whole 8^3 output is the whole input) must agree on every voxel of both fields (measured: velocity 4.4e-7 / 1.4e-6 f16x3,
    8.5e-7 / 3.0e-6 f32), and every branch that differs from the oracle's own must sit within kink.FLIP_TOL of zero.  The
    displacement is held to the committed fixture as well.  (One float64 evaluation per arithmetic: about 20 s each.)"""
    import kink
    from test_gpu_model import _check, DZ, VF, OM
    p, mid, x, d_o, v_o = golden
    e = engine_factory(mid_chan=mid, compute_vel=True, precision=prec)
    e.load_params(p, premodulated=False)
    e.set_cosmology(OM, DZ)
    assert bool(e.query("gauge_active"))
    if prec != "f16":
        e.probe_begin((0, 0, 0), 8)
    try:
        (d, v), ran = counted(e, lambda: e.forward(x, DZ, VF))
        br = e.probe_read() if prec != "f16" else None
    finally:
        if prec != "f16":
            e.probe_end()
    print("  width %d %s against the fixture: disp rel-L2 %.2e max/RMS %.2e, vel rel-L2 %.2e max/RMS %.2e" % (
        mid, prec, rel_l2(d, d_o), max_over_rms(d, d_o), rel_l2(v, v_o), max_over_rms(v, v_o)))
    assert d.shape == d_o.shape == (3, 8, 8, 8)
    assert not any(k.startswith("up_h3") for k in ran), sorted(ran)
    if prec == "f16x3":
        assert ran.get("conv_h3n<FLAT3,vel,dx>") == 1 and "conv_h3g<FLAT3,vel,dx>" in ran, sorted(ran)
    if prec == "f16":
        assert np.all(np.isfinite(d)) and np.all(np.isfinite(v))
        assert rel_l2(d, d_o) <= 2e-3 and rel_l2(v, v_o) <= 4e-2
        return
    _check(d, None, d_o, None, "style-vel mid%d %s" % (mid, prec))
    d_c, v_c, st = kink.oracle_cone(p, x, OM, DZ, VF, br)
    kink.assert_cone("style-vel mid%d %s" % (mid, prec), d, v, d_c, v_c, st)     # its default bounds are _check's


@pytest.mark.parametrize("mid", [72, 80])
def test_one_tile_periodic_schedule_equals_the_padded_one(engine_factory, monkeypatch, mid):
    """tests/test_gpu_level_wiring.py at widths 72 and 80, f16x3 on the direct kernels (NBE_WINO=0), a 48^3 box: only data
    movement differs between the schedules, so the fields agree bit for bit.  By the planner's rule (two_source_width, restated
    in tests/wide_cases.py and asserted here on that table only) width 72 has no two-source width -- a 16-channel chunk would
    straddle the tensors, so level 1 should copy its skip connection into the concat tensor -- and width 80 has one.  WHICH path
    level 1 took is not visible from here: there is no query key for it (tests/test_gpu_level_wiring.py says the same of width
    16).  What is checked on the engine is that both widths give the padded schedule's bits, whichever path they take."""
    import test_gpu_level_wiring as LW
    size = LW.SIZES[0]
    assert W.two_source_width(mid, "f16x3") == (mid == 80)
    d0, v0 = LW._fields(engine_factory, monkeypatch, mid, "f16x3", size, False, False)
    d1, v1 = LW._fields(engine_factory, monkeypatch, mid, "f16x3", size, True, False)
    print("  f16x3 mid %d %s direct kernels: disp differs at %d voxels, vel at %d" % (mid, size, int((d1 != d0).sum()), int((v1 != v0).sum())))
    assert np.abs(d0).max() > 0 and np.abs(v0).max() > 0
    assert np.array_equal(d1, d0) and np.array_equal(v1, v0)


def test_zz_worst_cases():
    """prints the worst figure per width, stage, arithmetic and tolerance class of this run (DESIGN.md section 2c records them)"""
    print("\n  width | stage | arithmetic | class | worst rel-L2 (bound) | worst max/RMS (bound)")
    for mid in W.WIDTHS:
        for (stage, arith, cls), (e2, em) in sorted(TB.TREES[tree(mid)].worst.items()):
            print("  %3d | %-26s | %-10s | %-4s | %.2e (%.0e) | %.2e (%.0e)" % (mid, stage, arith, cls, e2, TB.TOL[cls][0], em, TB.TOL[cls][1]))
    if T0[0] is not None:
        print("  wall time of this module so far: %.0f s" % (time.time() - T0[0]))
