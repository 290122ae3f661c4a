"""The first layer (stem_h3_kernel), 2x up-sampling (up_h3_kernel, eight parities in one launch) and the stride-2 / unfused
1x1x1 layers (conv_h3_kernel<MODE_DOWN / MODE_FLAT1>, conv_mfma_kernel in strict float32) at the edges of their own tiling:
against the float64 oracle, for position independence bit by bit, and for what their masked lanes leave alone.

Parity.  Every case of tests/stream_cases.py (the tiling it rests on is restated there) runs through the production launch
path (nbe_test_layer -> run_conv) on f16x3 with velocity; the cases marked `rep` also on the other five (arithmetic,
velocity) combinations -- f32 / f16x3 / f16, with and without velocity (stem: dW without dX).  Those are, per family, one case
per residue class of the tile count and one per tiles-per-workgroup class:
  stem  w33 (ragged tile), w128 (whole tile), w129 (tnx = 2, one column in the second tile): one tile per workgroup;
        nt513 (workgroup 0 runs two tiles), nt1548 (every workgroup three or four: a patch buffer is used again);
  up    row255 / row256 / row257 (Q = 255, 256, 257), 9x15x17 (nine tiles, an XCD with two);
  down  q255 / q256 / q257, q2322 (ten tiles, two XCDs with two), odd (odd input extents);
  skip  q255 / q256 / q257 (128 -> 64, 64 -> 3, 3 -> 64 without input tangent), pitch-128-64 (rows and a plane gap masked).
Operands and oracle as test_gpu_layers.py::test_layer_vel builds them (float16 operands rounded for the float16 model,
LeakyReLU on), held by layer_checks._chk to the per-layer classes 5e-6 / 1e-4 (f32, f16x3) and 5e-4 / 5e-3 (f16): no
tolerance of this module's own.  Each case asserts the profile entry run_conv records, so that a case which falls to another
kernel fails instead of passing on that kernel's merits.

Position independence.  All these kernels give an output a K sum of fixed order, so its bits must not depend on where its
tile begins; the volumes are chosen so that the compared voxels change tile, tile half and wave quarter, and for the stem
the iteration and patch buffer of their persistent workgroup (numbers in each test's docstring)."""

import zlib

import numpy as np
import pytest

import stream_cases as S
import test_gpu_blocks as TB
from conftest import rel_l2, max_over_rms
from layer_checks import RTOL_L2, RTOL_MAX, RTOL_L2_F16, RTOL_MAX_F16, _chk, _h
from oracle import layers as L

pytestmark = pytest.mark.gpu

HALF_PRECS = ("f16x3", "f16")
COMBOS = [(p, v) for p in ("f32", "f16x3", "f16") for v in (True, False)]
WORST = {}                                     # (kernel, arithmetic) -> [rel-L2, max/RMS]
MODE = {"conv3": "FLAT3", "skip": "FLAT1", "down": "DOWN", "up": "FLAT1"}


@pytest.fixture(scope="module")
def engines(engine_factory):
    made = {}

    def get(prec):
        if prec not in made:
            made[prec] = engine_factory(precision=prec)
        return made[prec]
    return get


@pytest.fixture(scope="module")
def loaded(engine_factory):
    """production width, a loaded network: the blocks' own launches (nbe_test_block)"""
    made = {}

    def get(prec, mid=64, fresh=False):
        if fresh or (prec, mid) not in made:
            e = engine_factory(mid_chan=mid, precision=prec, compute_vel=True)
            e.load_params(TB.params_of(mid), False)
            e.set_cosmology(TB.OM, TB.DZ)
            if fresh:
                return e
            made[(prec, mid)] = e
        return made[(prec, mid)]
    return get


def kernel_name(case, prec, vel):
    """the profile entry run_conv gives the launch (conv_label, csrc/nbe_conv_select.h)"""
    tang = "vel,%s" % ("dx" if case.has_dx else "nodx") if vel else "novel,nodx"
    if prec == "f32":
        return "conv_mfma<%s,%s,ni" % (MODE[case.kind], tang)
    if case.kind == "conv3":
        return "stem_h3<FLAT3,vel,nodx>" if vel else "stem_h3<FLAT3,novel>"
    if case.kind == "up":
        return "up_h3<8 parities,vel,dx>" if vel else "up_h3<8 parities,novel>"
    return "%s<%s,%s>" % ("conv_h1" if prec == "f16" else "conv_h3", MODE[case.kind], tang)


def profiled(e, run):
    e.profile_reset()
    e.profile_enable(True)
    try:
        out = run()
        prof = e.profile_read()
    finally:
        e.profile_enable(False)
    return out, [p["kernel"] for p in prof if p["launches"] > 0]


# ---- parity ----------------------------------------------------------------------------------------------------------------------
PARITY = [(c, p, v) for c in S.CASES for p, v in COMBOS if c.rep or (p, v) == ("f16x3", True)]
_REF = {}                                      # the current case's operands and oracle, per operand rounding: computed once


def reference(case, half):
    """operands and float64 oracle (value and tangent, behind the activation) of a case; kept for the run of tests of that case"""
    if _REF.get("case") != case.name:
        _REF.clear()
        _REF["case"] = case.name
        _REF["ops"] = S.operands(case)
    if half not in _REF:
        x, dx, w, dw, b = _REF["ops"]
        f = lambda a: None if a is None else _h(a, half).astype(np.float64)
        y, dy = L.conv_layer_vel(case.kind, f(x), f(dx), f(w), f(dw), b.astype(np.float64))
        if case.crop:
            cr = slice(case.crop, -case.crop)
            y, dy = y[:, cr, cr, cr], dy[:, cr, cr, cr]
        y, dy = L.leaky_relu_vel(y, dy)
        for a in (y, dy):
            a.setflags(write=False)
        _REF[half] = (y, dy)
    return _REF["ops"], _REF[half]


def _note(kern, prec, half, got, want, what):
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    print("  %-40s rel-L2 %.2e  max/RMS %.2e" % (what, e2, em))
    w = WORST.setdefault((kern, prec), [0.0, 0.0])
    w[0], w[1] = max(w[0], e2), max(w[1], em)
    _chk(got, want, what, half)


@pytest.mark.parametrize("case,prec,vel", PARITY, ids=["%s-%s-%s" % (c.name, p, "vel" if v else "novel") for c, p, v in PARITY])
def test_against_oracle(engines, case, prec, vel):
    e = engines(prec)
    half = prec == "f16"
    (x, dx, w, dw, b), (y_o, dy_o) = reference(case, half)
    if vel:
        (y, dy), ran = profiled(e, lambda: e.test_layer(case.kind, x, w, b, dx=dx, dw=dw, crop=case.crop, act=True))
    else:
        y, ran = profiled(e, lambda: e.test_layer(case.kind, x, w, b, crop=case.crop, act=True))
    want = kernel_name(case, prec, vel)
    assert ran and all(k.startswith(want) for k in ran), (want, ran)
    kern = "%s %s" % (want.split("<")[0], "stem" if case.kind == "conv3" else case.kind)
    _note(kern, prec, half, y, y_o, "%s value" % case.name)
    if vel:
        _note(kern, prec, half, dy, dy_o, "%s tangent" % case.name)


# ---- position independence ----------------------------------------------------------------------------------------------------------
def _operands(kind, cin, cout, dims, seed):
    rng = np.random.default_rng(seed)
    k = S.K[kind]
    x, dx = S.rand(rng, cin, *dims), S.rand(rng, cin, *dims)
    w = (S.rand(rng, cout, cin, k, k, k) / np.sqrt(cin * k ** 3)).astype(np.float32)
    dw = (S.rand(rng, cout, cin, k, k, k) / np.sqrt(cin * k ** 3)).astype(np.float32)
    return x, dx, w, dw, 0.1 * S.rand(rng, cout)


def _sub(a, off):
    return np.ascontiguousarray(a[:, off[0]:, off[1]:, off[2]:])


def _same_bits(e, kind, ops, offsets, out_off, crop=0, has_dx=True, want=None):
    x, dx, w, dw, b = ops
    run = lambda xx, dd: e.test_layer(kind, xx, w, b, dx=dd if has_dx else None, dw=dw, crop=crop, act=True)
    (y, dy), ran = profiled(e, lambda: run(x, dx))
    assert ran and all(k.startswith(want) for k in ran), (want, ran)
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(dy)) and np.abs(y).max() > 0 and np.abs(dy).max() > 0
    for off, oo in zip(offsets, out_off):
        ys, dys = run(_sub(x, off), _sub(dx, off))
        for name, got, full in (("y", ys, y), ("dy", dys, dy)):
            ref = full[:, oo[0]:, oo[1]:, oo[2]:]
            assert got.shape == ref.shape, (name, off, got.shape, ref.shape)
            assert np.array_equal(got, ref), "%s depends on where the volume begins (offset %s): %d of %d voxels differ" % (
                name, off, int((got != ref).sum()), got.size)


OFFSETS = ((1, 3, 5), (3, 3, 5))


@pytest.mark.parametrize("prec", HALF_PRECS)
def test_stem_is_position_independent(engines, prec):
    """3 -> 64 on a (7, 70, 140) input: 5 x 68 x 138 outputs, tnx = 2, 680 tiles on 512 workgroups -- the voxels of tiles
    512 .. 679 (plane 3 from row 52, plane 4) are their workgroup's second tile, staged in patch buffer 1.  From offset
    (1, 3, 5) the volume has 4 x 65 x 133 outputs in 520 tiles, from (3, 3, 5) 2 x 65 x 133 in 260: all but eight tiles of
    the first, and all of the second, are first tiles in buffer 0, so nearly every voxel that ran in iteration 1 now runs in
    iteration 0 of another workgroup.  The x offset 5 moves every voxel five columns: 5 of 32 change wave, columns 128 .. 132
    change tile."""
    full, sub = S.stem_tiling((7, 70, 140)), S.stem_tiling((6, 67, 135))
    assert (full.nt, sub.nt, S.stem_tiling((4, 67, 135)).nt) == (680, 520, 260)
    assert S.stem_place(full, 4, 10, 40)[1:] == (1, 1, 1) and S.stem_place(sub, 3, 7, 35)[1:] == (0, 0, 1)
    assert S.stem_place(full, 0, 3, 130)[0] % 2 == 1 and S.stem_place(sub, 0, 0, 125)[0] % 2 == 0
    ops = _operands("conv3", 3, 64, (7, 70, 140), 11)
    _same_bits(engines(prec), "conv3", ops, OFFSETS, OFFSETS, has_dx=False, want="stem_h3<FLAT3,vel,nodx>")


@pytest.mark.parametrize("prec", HALF_PRECS)
def test_up_is_position_independent(engines, prec):
    """64 -> 64 on (5, 9, 23): 1035 positions, five tiles; from (1, 3, 5) it is (4, 6, 18) = 432 positions, from (3, 3, 5)
    (2, 6, 18) = 216.  Input voxel (4, 8, 22) is position 1034 (tile 4, half 0, quarter 0, lane 10) of the volume, 431 (tile 1,
    half 1, quarter 1, lane 15) and 215 (tile 0, half 1, quarter 2, lane 23) of the sub-volumes; its eight outputs are stored
    at offsets 2 (a, b, c) lower."""
    assert [S.up_place(q) for q in (1034, 431, 215)] == [(4, 0, 0, 10), (1, 1, 1, 15), (0, 1, 2, 23)]
    ops = _operands("up", 64, 64, (5, 9, 23), 12)
    _same_bits(engines(prec), "up", ops, OFFSETS, [tuple(2 * o for o in off) for off in OFFSETS], want="up_h3<8 parities,vel,dx>")


@pytest.mark.parametrize("prec", HALF_PRECS)
def test_skip_is_position_independent(engines, prec):
    """the unfused 1x1x1 skip with its centre crop (in_off != 0, Wv < W), 128 -> 64 on (8, 10, 30): 4 x 6 x 26 outputs on the
    input's pitch, Q = (3 x 10 + 5) x 30 + 26 = 1076, five tiles; from (1, 3, 5) Q = (2 x 7 + 2) x 25 + 21 = 421, from
    (3, 3, 5) Q = 2 x 25 + 21 = 71: output (3, 5, 25) is position 1075 (tile 4), 420 (tile 1) and 70 (tile 0)."""
    assert [S.flat_q("skip", d, 2) for d in ((8, 10, 30), (7, 7, 25), (5, 7, 25))] == [1076, 421, 71]
    ops = _operands("skip", 128, 64, (8, 10, 30), 13)
    _same_bits(engines(prec), "skip", ops, OFFSETS, OFFSETS, crop=2,
               want="%s<FLAT1,vel,dx>" % ("conv_h1" if prec == "f16" else "conv_h3"))


@pytest.mark.parametrize("prec", HALF_PRECS)
def test_down_is_position_independent(engines, prec):
    """even offsets keep the stride-2 phase: input offsets (2, 4, 6) and (4, 2, 10) move the outputs by (1, 2, 3) and (2, 1, 5).
    64 -> 64 on (10, 12, 44): 5 x 6 x 22 = 660 outputs, three tiles; the sub-volumes have 4 x 4 x 19 = 304 (two tiles) and
    3 x 5 x 17 = 255 (one): output (4, 5, 21) is position 659 (tile 2, wave pair 2), 303 (tile 1, pair 0) and 254 (tile 0, pair 3)."""
    assert [S.flat_q("down", d) for d in ((10, 12, 44), (8, 8, 38), (6, 10, 34))] == [660, 304, 255]
    ops = _operands("down", 64, 64, (10, 12, 44), 14)
    _same_bits(engines(prec), "down", ops, ((2, 4, 6), (4, 2, 10)), ((1, 2, 3), (2, 1, 5)),
               want="%s<DOWN,vel,dx>" % ("conv_h1" if prec == "f16" else "conv_h3"))


def _block_input(rng, *shape):
    """the block hook shifts the range by max |x| of what goes in (a power of two): the largest value sits in the last voxel,
    which every sub-volume keeps, so that all of them run at the same scale"""
    x = S.rand(rng, *shape)
    x[0, -1, -1, -1] = 7.5
    assert np.abs(x).max() == 7.5
    return x


@pytest.mark.parametrize("prec", HALF_PRECS)
def test_up_r0_is_position_independent(loaded, prec, monkeypatch):
    """up_r0 as the periodic-yx schedule launches it: the input carries a one-voxel halo that is not up-sampled (in_off != 0,
    Wv = W - 2), and the result goes to the interior of the second half of the concat tensor (out_g0 != 0, a halo round it).
    (4, 7, 21) on a pitch of 9 x 23: Q = (3 x 9 + 6) x 23 + 21 = 780, four tiles; the sub-volumes (3, 4, 16) and (1, 4, 16)
    have Q = (2 x 6 + 3) x 18 + 16 = 286 and 3 x 18 + 16 = 70."""
    monkeypatch.setenv("NBE_WINO", "0")
    e = loaded(prec)
    rng = np.random.default_rng(21)
    x, dx = _block_input(rng, 64, 4, 7, 21), S.rand(rng, 64, 4, 7, 21)
    x2, dx2 = S.rand(rng, 64, 8, 14, 42), S.rand(rng, 64, 8, 14, 42)
    full, ran = profiled(e, lambda: e.test_block('up_r0', x, dx=dx, x2=x2, dx2=dx2, pad=1))
    assert "up8" in full["paths"] and ran == ["up_h3<8 parities,vel,dx>"], (full["paths"], ran)
    assert np.abs(full["y"][64:]).max() > 0 and np.abs(full["dy"][64:]).max() > 0
    for off in OFFSETS:
        o2 = tuple(2 * o for o in off)
        sub = e.test_block('up_r0', _sub(x, off), dx=_sub(dx, off), x2=_sub(x2, o2), dx2=_sub(dx2, o2), pad=1)
        for k in ("y", "dy"):
            ref = full[k][:, o2[0]:, o2[1]:, o2[2]:]
            assert sub[k].shape == ref.shape and np.all(np.isfinite(ref))
            assert np.array_equal(sub[k], ref), "%s depends on where the volume begins (offset %s)" % (k, off)


@pytest.mark.parametrize("prec", HALF_PRECS)
def test_conv_l00_hidden_is_position_independent(loaded, prec, monkeypatch):
    """conv_l00/conv_0 of the loaded network is the stem launch the schedule makes: on f16x3 its block is fused, so the hidden
    tensor has the INPUT's pitch (Ho, Wo) = (H, W) != (Hv, Wv).  A residual block needs five planes, so the volume is
    (8, 70, 140): hidden tensors of 6 x 68 x 138, 5 x 65 x 133 and 3 x 65 x 133 voxels in 816, 650 and 390 tiles -- hidden voxel
    (5, 60, 40) is tile 800 (second tile of its workgroup, patch buffer 1), from (1, 3, 5) tile 634 (second tile, buffer 1 of
    another workgroup) and from (3, 3, 5) tile 374 (first tile, buffer 0)."""
    tl = [S.stem_tiling(d) for d in ((8, 70, 140), (7, 67, 135), (5, 67, 135))]
    assert [t.nt for t in tl] == [816, 650, 390]
    assert [S.stem_place(t, *v)[:3] for t, v in zip(tl, ((5, 60, 40), (4, 57, 35), (2, 57, 35)))] == [(800, 1, 1), (634, 1, 1), (374, 0, 0)]
    monkeypatch.setenv("NBE_WINO", "0")
    e = loaded(prec)
    x = _block_input(np.random.default_rng(22), 3, 8, 70, 140)
    full, ran = profiled(e, lambda: e.test_block('conv_l00', x))
    assert "stem_h3<FLAT3,vel,nodx>" in ran, ran
    assert not full["paths"] & {"wino_0", "wino_1"}, full["paths"]
    for off in OFFSETS:
        sub = e.test_block('conv_l00', _sub(x, off))
        for k in ("h", "dh"):
            ref = full[k][:, off[0]:, off[1]:, off[2]:]
            assert sub[k].shape == ref.shape and np.all(np.isfinite(ref)) and np.abs(ref).max() > 0
            assert np.array_equal(sub[k], ref), "%s depends on where the volume begins (offset %s)" % (k, off)


# ---- what the masked lanes leave alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("block,shape", [("up_r0", (3, 7, 13)), ("down_l0", (6, 10, 38))], ids=["up", "down"])
@pytest.mark.parametrize("prec", HALF_PRECS)
def test_masked_lanes_neither_read_into_nor_write_past_the_result(loaded, prec, block, shape):
    """A NaN input of the same shape leaves NaN wherever the context's workspace was written (NaN in, NaN out: no error),
    also behind the tensors, where the last tile's masked lanes point: up (3, 7, 13) has 273 positions, 17 in its second tile;
    down (6, 10, 38) has 3 x 5 x 19 = 285 outputs, 29 in its second tile and 227 clamped entries of inbase.  The finite case
    on that workspace must give the bits of a context that never saw the NaN (mid 24: a ragged last channel group)."""
    mid = 24
    rng = np.random.default_rng(zlib.crc32(block.encode()))
    x, dx = _block_input(rng, mid, *shape), S.rand(rng, mid, *shape)
    want = loaded(prec, mid, fresh=True).test_block(block, x, dx=dx)
    e = loaded(prec, mid, fresh=True)
    nan = np.full_like(x, np.nan)
    out = e.test_block(block, nan, dx=nan)
    assert np.isnan(out["y"]).all() and np.isnan(out["dy"]).all()
    got, ran = profiled(e, lambda: e.test_block(block, x, dx=dx))
    kern = "up_h3<8 parities,vel,dx>" if block == "up_r0" else "%s<DOWN,vel,dx>" % ("conv_h1" if prec == "f16" else "conv_h3")
    assert ran == [kern], ran
    for k in ("y", "dy"):
        assert np.all(np.isfinite(want[k])) and np.abs(want[k]).max() > 0
        assert np.array_equal(got[k], want[k]), "%s differs after a NaN run on the same workspace" % k


def test_zz_worst_cases():
    """prints the worst figure per kernel and arithmetic of this run against the class it is held to"""
    print("\n  kernel | arithmetic | worst rel-L2 (bound) | worst max/RMS (bound)")
    for (kern, prec), (e2, em) in sorted(WORST.items()):
        t2, tm = (RTOL_L2_F16, RTOL_MAX_F16) if prec == "f16" else (RTOL_L2, RTOL_MAX)
        print("  %-18s | %-5s | %.2e (%.0e) | %.2e (%.0e)" % (kern, prec, e2, t2, em, tm))
