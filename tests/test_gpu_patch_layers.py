"""The 3x3x3 patch kernels (conv_h3q / h3g / h2q / h3p_kernel) and the Winograd-z kernel (conv_h3w_kernel, three forms) at the
edges of their own tiling: against the float64 oracle, for position independence bit by bit, and for what the masked part of
a ragged patch leaves alone.  Strict float32 (conv_mfma_kernel in FLAT3 mode and its gauged form) runs the same cases.

Parity.  Every case of tests/patch_cases.py (the tiling and the kernel selection it rests on are restated there) runs through
the layer hooks (nbe_test_layer, nbe_test_layer_gauged -> run_conv) on f16x3 in the gauged form -- conv_h3w_kernel where the
launch has a Winograd-z form, and conv_h3g_kernel under NBE_WINO=0; the cases marked `rep` also on
  f16x3    plain tangent (conv_h3q), displacement only with and without NBE_WINO=0 (conv_h3w NOVEL, conv_h2q<true>),
  float16  gauged (conv_h3w F16, or conv_h2q<false, true> where the chunk count is odd), plain tangent (conv_h2q<false>),
           displacement only (conv_h3p),
  float32  plain tangent and gauged (conv_mfma, conv_mfma_g);
the cases with a residual (cases of their own: a residual takes the f16x3 gauged launch to conv_h3g) also on conv_h3q and on
the float16 gauged kernels (the Winograd-z F_RES epilogue, conv_h2q).
One set of operands per case serves every form: unit-norm weight rows as the modulation leaves them, beta for the gauged
forms (oracle: dw = w beta, as test_gpu_layers.py::test_layer_gauged), a drawn dw for the plain ones; float16 operands rounded
for the float16 model.  The oracle's three products W.x, W.dx and dW.x are evaluated once per case and rounding.  Held by
layer_checks._chk to the per-layer classes 5e-6 / 1e-4 (f32, f16x3) and 5e-4 / 5e-3 (f16), conv_h1w by _chk_f16w (7e-4 / 7e-3,
tangent away from the kink): no tolerance of this module's own.  Only a tangent that misses the plain check is looked at
again (at_the_kink below): voxels whose branch differs from the oracle's, all of them within kink.FLIP_TOL RMS of zero and at
most kink's 1e-3 of the tensor, take the kernel's branch, and the plain check is repeated.  Each test asserts the profile entry
run_conv records against the restated selection, so that a case which falls to another kernel fails instead of passing on
that kernel's merits.

Position independence.  Every kernel gives an output a K sum of fixed order, so its bits must not depend on where its tile
begins, on the branch of the tile order its plane pair is decoded in, or on its cout tile's neighbour (numbers in each
test's docstring).

The masked halo.  The layer hook zeroes its workspace, so there a masked lane's value leaking into a stored output would add
zero; the block hook keeps its context's workspace, which a NaN run fills with NaN wherever a tensor lay."""

import numpy as np
import pytest

import patch_cases as P
import test_gpu_blocks as TB
from conftest import rel_l2, max_over_rms
from kink import FLIP_TOL
from layer_checks import (RTOL_L2, RTOL_MAX, RTOL_L2_F16, RTOL_MAX_F16, RTOL_L2_F16W, RTOL_MAX_F16W, _chk, _chk_f16w, _h)
from oracle import layers as L
from test_gpu_stream_layers import profiled, _sub

pytestmark = pytest.mark.gpu

WORST = {}                                     # (kernel, arithmetic, class) -> [rel-L2, max/RMS]
BOUNDS = {"f32": (RTOL_L2, RTOL_MAX), "f16": (RTOL_L2_F16, RTOL_MAX_F16), "f16w": (RTOL_L2_F16W, RTOL_MAX_F16W)}


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
    """a loaded network of width mid: the blocks' own launches (nbe_test_block), a fresh context per call"""
    def get(prec, mid, vel):
        e = engine_factory(mid_chan=mid, precision=prec, compute_vel=vel)
        e.load_params(TB.params_of(mid), False)
        e.set_cosmology(TB.OM, TB.DZ)
        return e
    return get


def set_wino(monkeypatch, on):
    if on:
        monkeypatch.delenv("NBE_WINO", raising=False)
    else:
        monkeypatch.setenv("NBE_WINO", "0")


def launch(e, form, o, x, dx, act, res=False):
    """(y, dy or None) of one launch form on operands o with the input (x, dx)"""
    r, dr = (o.r, o.dr) if res else (None, None)
    if form.tangent == "gauged":
        return e.test_layer_gauged(x, dx, o.w, o.beta, o.b, act=act, res=r, dres=dr)
    if form.tangent == "vel":
        return e.test_layer("conv3", x, o.w, o.b, dx=dx, dw=o.dw, act=act, res=r, dres=dr)
    return e.test_layer("conv3", x, o.w, o.b, act=act, res=r), None


# ---- parity ----------------------------------------------------------------------------------------------------------------------
PARITY = [(c, f) for c in P.CASES for f in P.forms(c)]


class Reference:
    """operands and float64 oracle of the current case; the products are computed once per operand rounding and left unchanged"""
    def __init__(self, case):
        self.case, self.ops, self.memo = case, P.operands(case), {}

    def product(self, half, a, wt):
        key = (half, a, wt)
        if key not in self.memo:
            f = lambda t: _h(t, half).astype(np.float64)
            y = L.conv_layer("conv3", f(getattr(self.ops, a)), f(getattr(self.ops, wt)), np.zeros(self.case.cout))
            y.setflags(write=False)
            self.memo[key] = y
        return self.memo[key]

    def oracle(self, half, tangent):
        """(y, dy, y before the activation, dy before it); dy None for displacement only"""
        o, c = self.ops, self.case
        col = lambda v: v.astype(np.float64)[:, None, None, None]
        wx = self.product(half, "x", "w")
        y, dy = wx + col(o.b), None
        if tangent == "gauged":
            dy = self.product(half, "dx", "w") + col(o.beta) * wx
        elif tangent == "vel":
            dy = self.product(half, "dx", "w") + self.product(half, "x", "dw")
        if c.res:
            y = y + _h(o.r, half)
            dy = None if dy is None else dy + _h(o.dr, half)
        if not c.act:
            return y, dy, None, None
        if dy is None:
            return L.leaky_relu(y), None, y, None
        return L.leaky_relu_vel(y, dy) + (y, dy)


_REF = []


def reference(case):
    if not _REF or _REF[0].case.name != case.name:
        _REF[:] = [Reference(case)]
    return _REF[0]


def _record(kern, prec, cls, e2, em):
    w = WORST.setdefault((kern, prec, cls), [0.0, 0.0])
    w[0], w[1] = max(w[0], e2), max(w[1], em)


def _note(kern, prec, cls, got, want, what, record=True):
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    print("  %-44s rel-L2 %.2e  max/RMS %.2e" % (what, e2, em))
    if record:
        _record(kern, prec, cls, e2, em)


MAX_FLIP_FRAC = 1e-3                           # the default max_flip_frac of kink.assert_cone


def at_the_kink(y, y_pre, dy_pre, what):
    """The tangent of LeakyReLU jumps by a factor of 100 where the value changes sign, so two evaluations differ wherever a
    pre-activation is zero to within their rounding (tests/kink.py; c128-128 on conv_h3w has one such voxel among 152064: the
    oracle's pre-activation is 7.4e-7, the kernel's -6e-9, the rest of the tangent within 7.2e-6 RMS).  For a tangent that
    missed the plain check: the voxels where the kernel's value shows another branch than the oracle's must all lie within
    kink.FLIP_TOL RMS of zero and be at most MAX_FLIP_FRAC of the tensor; the oracle's tangent with the kernel's branch on
    those voxels is returned for a second plain check.  A flip anywhere else, or a tangent wrong on its own branch, fails."""
    flips = (y > 0) != (y_pre > 0)
    near = np.abs(y_pre) <= FLIP_TOL * float(np.sqrt(np.mean(y_pre ** 2)))
    print("  %-44s %d of %d branches differ from the oracle's, %d of them within %.0e RMS of the kink" % (
        what, int(flips.sum()), flips.size, int((flips & near).sum()), FLIP_TOL))
    assert flips.any(), "%s: the tangent misses its class and no branch differs from the oracle's" % what
    assert not (flips & ~near).any(), "%s: a branch flipped at |pre-activation| = %.2e RMS" % (
        what, float(np.abs(y_pre[flips]).max() / np.sqrt(np.mean(y_pre ** 2))))
    assert flips.sum() <= MAX_FLIP_FRAC * flips.size, "%s: %d of %d branches flipped" % (what, int(flips.sum()), flips.size)
    return L.leaky_relu_vel(y_pre, dy_pre, branch=y > 0)[1]


@pytest.mark.parametrize("case,form", PARITY, ids=["%s-%s" % (c.name, P.form_id(f)) for c, f in PARITY])
def test_against_oracle(engines, case, form, monkeypatch):
    e = engines(form.prec)
    half = form.prec == "f16"
    ref = reference(case)
    o = ref.ops
    y_o, dy_o, y_pre, dy_pre = ref.oracle(half, form.tangent)
    kernel, label = P.select(form, case.cin, case.dv, case.res)
    set_wino(monkeypatch, form.wino)
    (y, dy), ran = profiled(e, lambda: launch(e, form, o, o.x, o.dx, case.act, case.res))
    assert ran and all(k.startswith(label) for k in ran), (kernel, label, ran)
    assert (dy is None) == (dy_o is None)
    what = "%s %s" % (case.name, P.form_id(form))
    if kernel == "h3w_f16":
        _note(kernel, form.prec, "f16w", y, y_o, what + " value")
        _note(kernel, form.prec, "f16w", dy, dy_o, what + " tangent (kink voxels included)", record=False)
        _chk_f16w(y, y_o, what + " value")
        _record(kernel, form.prec, "f16w", *_chk_f16w(dy, dy_o, what + " tangent", *((y_pre, dy_pre) if case.act else ())))
        return
    cls = "f16" if half else "f32"
    _note(kernel, form.prec, cls, y, y_o, what + " value")
    _chk(y, y_o, what + " value", half)
    if dy is not None:
        t2, tm = BOUNDS[cls]
        if case.act and not (rel_l2(dy, dy_o) <= t2 and max_over_rms(dy, dy_o) <= tm):
            _note(kernel, form.prec, cls, dy, dy_o, what + " tangent, the oracle's branches", record=False)
            dy_o = at_the_kink(y, y_pre, dy_pre, what)
        _note(kernel, form.prec, cls, dy, dy_o, what + " tangent")
        _chk(dy, dy_o, what + " tangent", half)


# ---- position independence ----------------------------------------------------------------------------------------------------------
def _same_bits(e, form, kernel, dims, offsets, seed):
    """the full volume, then the sub-volumes from `offsets`: the same bits on the common voxels, from `kernel` each time"""
    o = P.make_operands(64, 64, dims, seed)
    label = P.select(form, 64, tuple(n - 2 for n in dims))[1]
    run = lambda x, dx: launch(e, form, o, x, dx, True)
    (y, dy), ran = profiled(e, lambda: run(o.x, o.dx))
    assert ran and all(k.startswith(label) for k in ran), (label, ran)
    outs = [("y", y)] + ([] if dy is None else [("dy", dy)])
    for _, a in outs:
        assert np.all(np.isfinite(a)) and np.abs(a).max() > 0
    for off in offsets:
        sub_dv = tuple(n - 2 - d for n, d in zip(dims, off))
        assert P.select(form, 64, sub_dv)[0] == kernel
        (ys, dys), ran = profiled(e, lambda: run(_sub(o.x, off), _sub(o.dx, off)))
        assert ran and all(k.startswith(label) for k in ran), (label, ran)
        for (name, full), got in zip(outs, (ys, dys)):
            want = full[:, off[0]:, off[1]:, off[2]:]
            assert got.shape == want.shape == (64,) + sub_dv, (name, off, got.shape, want.shape)
            assert np.array_equal(got, want), "%s depends on where the volume begins (offset %s): %d of %d voxels differ" % (
                name, off, int((got != want).sum()), got.size)


DIRECT = [("h3q", P.Form("f16x3", "vel", True)), ("h3g_wide", P.Form("f16x3", "gauged", False)),
          ("h2q_split", P.Form("f16x3", "novel", False)), ("h2q_f16", P.Form("f16", "vel", True)),
          ("h2q_f16_g", P.Form("f16", "gauged", False)), ("h3p", P.Form("f16", "novel", True))]


@pytest.mark.parametrize("kernel,form", DIRECT, ids=[k for k, _ in DIRECT])
def test_direct_kernels_are_position_independent(engines, kernel, form, monkeypatch):
    """64 -> 64 on a (8, 22, 72) input: 6 x 20 x 70 outputs; from (1, 3, 5) 5 x 17 x 65, from (3, 3, 5) 3 x 17 x 65.  On the
    8-row tiles all three have 3 x 3 tiles per plane (2 x 3 on the 16-row tiles of conv_h2q), and the offsets (3, 5) move every
    voxel to another row and column of its tile: rows 8 .. 10 of tile row 1 become rows 5 .. 7 of tile row 0, columns 64 .. 68
    of tile column 2 become columns 59 .. 63 of tile column 1.  A plane is a workgroup of its own: the z offsets 1 and 3 change
    every tile's number, and with it its workgroup and XCD."""
    dims, offsets = (8, 22, 72), ((1, 3, 5), (3, 3, 5))
    dvs = [(6, 20, 70), (5, 17, 65), (3, 17, 65)]
    rows = P.KERNELS[kernel].rows
    assert [P.tiling(kernel, dv, 64)[1:4] for dv in dvs] == [(-(-dv[1] // rows), 3, dv[0] * -(-dv[1] // rows) * 3) for dv in dvs]
    assert rows == 16 or [P.tiling(kernel, dv, 64).tny for dv in dvs] == [3, 3, 3]
    assert P.select(form, 64, dvs[0])[0] == kernel
    set_wino(monkeypatch, form.wino)
    _same_bits(engines(form.prec), form, kernel, dims, offsets, 31)


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
def test_winograd_z_is_position_independent(engines, prec, monkeypatch):
    """conv_h3w_kernel with a tangent (f16x3) and its float16 form pair planes from the first one, so the z offsets are even.
    64 -> 64 on a (22, 14, 40) input: 20 x 12 x 38 outputs, ten plane pairs = one block of eight and rem 2; from (2, 3, 5)
    18 x 9 x 33, nine pairs = one block and rem 1; from (4, 3, 5) 16 x 9 x 33, eight pairs = one whole block.  Output planes
    18 and 19 are pair 9 of the volume (remainder branch, rem 2), pair 8 from the first offset (remainder branch, rem 1) and
    pair 7 from the second (inside the block); planes 4 .. 17 stay in the block but change their place in it.  Tiles: 2 x 2
    per pair each time, rows and columns move by (3, 5) within them."""
    dvs = [(20, 12, 38), (18, 9, 33), (16, 9, 33)]
    kernel = "h3w_f16x3" if prec == "f16x3" else "h3w_f16"
    form = P.Form(prec, "gauged", True)
    tl = [P.tiling(kernel, dv, 64) for dv in dvs]
    assert [(t.tny, t.tnx, t.ntiles, t.remainder) for t in tl] == [(2, 2, 40, 8), (2, 2, 36, 4), (2, 2, 32, 0)]
    assert [dv[0] // 2 % P.zblock(dv[0]) for dv in dvs] == [2, 1, 0]
    last = [P.decode_pairs(t.ntiles - 1, dv[0], t.tny, t.tnx) for t, dv in zip(tl, dvs)]
    assert last == [(9, 1, 1, True), (8, 1, 1, True), (7, 1, 1, False)]
    assert P.select(form, 64, dvs[0])[0] == kernel
    set_wino(monkeypatch, True)
    _same_bits(engines(prec), form, kernel, (22, 14, 40), ((2, 3, 5), (4, 3, 5)), 32)


def test_winograd_z_displacement_only_is_position_independent(engines, monkeypatch):
    """conv_h3w_kernel<., NOVEL> owns two blocks of eight rows per tile whose accumulator sets sum their products in different
    orders (tests/test_gpu_wino_skip_phase.py): a row keeps its bits only if it keeps its block, so the y offset is 16.
    64 -> 64 on a (22, 38, 40) input: 20 x 36 x 38 outputs, 3 x 2 tiles of 16 rows per pair, ten pairs (rem 2, 60 tiles, 12 in
    the remainder branch); from (2, 16, 5) 18 x 20 x 33: 2 x 2 tiles, nine pairs (rem 1, 36 tiles, 4); from (4, 16, 5)
    16 x 20 x 33: eight pairs, one whole block (32 tiles).  Rows 16 .. 35 become rows 0 .. 19: the third tile row's four rows
    (first block, the second wholly masked) become the second's first block of four, its second block wholly masked."""
    dvs = [(20, 36, 38), (18, 20, 33), (16, 20, 33)]
    form = P.Form("f16x3", "novel", True)
    tl = [P.tiling("h3w_novel", dv, 64) for dv in dvs]
    assert [(t.tny, t.tnx, t.ntiles, t.remainder) for t in tl] == [(3, 2, 60, 12), (2, 2, 36, 4), (2, 2, 32, 0)]
    assert [P.second_block_rows(16 * ty, 36) for ty in range(3)] == [8, 8, 0]
    assert [P.second_block_rows(16 * ty, 20) for ty in range(2)] == [8, 0]
    assert P.select(form, 64, dvs[0])[0] == "h3w_novel"
    set_wino(monkeypatch, True)
    _same_bits(engines("f16x3"), form, "h3w_novel", (22, 38, 40), ((2, 16, 5), (4, 16, 5)), 33)


# ---- the masked halo of a ragged patch ----------------------------------------------------------------------------------------------------------
HALO = [("f16x3", True, True, "conv_h3w<FLAT3,vel,dx>"), ("f16x3", True, False, "conv_h3g<FLAT3,vel,dx>"),
        ("f16x3", False, True, "conv_h3w<FLAT3,novel>"), ("f16", True, True, "conv_h1w<FLAT3,vel,dx>")]


@pytest.mark.parametrize("prec,vel,wino,label", HALO, ids=["f16x3", "f16x3-direct", "f16x3-novel", "f16"])
def test_masked_halo_neither_leaks_into_nor_past_the_result(loaded, prec, vel, wino, label, monkeypatch):
    """conv_l01 at mid 24 on a (8, 21, 45) input: the block runs fused, so its hidden tensor (6 x 19 x 43) lies on the input's
    pitch 21 x 45 and the result has four planes of 17 x 41 -- 3 x 2 tiles of 8 x 32 (2 x 2 of 16 x 32) with one row and nine
    columns in the last ones.  Every patch kernel fetches the whole 10 x 34 (18 x 34) patch of a tile whatever Hv and Wv are and
    masks in the epilogue: the rows and columns beyond (Hv + 2, Wv + 2) are the pitch's padding, the next plane, or what lies
    behind the tensor.  A NaN input of the same shape leaves NaN wherever the context's workspace was written (NaN in, NaN out:
    no error); the finite case on that workspace must then give the bits of a context that never saw the NaN."""
    set_wino(monkeypatch, wino)
    mid, shape = 24, (8, 21, 45)
    rows = 16 if not vel else 8
    assert (P.tiles_of(17, rows), P.tiles_of(41, P.HP_COLS), 17 % 8, 41 % P.HP_COLS) == (3 if vel else 2, 2, 1, 9)
    rng = np.random.default_rng(41)
    x = P.rand(rng, mid, *shape)
    dx = P.rand(rng, mid, *shape) if vel else None
    want = loaded(prec, mid, vel).test_block('conv_l01', x, dx=dx)
    e = loaded(prec, mid, vel)
    nan = np.full_like(x, np.nan)
    out = e.test_block('conv_l01', nan, dx=nan if vel else None)
    assert out["y"].shape == (mid, 4, 17, 41) and np.isnan(out["y"]).all() and (not vel or np.isnan(out["dy"]).all())
    got, ran = profiled(e, lambda: e.test_block('conv_l01', x, dx=dx))
    assert ran == [label], ran
    assert "skip_fused" in got["paths"] and got["paths"] == want["paths"], (got["paths"], want["paths"])
    for k in ("y", "dy", "h", "dh") if vel else ("y", "h"):
        assert np.all(np.isfinite(want[k])) and np.abs(want[k]).max() > 0
        assert np.array_equal(got[k], want[k]), "%s differs after a NaN run on the same workspace" % k


def test_zz_worst_cases():
    """prints the worst figure per kernel and arithmetic of this run against the class it is held to"""
    print("\n  kernel | arithmetic | worst rel-L2 (bound) | worst max/RMS (bound)")
    for (kern, prec, cls), (e2, em) in sorted(WORST.items()):
        t2, tm = BOUNDS[cls]
        print("  %-10s | %-5s | %.2e (%.0e) | %.2e (%.0e)" % (kern, prec, e2, t2, em, tm))
