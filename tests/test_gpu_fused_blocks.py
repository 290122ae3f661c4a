"""The fused conv_1 + skip launches of a residual block -- conv_h3w_kernel<SKIP> in its three forms and conv_h3g_kernel with
nskip > 0, on one input tensor and on two -- at the edges of their own tiling, through the block hook (nbe_test_block), which
is the one way to build them: against the float64 oracle, for position independence bit by bit, and for what the masked part
of a ragged tile leaves alone.  The cases, the launch forms (w, g, n, h) and the kernel selection they rest on are in
tests/fused_cases.py; tests/test_fused_cases.py holds that table to its edges on the CPU.

Parity.  Every (case, form) runs through test_gpu_blocks.run_case with all of its checks: both stages against the oracle of
tests/block_ref.py at the per-layer classes of tests/layer_checks.py, the branches behind the activations, the gauge vectors,
the path bits, and for conv_r00 the two-source form against the concat form (bit for bit under NBE_WINO=0).  No tolerance
of this module's own.  On top of that each test asserts the profile entries run_conv records -- label and launch count of
conv_0 and of conv_1 as fused_cases.launches() restates the selection -- and the exact path word, so that a case which falls
to another kernel fails instead of passing on that kernel's merits.

Position independence.  A kernel gives an output a K sum of fixed order, so its bits must not depend on the tile, the branch
of the tile decode or the block of plane pairs it is computed in.  The method is test_gpu_wino_skip_phase.py's: the block
input embedded in a larger tensor whose surroundings repeat its own values (the same max |x|, hence the same range shift).

The masked halo.  test_gpu_patch_layers.py's method: a NaN run fills a fresh context's workspace with NaN wherever a tensor
lay; the finite case on that context must then give the bits of a context that never saw the NaN."""

import time

import numpy as np
import pytest

import block_ref as B
import fused_cases as F
import test_gpu_blocks as TB
from test_gpu_blocks import engines  # noqa: F401  (the module-scoped engine cache, as a fixture of this module)
from test_gpu_patch_layers import loaded, set_wino  # noqa: F401  (loaded: a fresh loaded context per call, as a fixture)
from oracle import layers as L
from stream_cases import rand

pytestmark = pytest.mark.gpu

# run_case files its figures in the table of the tree it is given: one table per launch form, same parameters as "style"
for _f in F.ALL:
    TB.TREES["fused-" + _f] = TB.Tree(lambda mid, vel: TB.params_of(mid), TB.expect_fused, TB.GAUGE_DEV)
T0 = [None]


def counted(e, run):
    """(run(), {profile label: launches}) of the convolution launches of run()"""
    if T0[0] is None:
        T0[0] = time.time()
    e.profile_reset()
    e.profile_enable(True)
    try:
        out = run()
        prof = e.profile_read()
    finally:
        e.profile_enable(False)
    return out, {p["kernel"]: p["launches"] for p in prof if p["launches"] > 0}


# ---- parity ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case,form", F.PARITY, ids=["%s-%s" % (c.name, f) for c, f in F.PARITY])
def test_against_the_oracle(engines, case, form, monkeypatch):  # noqa: F811
    f = F.FORMS[form]
    wino_on = F.wino_env(case, form)
    set_wino(monkeypatch, wino_on)
    e = engines(case.mid, f.prec, f.vel)
    srcs = F.sources(case, form)
    print("  %s [%s]: %s" % (case.name, form, case.why))
    with L.backend('torch'):
        out, ran = counted(e, lambda: TB.run_case(e, case.block, case.mid, f.prec, f.vel, F.shape(case), wino_on=wino_on,
                                                  forms=srcs, tree="fused-" + form))
    assert set(out) == set(srcs), (sorted(out), srcs)
    assert ran == F.labels(case, form), (ran, F.labels(case, form))
    for src, r in out.items():
        assert r["paths"] == F.paths(case, form, src), (src, r["paths"], F.paths(case, form, src))
        assert r["y"].shape == (B.channels(case.block, case.mid)[2],) + case.dv


# ---- position independence ----------------------------------------------------------------------------------------------------------
def _embed(a, lead, trail):
    """a inside a larger tensor whose surroundings repeat a's own values (the same max |x|: the same range shift)"""
    return None if a is None else np.ascontiguousarray(np.pad(a, ((0, 0),) + tuple(zip(lead, trail)), mode='wrap'))


BASE = (18, 9, 33)                             # result extents of the embedded case: nine plane pairs, 2 x 2 tiles (1 x 2 of 16 rows)
#       id        block       mid  form  two    lead          trail
POS = [("z2", 'conv_l01', 64, f, False, (2, 0, 0), (2, 0, 0)) for f in "wnh"] + \
      [("z16", 'conv_l01', 64, f, False, (16, 0, 0), (0, 0, 0)) for f in "wnh"] + \
      [("yx", 'conv_l01', 64, f, False, (0, 16 if f == "n" else 7, 31), (0, 1, 1)) for f in "wnh"] + \
      [("two", 'conv_r00', 64, f, True, (2, 16 if f == "n" else 7, 31), (2, 1, 1)) for f in "wn"] + \
      [("z1", 'conv_l01', 64, "g", False, (1, 7, 31), (0, 1, 1)), ("two", 'conv_r00', 16, "g", True, (3, 7, 31), (0, 1, 1))]


@pytest.mark.parametrize("name,block,mid,form,two,lead,trail", POS, ids=["%s-%s-%s" % (p[0], p[1], p[3]) for p in POS])
def test_position_independence(engines, name, block, mid, form, two, lead, trail, monkeypatch):  # noqa: F811
    """The result of 18 planes x 9 x 33 (input 22 x 13 x 37) and the same input inside a larger one, bit for bit on the common
    voxels of the hidden tensor and of the result, in conv_0 (two planes, rows and columns more) as in conv_1:
      z2   lead and trail of 2 planes: 9 plane pairs (one block of 8 and remainder 1) become 11 (remainder 3); pair p becomes
           pair p + 1, so pair 7 leaves the block for the first place of the remainder branch and pair 8, the single
           remainder pair, becomes the second of three; conv_0: 10 pairs (remainder 2) become 12 (remainder 4);
      z16  lead of 16 planes: 17 pairs, two whole blocks and remainder 1; pairs 0 .. 7 move from block 0 to block 1 and pair
           8 stays the remainder pair behind another block; conv_0: 18 pairs, remainder 2 behind two blocks;
      yx   lead of 7 rows and 31 columns (trail 1, 1): result 17 x 65, 3 x 3 tiles; every voxel changes its row and column
           within its tile, and rows 1 .. 8 and columns 1 .. 32 cross a tile boundary.  The displacement-only form sums its
           two row blocks in different orders (tests/test_gpu_wino_skip_phase.py), so a row keeps its bits only in its own
           block: there the lead is 16 rows (result 26 x 65, 2 x 3 tiles of 16 rows);
      two  conv_r00 from two source tensors, both embedded alike: z2 and yx at once;
      z1   the direct kernel (NBE_WINO=0) decodes planes, not pairs: an odd lead, which moves every tile to another workgroup."""
    f = F.FORMS[form]
    case = F.Case(name, block, mid, BASE, 0, form, "")
    big = case._replace(dv=tuple(n + a + b for n, a, b in zip(BASE, lead, trail)))
    wino_on = F.wino_env(case, form) and F.wino_env(big, form)
    assert wino_on == f.wino                                     # the g cases run under NBE_WINO=0 whatever the plane count
    set_wino(monkeypatch, wino_on)
    src = "two" if two else "cat"
    if form != "g":
        assert lead[0] % 2 == 0 and F.launches(big, form, src)[1].kernel == F.launches(case, form, src)[1].kernel
        t = F.launch_tiling(F.launches(big, form, src)[1])
        npair = big.dv[0] // 2
        moved = [F.decode_pairs(i, big.dv[0], t.tny, t.tnx) for i in range(t.ntiles)]
        if name == "z2":
            assert npair == 11 and sorted({p[0] for p in moved if p[3]}) == [8, 9, 10]
        if name == "z16":
            assert npair == 17 and sorted({p[0] for p in moved if p[3]}) == [16] and t.ntiles - t.remainder == 2 * 8 * t.tny * t.tnx
        if name == "yx":
            assert (t.tny, t.tnx) == ((2, 3) if form == "n" else (3, 3))
    e = engines(mid, f.prec, f.vel)
    D, H, W, _ = F.shape(case)
    g_in = B.gauges(TB.params_of(mid), TB.s64(), block, mid)[0]
    x, dxs = TB.make_input(block, mid, f.prec, f.vel, (D, H, W, 0), g_in)
    X, DXS = _embed(x, lead, trail), _embed(dxs, lead, trail)
    assert np.abs(X).max() == np.abs(x).max() and X.shape[1:] == F.shape(big)[:3]

    def run(a, da):
        if two:
            return e.test_block(block, a[:mid], dx=None if da is None else da[:mid], x2=a[mid:], dx2=None if da is None else da[mid:],
                                two_source=True)
        return e.test_block(block, a, dx=da)
    label = F.launches(case, form, src)[1].label
    small, ran = counted(e, lambda: run(x, dxs))
    assert ran == {label: 2}, ran
    large, ran = counted(e, lambda: run(X, DXS))
    assert ran == {label: 2}, ran
    assert small["paths"] == large["paths"] == F.paths(case, form, src), (small["paths"], large["paths"])
    dz, dy, dx = lead
    for k, crop in (("h", 1), ("dh", 1), ("y", 2), ("dy", 2)):    # the hidden tensor shrinks by 1 per side, the result by 2
        if small[k] is None:
            continue
        n = small[k].shape
        common = large[k][:, dz:dz + n[1], dy:dy + n[2], dx:dx + n[3]]
        assert common.shape == n and n[1:] == (D - 2 * crop, H - 2 * crop, W - 2 * crop)
        assert np.all(np.isfinite(small[k])) and np.abs(small[k]).max() > 0
        assert np.array_equal(common, small[k]), "%s %s: %d of %d values differ after the shift by %s" % (
            block, k, int((common != small[k]).sum()), common.size, lead)


# ---- the masked rows and columns of the last tiles ----------------------------------------------------------------------------------------------------------
HALO = [('conv_r00', (4, 9, 33), True), ('conv_l01', (4, 7, 31), False)]


@pytest.mark.parametrize("form", list(F.ALL))
@pytest.mark.parametrize("block,dv,two", HALO, ids=["r00-two-9x33", "l01-7x31"])
def test_masked_rows_and_columns_neither_leak_into_nor_past_the_result(loaded, block, dv, two, form, monkeypatch):  # noqa: F811
    """Mid 64.  conv_r00 from two source tensors at a result of 4 x 9 x 33: 2 x 2 tiles whose last ones hold one row, one column
    (the 16-row tiles: one row in the second row block); conv_l01 at 4 x 7 x 31: one tile, one row and one column short.  Every
    form fetches whole patches whatever Hv and Wv are -- the main input's through LDS, the skip's centre voxels (sk_load; the
    direct kernel's skip patches) straight from the block input -- and masks in the epilogue: what lies beyond is the input's
    pitch, the next plane, or whatever the workspace held.  After a NaN run of the same shape the workspace holds NaN wherever a
    tensor lay; the finite case on it must give the bits of a context that never saw the NaN."""
    f = F.FORMS[form]
    case = F.Case("halo", block, 64, dv, 0, form, "")
    set_wino(monkeypatch, f.wino)
    src = "two" if two else "cat"
    assert F.sources(case, form)[-1] == src
    c1 = F.launches(case, form, src)[1]
    t = F.launch_tiling(c1)
    assert (t.tny, t.tnx) == ((1, 2) if (two and form == "n") else (2, 2) if two else (1, 1))
    mid, (D, H, W, _) = 64, F.shape(case)
    rng = np.random.default_rng(43)
    cin = B.channels(block, mid)[0]
    x = rand(rng, cin, D, H, W)
    dx = rand(rng, cin, D, H, W) if f.vel else None

    def run(e, a, da):
        if two:
            return e.test_block(block, a[:mid], dx=None if da is None else da[:mid], x2=a[mid:], dx2=None if da is None else da[mid:],
                                two_source=True)
        return e.test_block(block, a, dx=da)
    want = run(loaded(f.prec, mid, f.vel), x, dx)
    e = loaded(f.prec, mid, f.vel)
    nan = np.full_like(x, np.nan)
    out = run(e, nan, nan if f.vel else None)
    assert out["y"].shape == (mid,) + dv and np.isnan(out["y"]).all() and (not f.vel or np.isnan(out["dy"]).all())
    got, ran = counted(e, lambda: run(e, x, dx))
    assert ran == {c1.label: 2}, ran
    assert got["paths"] == want["paths"] == F.paths(case, form, src), (got["paths"], want["paths"])
    for k in ("y", "dy", "h", "dh") if f.vel else ("y", "h"):
        assert np.all(np.isfinite(want[k])) and np.abs(want[k]).max() > 0
        assert np.array_equal(got[k], want[k]), "%s differs after a NaN run on the same workspace" % k


def test_zz_worst_cases():
    """prints the worst figure per stage, launch form and tolerance class of this run (DESIGN.md section 2c records them)"""
    print("\n  stage | form | arithmetic | class | worst rel-L2 (bound) | worst max/RMS (bound)")
    for f in F.ALL:
        for (stage, arith, cls), (e2, em) in sorted(TB.TREES["fused-" + f].worst.items()):
            print("  %-22s | %s | %-10s | %-4s | %.2e (%.0e) | %.2e (%.0e)" % (stage, f, arith, cls, e2, TB.TOL[cls][0], em, TB.TOL[cls][1]))
    if T0[0] is not None:
        print("  wall time of this module so far: %.0f s" % (time.time() - T0[0]))
