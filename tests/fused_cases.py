"""Case table of tests/test_gpu_fused_blocks.py: a residual block's two launches through the block hook (nbe_test_block), with
the 1x1x1 skip fused into conv_1, at the edges of the tiling of the kernels that run them.  The tiling itself is the
restatement of tests/patch_cases.py (tiles_of, patch_tiles, decode_pairs, decode_z, zblock, nct, nchunk, second_block_rows,
xcd_tile); what is restated here is the geometry of a block, which kernel each of its launches gets, and what the hook reports.

Geometry (resblock / resblock_part, nbe_engine_net.cpp:183-245; alloc_hidden :169-173).  For a block input (D, H, W, pad) with
sy = 0 if pad else 2 (pad = 1: periodic in y and x, a halo of one voxel is filled around every tensor):
  * conv_0 is a launch over D - 2 planes of (H - sy, W - sy) (:204: Hv = x.p.H - 2 with the halo in x.p.H), written into the
    hidden tensor, which in a fused block has the input's row and plane pitch (:171);
  * conv_1 + skip is a launch over D - 4 planes of (H - 2 sy, W - 2 sy) (:213); it reads the hidden tensor and, at the centre
    voxel of its 3x3x3 stencil two planes, rows and columns into the block input (sk_off, :193), the block input itself.
A Case below is named by its RESULT extents (Dv, Hv, Wv): shape() gives the input.

Which kernel (conv_select / h3w_ok, nbe_conv_select.h:97-162; run_conv, nbe_engine_net.cpp:87-100; block_fused :159):
  * conv_l00/conv_0 has no input tangent and runs on the stem kernel in every half-precision form (:124);
  * f16x3 with velocity: gauged, so conv_h3w<SKIP, false> where the launch's plane count is even (h3w_pairs_planes), NBE_WINO
    is not 0 and 4 nchunk <= 32 stages, 2 nskip <= 16 skip entries; otherwise conv_h3g<false> (h3g_wide), which runs the
    fused skip itself (nskip > 0): the block is fused either way;
  * f16x3 displacement only: conv_h3w<SKIP, true> under the same conditions, and only there is the block fused;
  * float16 with velocity: conv_h3w<SKIP, false, true> under the same conditions on 32-channel stages -- an even chunk count
    of conv_0, of conv_1 and of the skip, sources switching between whole stages, a skip input with a tangent (not conv_l00);
  * nskip = pad16(cin) / 16 chunks (launch_conv, nbe_kernels.hip:278), half as many stages in the float16 form
    (launch_h3w, nbe_kernels_wino.h:897); the two-source form switches sources at csplit = s_csplit = mid / 16 (:269, :277).
conv_0 and conv_1 of a block run the same kernel family and so share a profile label (conv_label, :166-188) except in
conv_l00; launches() gives (layer, kernel, label, extents, ...) per launch, paths() the exact word of the hook.

Launch forms of a case
  w  f16x3, velocity                      conv_h3w<SKIP> (even planes)
  g  the same operands under NBE_WINO=0, or unchanged where the plane count is odd: conv_h3g wide with the fused skip
  n  f16x3, displacement only             conv_h3w<SKIP, NOVEL>: 16-row tiles, two row blocks per workgroup
  h  float16, velocity                    conv_h3w<SKIP, false, F16>
and on conv_r00 each of them on the concat tensor and on two source tensors (one run_case call runs both)."""

import collections

import block_ref as B
from patch_cases import (tiles_of, patch_tiles, decode_pairs, decode_z, zblock, nct, nchunk, second_block_rows, tiling, walk,  # noqa: F401
                         HP_ROWS, HP_COLS, MAX_WSTAGES, F16_CHUNKS)
from stream_cases import xcd_tile  # noqa: F401
from test_gpu_blocks import expect_fused  # noqa: F401  (the module imports without a GPU)

MAX_WSKIP = 16                                 # NBE_MAX_WSKIP, nbe_conv_select.h:25

Form = collections.namedtuple("Form", "prec vel wino")
FORMS = {"w": Form("f16x3", True, True), "g": Form("f16x3", True, False), "n": Form("f16x3", False, True),
         "h": Form("f16", True, True)}

# forms: the letters of the launch forms the case runs on; every case runs w or g
Case = collections.namedtuple("Case", "name block mid dv pad forms why")


def _c(name, dv, forms, why, block="conv_l01", mid=64, pad=0):
    return Case(name, block, mid, dv, pad, forms, why)


def shape(case):
    """(D, H, W, pad) of the block input"""
    sy = 0 if case.pad else 2
    return (case.dv[0] + 4, case.dv[1] + 2 * sy, case.dv[2] + 2 * sy, case.pad)


def wino_env(case, form):
    """is NBE_WINO left alone?  The g form of an odd plane count needs no switch: no launch of it has a Winograd-z form"""
    return FORMS[form].wino or case.dv[0] % 2 == 1


def sources(case, form):
    """the forms of the block input run_case runs: the decoder blocks also from two tensors where whole chunks (stages) allow"""
    f = FORMS[form]
    two = case.block in B.DECODERS and case.mid % (32 if f.prec == "f16" else 16) == 0 and fused(case, form)
    return ("cat", "two") if two else ("cat",)


# ---- which kernel runs ---------------------------------------------------------------------------------------------------------
def _h3w(prec, nplanes, wino, chunks, split=None):
    """h3w_ok for a launch of the block hook: chunks = the chunk counts that must be whole stages (conv's, the skip's)"""
    per = F16_CHUNKS if prec == "f16" else 1
    if not wino or nplanes % 2:
        return False
    if any(n % per for n in chunks) or (split is not None and split % per):
        return False
    return 4 * (chunks[0] // per) <= MAX_WSTAGES and all(2 * (n // per) <= MAX_WSKIP for n in chunks[1:])


def fused(case, form):
    """block_fused (nbe_engine_net.cpp:159) with what makes L1->fskip exist per arithmetic (pack_wino, wino_f16_layer)"""
    f = FORMS[form]
    cin, cmid, _ = B.channels(case.block, case.mid)
    if f.prec == "f16x3" and f.vel:
        return True
    inside = wino_env(case, form) and f.wino and case.dv[0] % 2 == 0
    if not f.vel:
        return inside
    return inside and case.block != "conv_l00" and nchunk(cmid) % 2 == 0 and nchunk(cin) % 2 == 0


Launch = collections.namedtuple("Launch", "layer kernel label dv cin cout nskip split")

_LABEL = {"h3w_f16x3": "conv_h3w<FLAT3,vel,dx>", "h3g_wide": "conv_h3g<FLAT3,vel,dx>", "h3w_novel": "conv_h3w<FLAT3,novel>",
          "h3w_f16": "conv_h1w<FLAT3,vel,dx>"}


def launches(case, form, src="cat"):
    """[conv_0, conv_1] of a fused case: nskip and split (where the sources switch; None on the concat tensor) in the units
    of the kernel, 16-channel chunks or 32-channel stages"""
    f = FORMS[form]
    assert fused(case, form), (case.name, form)
    cin, cmid, cout = B.channels(case.block, case.mid)
    D, H, W, pad = shape(case)
    sy = 0 if pad else 2
    wino = f.wino and wino_env(case, form)
    split = case.mid // 16 if src == "two" else None
    per = F16_CHUNKS if f.prec == "f16" else 1
    wk = "h3w_f16x3" if f.vel and f.prec == "f16x3" else "h3w_novel" if not f.vel else "h3w_f16"
    out = []
    dv0, dv1 = (D - 2, H - sy, W - sy), case.dv
    if case.block == "conv_l00":
        out.append(Launch("conv_0", "stem", "stem_h3<FLAT3,vel,nodx>" if f.vel else "stem_h3<FLAT3,novel>", dv0, cin, cmid, 0, None))
    else:
        k = wk if _h3w(f.prec, dv0[0], wino, [nchunk(cin)], split) else "h3g_wide"
        out.append(Launch("conv_0", k, _LABEL[k], dv0, cin, cmid, 0, None if split is None else split // per))
    k = wk if _h3w(f.prec, dv1[0], wino, [nchunk(cmid), nchunk(cin)], split) else "h3g_wide"
    assert k != "h3g_wide" or (f.prec == "f16x3" and f.vel), (case.name, form)       # the one direct kernel with a fused skip
    out.append(Launch("conv_1", k, _LABEL[k], dv1, cmid, cout, nchunk(cin) // per, None if split is None else split // per))
    return out


def labels(case, form):
    """{profile label: launches} of one run_case call on the case"""
    n = collections.Counter()
    for src in sources(case, form):
        for la in launches(case, form, src):
            n[la.label] += 1
    return dict(n)


def paths(case, form, src):
    """the exact path word of nbe_test_block (run_conv, nbe_engine_net.cpp:110-114)"""
    c0, c1 = launches(case, form, src)
    p = {"skip_fused"}
    if case.block == "conv_l00":
        p.add("skip_nodx")
    if src == "two":
        p |= {"two_source", "two_source_skip"}
    if c0.kernel.startswith("h3w"):
        p.add("wino_0")
    if c1.kernel.startswith("h3w"):
        p.add("wino_1")
    return p


# ---- the cases ---------------------------------------------------------------------------------------------------------
ALL = "wgnh"

# a block per width of the skip's chunk loop, at a result of 4 x 9 x 33: one row and one column into the last tiles
BLOCKS = [
    _c("l01-m64", (4, 9, 33), ALL, "nskip 4 (two float16 stages); grid 8 on conv_h3w"),
    _c("r00-m64", (4, 9, 33), ALL, "nskip 8, the sources switching at chunk 4: both weight homes of sk_wbase", block="conv_r00"),
    _c("r00-m16", (4, 9, 33), "wgn", "nskip 2, switching at chunk 1; a 16-channel cout tile", block="conv_r00", mid=16),
    _c("l01-m24", (4, 9, 33), "wgn", "24 channels padded to 32: nskip 2, a ragged channel group", mid=24),
    _c("l00-m64", (4, 9, 33), "wgn", "nskip 1, F_SKIP_NODX; conv_0 on the stem kernel", block="conv_l00"),
]

# rows and columns, two result planes: the result's extents AND the hidden tensor's (+ 2) each visit 7, 8, 9, 15, 16, 17 rows
# and 31, 32, 33, 63, 64, 65 columns; for the 16-row tiles of the n form also 23, 24, 25
EDGES = [
    _c("e5x29", (2, 5, 29), ALL, "hidden 7 x 31: conv_0 one row and one column short of a tile"),
    _c("e6x30", (2, 6, 30), ALL, "hidden exactly 8 x 32, the result not"),
    _c("e7x31", (2, 7, 31), ALL, "one short of the tile; hidden 9 x 33"),
    _c("e8x32", (2, 8, 32), ALL, "exactly one 8 x 32 tile: one workgroup; the n form's second row block wholly masked"),
    _c("e9x33", (2, 9, 33), ALL, "one row and one column into the last tiles; one second-block row stored; direct grid 8"),
    _c("e13x61", (2, 13, 61), ALL, "hidden 15 x 63"),
    _c("e14x62", (2, 14, 62), ALL, "hidden exactly 16 x 64, the result not"),
    _c("e15x63", (2, 15, 63), ALL, "one short of two tiles; 7 second-block rows stored; hidden 17 x 65"),
    _c("e16x64", (2, 16, 64), ALL, "exactly 2 x 2 tiles (1 x 2 of 16 rows, the second row block whole)"),
    _c("e17x65", (2, 17, 65), ALL, "3 x 3 tiles, the last ones one row, one column"),
    _c("e16x32", (2, 16, 32), "wn", "exactly one 16 x 32 tile of the n form: one workgroup"),
    _c("e14x30", (2, 14, 30), "wn", "n form: hidden exactly one 16 x 32 tile"),
    _c("e21x33", (2, 21, 33), "wn", "n form: hidden 23 rows"),
    _c("e22x32", (2, 22, 32), "wn", "n form: hidden 24 rows"),
    _c("e23x31", (2, 23, 31), "wn", "n form: one row short of a second tile's second block; hidden 25 rows"),
    _c("e24x32", (2, 24, 32), "wn", "n form: the last tile's second row block stores nothing"),
    _c("e25x33", (2, 25, 33), "wn", "n form: one row in the last tile's second block"),
]

# planes, at 9 x 33 (2 x 2 tiles of 8 rows, 1 x 2 of 16): zblock = 8 pairs.  conv_0 runs two planes more than conv_1
PLANES = [
    _c("z14", (14, 9, 33), "wg", "conv_0 on 16 planes: one whole block of pairs"),
    _c("z16", (16, 9, 33), ALL, "8 pairs: one whole block, no remainder; conv_0 on 18 planes, remainder 1"),
    _c("z18", (18, 9, 33), ALL, "9 pairs: remainder 1; conv_0 remainder 2"),
    _c("z20", (20, 9, 33), ALL, "conv_0 on 22 planes: remainder 3"),
    _c("z22", (22, 9, 33), ALL, "11 pairs: remainder 3; conv_0 on 24 planes, remainder 4"),
    _c("z30", (30, 9, 33), ALL, "conv_0 on 32 planes: two whole blocks"),
    _c("z32", (32, 9, 33), ALL, "16 pairs: two whole blocks, blk > 0; conv_0 on 34 planes, two blocks and remainder 1"),
    _c("z3", (3, 9, 33), "g", "odd: conv_0 (5 planes) and conv_1 both on the direct fused kernel, no switch"),
    _c("z17", (17, 9, 33), "g", "odd, 17 planes: the direct kernel's z decode beyond 16"),
    _c("r00-m16-z18", (18, 9, 33), "wn", "two sources with a remainder pair", block="conv_r00", mid=16),
]

# workgroups of the conv_1 launch: pairs x tiles (w, h), pairs x 16-row tiles (n), planes x tiles (g)
GRIDS = [
    _c("g-grid1", (1, 8, 32), "g", "direct: one workgroup"),
    _c("grid7", (14, 5, 20), "wnh", "seven workgroups, one per plane pair: XCD 7 idle"),
    _c("g-grid7", (7, 8, 20), "g", "direct: seven workgroups"),
    _c("grid9", (6, 17, 30), "wh", "nine workgroups: XCD 0 runs two"),
    _c("g-grid9", (3, 17, 30), "g", "direct: nine workgroups"),
    _c("grid15", (10, 20, 19), "wh", "15 workgroups"),
    _c("g-grid15", (5, 20, 32), "g", "direct: 15 workgroups"),
    _c("grid17", (34, 6, 21), "wnh", "17 workgroups (XCD 0 runs three), the last pair in the remainder branch"),
    _c("g-grid17", (17, 4, 30), "g", "direct: 17 workgroups"),
    _c("n-grid8", (4, 17, 33), "wn", "n form: 2 pairs x 2 x 2 tiles of 16 rows"),
    _c("n-grid9", (6, 33, 30), "wn", "n form: 3 pairs x 3 tiles"),
    _c("n-grid15", (10, 36, 19), "wn", "n form: 5 pairs x 3 tiles"),
]

# periodic in y and x (level-0 blocks): the hidden tensor has the result's extents, every tensor a filled halo
PERIODIC = [
    _c("p8x32", (2, 8, 32), ALL, "periodic: exactly one tile in both launches", pad=1),
    _c("p9x33", (2, 9, 33), ALL, "periodic: one row and column into the last tiles, two sources", block="conv_r00", pad=1),
    _c("p16x64", (2, 16, 64), "wn", "periodic: exactly 1 x 2 tiles of 16 rows", pad=1),
]

CASES = BLOCKS + EDGES + PLANES + GRIDS + PERIODIC
BY_NAME = {c.name: c for c in CASES}
PARITY = [(c, f) for c in CASES for f in ALL if f in c.forms]


def launch_tiling(la):
    """patch_cases.Tiling of a launch (None for the stem kernel, whose tiling is tests/stream_cases.py's)"""
    return None if la.kernel == "stem" else tiling(la.kernel, la.dv, la.cout)
