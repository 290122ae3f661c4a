"""Case table of tests/test_gpu_patch_layers.py, and the tiling of the kernels it is aimed at, restated in plain Python.

The 3x3x3 layers behind the first one run on the 2-D patch kernels (csrc/nbe_kernels_h3.hip) and on the Winograd-z kernel
(csrc/nbe_kernels_wino.h).  Every shape below is chosen from the tiling of the kernel that runs it; tests/test_patch_cases.py
holds the table to the edges it was chosen for.  Shapes are OUTPUT extents (Dv, Hv, Wv); the input is two larger per axis.

Patch tiles (nbe_conv_select.h:68-73)
  * tiles_of(n, tile) = ceil(n / tile); patch_tiles sets tny = tiles_of(Hv, rows), tnx = tiles_of(Wv, 32) and returns
    nz tny tnx: nz = Dv planes for the direct kernels (nbe_kernels_h3.hip:1079, :1465, :1785, :1811), nz = Dv / 2 plane
    pairs for conv_h3w_kernel (nbe_kernels_wino.h:903);
  * rows = 8 (HP_ROWS) for conv_h3p / h3q / h3g and conv_h3w with a tangent, 16 (H2_ROWS) for conv_h2q
    (nbe_kernels_h3.hip:1785) and for the displacement-only conv_h3w (2 HP_ROWS, nbe_kernels_wino.h:902);
  * every kernel fetches the whole (rows + 2) x 34 input patch of its tile; rows >= Hv and columns >= Wv are masked in the
    epilogue (ook: nbe_kernels_h3.hip:1016, :1380, :1721; nbe_kernels_wino.h:746).

Cout tiles and the grid
  * a cout tile is 64 channels = 8 groups of 8: nct = ceil(ceil(cout / 8) / 8) (nbe_kernels_h3.hip:804, :1153, :1525;
    nbe_kernels_wino.h:123), equal to the packing's ctiles (cout_tiles_ok, nbe_conv_select.h:76);
  * conv_h3q / h3g / h2q / h3w launch ntiles * nct workgroups in one dimension; workgroup b runs
    vt = xcd_tile(b, ntiles * nct), tile = vt / nct, cout tile ct = vt % nct: the cout tile runs fastest
    (nbe_kernels_h3.hip:805-806, :1154-1155, :1526-1527; nbe_kernels_wino.h:126-127);
  * conv_h3p launches (ntiles, nct): tile = xcd_tile(blockIdx.x, ntiles), ct = blockIdx.y (nbe_kernels_h3.hip:554-555, :1812).

Tile -> patch
  * direct kernels, z fastest: z = tile % Dv, tyx = tile / Dv, ty = tyx / tnx, tx = tyx % tnx
    (nbe_kernels_h3.hip:556-557, :807-808, :1156-1157, :1528-1529);
  * conv_h3w, plane pairs fastest in blocks of zblock = min(8, Dv / 2) (nbe_kernels_wino.h:912): with npair = Dv / 2,
    full = (npair / zblock) zblock and per_blk = zblock tny tnx, a tile below (npair / zblock) per_blk is
    (blk, r) = divmod(tile, per_blk), zp = blk zblock + r % zblock, tyx = r / zblock; the others are the REMAINDER
    branch: r = tile - (npair / zblock) per_blk, rem = npair - full, zp = full + r % rem, tyx = r / rem
    (nbe_kernels_wino.h:128-146); the planes are z0 = 2 zp and z0 + 1.

The displacement-only conv_h3w owns two blocks of eight rows per tile: rows y0 + r and y0 + 8 + r of wave row r; the
second block is stored where yy + HP_ROWS < Hv (ook2, nbe_kernels_wino.h:747).

Which kernel runs (conv_select, h3w_ok and conv_label of nbe_conv_select.h, through the layer hooks of
nbe_engine_test.cpp): see select() below."""

import collections
import zlib

import numpy as np

from stream_cases import xcd_tile, rand

HP_ROWS, HP_COLS, H2_ROWS = 8, 32, 16          # nbe_conv_select.h:15-16
CHUNK = 16                                     # H3_CHUNK, nbe_conv_select.h:14
COUT_TILE = 64
ZBLOCK = 8                                     # nbe_kernels_wino.h:912
MAX_WSTAGES = 32                               # NBE_MAX_WSTAGES, nbe_conv_select.h:24
F16_CHUNKS = 2                                 # H3W_F16_CHUNKS, nbe_conv_select.h:26


# ---- the tiling, restated ---------------------------------------------------------------------------------------------------
def tiles_of(n, tile):
    return (n + tile - 1) // tile


def patch_tiles(hv, wv, rows, nz):
    """(tny, tnx, ntiles)"""
    tny, tnx = tiles_of(hv, rows), tiles_of(wv, HP_COLS)
    return tny, tnx, nz * tny * tnx


def nchunk(cin):
    """16-channel K chunks of the packing (cin_pad / 16: layer_geometry, nbe_engine_weights.cpp:17)"""
    return (cin + CHUNK - 1) // CHUNK


def cout_groups(cout):
    return (cout + 7) // 8                     # nbe_kernels.hip:262


def nct(cout):
    return (cout_groups(cout) + 7) // 8


def decode_z(tile, dv, tnx):
    """(z, ty, tx) of a tile of the direct kernels"""
    z, tyx = tile % dv, tile // dv
    return z, tyx // tnx, tyx % tnx


def zblock(dv):
    return min(ZBLOCK, dv // 2)


def decode_pairs(tile, dv, tny, tnx):
    """(zp, ty, tx, in the remainder branch) of a tile of conv_h3w_kernel"""
    npair, zb = dv // 2, zblock(dv)
    full, per_blk = (npair // zb) * zb, zb * tny * tnx
    if tile < (npair // zb) * per_blk:
        blk, r = divmod(tile, per_blk)
        zi, tyx = r % zb, r // zb
        return blk * zb + zi, tyx // tnx, tyx % tnx, False
    r, rem = tile - (npair // zb) * per_blk, npair - full
    zi, tyx = r % rem, r // rem
    return full + zi, tyx // tnx, tyx % tnx, True


def second_block_rows(y0, hv):
    """rows of the displacement-only form's second row block that are stored (ook2): yy + 8 < Hv for yy = y0 .. y0 + 7"""
    return sum(1 for r in range(HP_ROWS) if y0 + r + HP_ROWS < hv)


# kernel -> (tile rows, planes per tile, tile decode, cout tile in the grid's second dimension)
Geometry = collections.namedtuple("Geometry", "rows zper pairs grid2d")
KERNELS = {
    "h3q": Geometry(HP_ROWS, 1, False, False),
    "h3g_wide": Geometry(HP_ROWS, 1, False, False),
    "h2q_split": Geometry(H2_ROWS, 1, False, False),
    "h2q_f16": Geometry(H2_ROWS, 1, False, False),
    "h2q_f16_g": Geometry(H2_ROWS, 1, False, False),
    "h3p": Geometry(HP_ROWS, 1, False, True),
    "h3w_f16x3": Geometry(HP_ROWS, 2, True, False),
    "h3w_f16": Geometry(HP_ROWS, 2, True, False),
    "h3w_novel": Geometry(2 * HP_ROWS, 2, True, False),
}

Tiling = collections.namedtuple("Tiling", "rows tny tnx ntiles nct grid remainder")


def tiling(kernel, dv, cout):
    """of a launch of `kernel` on output extents dv: grid = workgroups along x; remainder = tiles of conv_h3w's second branch"""
    g = KERNELS[kernel]
    tny, tnx, nt = patch_tiles(dv[1], dv[2], g.rows, dv[0] // g.zper)
    n = nct(cout)
    rem = sum(1 for t in range(nt) if decode_pairs(t, dv[0], tny, tnx)[3]) if g.pairs else 0
    return Tiling(g.rows, tny, tnx, nt, n, nt if g.grid2d else nt * n, rem)


def walk(kernel, dv, cout):
    """[(z or zp, ty, tx, ct)] in workgroup order, as the kernel decodes blockIdx"""
    g, t = KERNELS[kernel], tiling(kernel, dv, cout)
    out = []
    if g.grid2d:
        for ct in range(t.nct):
            for b in range(t.ntiles):
                out.append(decode_z(xcd_tile(b, t.ntiles), dv[0], t.tnx) + (ct,))
        return out
    for b in range(t.grid):
        vt = xcd_tile(b, t.ntiles * t.nct)
        tile, ct = vt // t.nct, vt % t.nct
        place = decode_pairs(tile, dv[0], t.tny, t.tnx)[:3] if g.pairs else decode_z(tile, dv[0], t.tnx)
        out.append(place + (ct,))
    return out


# ---- which kernel runs ---------------------------------------------------------------------------------------------------------
# A launch form is (arithmetic, tangent, NBE_WINO): tangent "gauged" goes through nbe_test_layer_gauged (beta), "vel" and
# "novel" through nbe_test_layer with and without dw.
Form = collections.namedtuple("Form", "prec tangent wino")

BASE_FORMS = [Form("f16x3", "gauged", True), Form("f16x3", "gauged", False)]
REP_FORMS = [Form("f16x3", "vel", True), Form("f16x3", "novel", True), Form("f16x3", "novel", False),
             Form("f16", "gauged", True), Form("f16", "vel", True), Form("f16", "novel", True),
             Form("f32", "vel", True), Form("f32", "gauged", True)]
RES_FORMS = [Form("f16x3", "vel", True), Form("f16", "gauged", True), Form("f16", "gauged", False)]


def form_id(f):
    return "%s-%s%s" % (f.prec, f.tangent, "" if f.wino else "-direct")


def packs_wino(prec, tangent, cin):
    """does the hook hand the launch a Winograd-z packing?  nbe_engine_test.cpp:78: only the gauged and the displacement-only
    launches; packs_wino / wino_f16_layer (nbe_engine_weights.cpp:34, nbe_engine_net.cpp:78): f16x3 with cin_pad <= 128,
    float16 with velocity, whole 32-channel stages and cin_pad <= 256"""
    if tangent == "vel":
        return False
    n = nchunk(cin)
    if prec == "f16x3":
        return 4 * n <= MAX_WSTAGES
    if prec == "f16":
        return tangent == "gauged" and n % F16_CHUNKS == 0 and 4 * (n // F16_CHUNKS) <= MAX_WSTAGES
    return False


def h3w_ok(prec, tangent, wino, cin, dv, res):
    """h3w_ok (nbe_conv_select.h:97-110) for a launch of the hooks (one source, no fused skip, small tensors); ka.ww is the
    packing where NBE_WINO allows it (run_conv, nbe_engine_net.cpp:100; launch_conv, nbe_kernels.hip:257)"""
    n = nchunk(cin)
    f16 = prec == "f16"
    if f16:
        if tangent != "gauged" or n & 1:
            return False
        n //= F16_CHUNKS
    ww = wino and packs_wino(prec, tangent, cin)
    return bool(ww and not (not f16 and res) and dv[0] % 2 == 0 and 4 * n <= MAX_WSTAGES)


def select(form, cin, dv, res=False):
    """(ConvKernel name, profile label prefix) of a launch: conv_select (nbe_conv_select.h:114-162) and conv_label (:166-188)"""
    prec, tangent, wino = form
    if prec == "f32":                                            # :118-121
        if tangent == "gauged":
            return "mfma_g", "conv_mfma_g<FLAT3,vel,dx,ni"
        return "mfma", "conv_mfma<FLAT3,%s,ni" % ("vel,dx" if tangent == "vel" else "novel,nodx")
    ok = h3w_ok(prec, tangent, wino, cin, dv, res)
    if tangent == "gauged":                                      # :133-145
        if prec == "f16x3":
            return ("h3w_f16x3", "conv_h3w<FLAT3,vel,dx>") if ok else ("h3g_wide", "conv_h3g<FLAT3,vel,dx>")
        return ("h3w_f16", "conv_h1w<FLAT3,vel,dx>") if ok else ("h2q_f16_g", "conv_h1g<FLAT3,vel,dx>")
    if prec == "f16x3":                                          # :146-150
        if tangent == "vel":
            return "h3q", "conv_h3<FLAT3,vel,dx>"
        return ("h3w_novel", "conv_h3w<FLAT3,novel>") if ok else ("h2q_split", "conv_h3<FLAT3,novel,nodx>")
    if tangent == "vel":                                         # :151
        return "h2q_f16", "conv_h1<FLAT3,vel,dx>"
    return "h3p", "conv_h1<FLAT3,novel,nodx>"                    # :154


# ---- the cases ---------------------------------------------------------------------------------------------------------
# rep: the case stands for a tiling situation and also runs on the launch forms beside the gauged f16x3 one (REP_FORMS);
# res: a residual is added before the activation, which brings RES_FORMS
Case = collections.namedtuple("Case", "name cin cout dv act res rep why")


def _c(name, dv, why, cin=16, cout=24, act=True, res=False, rep=False):
    return Case(name, cin, cout, dv, act, res, rep, why)


EDGES = [
    _c("e1x1", (2, 1, 1), "one output per plane: 255 of 256 lanes of the tile masked"),
    _c("e7x31", (2, 7, 31), "one row and one column short of the 8 x 32 tile"),
    _c("e8x32", (2, 8, 32), "exactly one 8 x 32 tile: no masked lane", rep=True),
    _c("e9x33", (2, 9, 33), "four tiles, three of them holding one row or one column", rep=True),
    _c("e15x17", (2, 15, 17), "one row short of the 16-row tile, one column into the second 16-column MFMA tile"),
    _c("e16x16", (2, 16, 16), "exactly one 16-row tile; exactly one 16-column MFMA tile"),
    _c("e17x15", (2, 17, 15), "one row past the 16-row tile, one column short of an MFMA tile", rep=True),
    _c("e8x65", (2, 8, 65), "tnx = 3, the last tile holds one column"),
    _c("e25x32", (2, 25, 32), "tny = 4; the 16-row tiles have one row in their second tile's first block", rep=True),
]

ODD = [
    _c("d1-9x33", (1, 9, 33), "a single plane: no Winograd-z form, the direct kernels' z decode with Dv = 1"),
    _c("d3-9x33", (3, 9, 33), "three planes: no Winograd-z form"),
    _c("d-grid1", (1, 5, 9), "direct kernels: one workgroup"),
    _c("d-grid7", (7, 8, 20), "direct kernels: seven workgroups (XCD 7 idle)"),
    _c("d-grid9", (3, 17, 31), "direct kernels, 8-row tiles: nine workgroups (XCD 0 runs two)"),
    _c("d-grid15", (5, 20, 32), "direct kernels, 8-row tiles: 15 workgroups"),
    _c("d-grid17", (17, 4, 30), "direct kernels: 17 workgroups (XCD 0 runs three)"),
    _c("d-nct2-odd", (3, 17, 20), "direct kernels: nine tiles x two cout tiles, the second holding one channel group", cout=72),
]

ORDER = [
    _c("z16", (16, 9, 33), "8 plane pairs: one whole block of the tile order, 32 tiles, no remainder tile", cout=64, rep=True),
    _c("z18", (18, 9, 33), "9 pairs: rem 1 beside two cout tiles, grid 72, 4 remainder tiles", cin=64, cout=72, rep=True),
    _c("z22", (22, 17, 33), "11 pairs: rem 3; 66 tiles of 8 rows (18 in the remainder), 44 of 16 rows (12)", cin=64, cout=64, rep=True),
    _c("z34", (34, 9, 65), "17 pairs: two whole blocks plus rem 1, 102 tiles, 6 in the remainder", rep=True),
]

GRIDS = [
    _c("grid7", (14, 5, 20), "conv_h3w: seven workgroups, one per plane pair (XCD 7 idle); 14 on the direct kernels", rep=True),
    _c("grid9", (6, 17, 30), "conv_h3w: nine workgroups (XCD 0 runs two); 18 on the direct kernels", rep=True),
    _c("grid15", (10, 20, 19), "conv_h3w: 15 workgroups"),
    _c("grid17", (34, 6, 21), "conv_h3w: 17 workgroups (XCD 0 runs three), the last pair in the remainder branch"),
    _c("nct2-odd", (2, 17, 20), "three tiles x two cout tiles: a tile's two workgroups land on different XCDs", cout=128),
    _c("cout68-2t", (2, 9, 20), "two tiles; the second cout tile holds one ragged channel group (4 of 8)", cout=68),
    _c("cout72-2t", (2, 9, 20), "two tiles; the second cout tile holds one whole channel group", cout=72, rep=True),
]

_CH = (4, 9, 33)
CHANNELS = [
    _c("cin8", _CH, "half a chunk of input channels, padded", cin=8, cout=64),
    _c("cin16", _CH, "one chunk: float16 has an odd chunk count", cin=16, cout=64),
    _c("cin24", _CH, "24 channels padded to two chunks; activation off", cin=24, cout=64, act=False),
    _c("cin48", _CH, "three chunks: never run before; odd for float16", cin=48, cout=64, rep=True),
    _c("cin64", _CH, "64 -> 64, the network's layer", cin=64, cout=64),
    _c("cin96", _CH, "six chunks, 24 stages: never run before; three float16 stages (an odd count)", cin=96, cout=64, rep=True),
    _c("cin128", _CH, "eight chunks: 32 stages, exactly NBE_MAX_WSTAGES", cin=128, cout=64, rep=True),
    _c("cout3", _CH, "the head's width on the wide tile: one ragged channel group", cin=64, cout=3),
    _c("cout8", _CH, "one channel group; activation off", cin=64, cout=8, act=False),
    _c("cout24", _CH, "three channel groups", cin=64, cout=24),
    _c("cout68", _CH, "two cout tiles, the second ragged", cin=64, cout=68),
    _c("cout128", _CH, "two whole cout tiles", cin=64, cout=128),
    _c("c128-128", _CH, "the widest layer: 32 stages and two cout tiles", cin=128, cout=128),
]

# A residual takes the f16x3 gauged launch off conv_h3w (h3w_ok refuses F_RES there), so the residual cases are cases of their
# own beside the channel cases above, whose chunk and cout counts all run on conv_h3w
RESIDUAL = [
    _c("res-64-64", _CH, "the network's conv_1 with its residual: conv_h3g, conv_h3q, the float16 F_RES epilogue (two stages)",
       cin=64, cout=64, res=True),
    _c("res-64-24", _CH, "a residual on three channel groups", cin=64, cout=24, res=True),
    _c("res-32-64", _CH, "a residual on one float16 stage", cin=32, cout=64, res=True),
]

# The float16 Winograd-z form needs whole 32-channel stages, so the 16 -> 24 cases above run on conv_h2q<false, true> there:
# cin-32 twins of a ragged, a four-row-tile and a two-block shape bring that form to the same edges
TWINS = [
    _c("e9x33-c32", (2, 9, 33), "e9x33 with one float16 stage", cin=32, rep=True),
    _c("e25x32-c32", (2, 25, 32), "e25x32 with one float16 stage", cin=32, rep=True),
    _c("z34-c32", (34, 9, 65), "z34 with one float16 stage: two blocks plus rem 1 on conv_h1w", cin=32, rep=True),
]

CASES = EDGES + ODD + ORDER + GRIDS + CHANNELS + RESIDUAL + TWINS
BY_NAME = {c.name: c for c in CASES}


def forms(case):
    """the launch forms a case runs on; a form whose NBE_WINO=0 twin selects the same kernel runs once"""
    fs = BASE_FORMS + (REP_FORMS if case.rep else []) + (RES_FORMS if case.res else [])
    out = []
    for f in fs:
        if not f.wino and select(f, case.cin, case.dv, case.res) == select(f._replace(wino=True), case.cin, case.dv, case.res):
            continue
        if f not in out:
            out.append(f)
    return out


def dims(case):
    return tuple(n + 2 for n in case.dv)


# ---- seeded operands ---------------------------------------------------------------------------------------------------------
Operands = collections.namedtuple("Operands", "x dx w dw beta b r dr")


def make_operands(cin, cout, dims_, seed, res=False):
    """float32: w has unit-norm rows, as the modulation leaves them (test_gpu_layers.py::test_layer_gauged) -- the gauged forms
    take (w, beta), their oracle dw = w beta; the plain forms take (w, dw) with dw as test_layer_vel draws it"""
    rng = np.random.default_rng(seed)
    x, dx = rand(rng, cin, *dims_), rand(rng, cin, *dims_)
    w = rand(rng, cout, cin, 3, 3, 3)
    w /= np.sqrt((w.astype(np.float64) ** 2).sum(axis=(1, 2, 3, 4), keepdims=True)).astype(np.float32)
    dw = (rand(rng, cout, cin, 3, 3, 3) / np.sqrt(cin * 27)).astype(np.float32)
    beta = (0.3 * rand(rng, cout)).astype(np.float32)
    b = 0.1 * rand(rng, cout)
    out = (cout,) + tuple(n - 2 for n in dims_)
    r, dr = (rand(rng, *out), rand(rng, *out)) if res else (None, None)
    return Operands(x, dx, w, dw, beta, b, r, dr)


def operands(case):
    return make_operands(case.cin, case.cout, dims(case), zlib.crc32(case.name.encode()), case.res)
