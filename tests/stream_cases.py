"""Case tables of tests/test_gpu_stream_layers.py, and the tiling of the kernels they are aimed at, restated in plain Python.

Three layer families run outside the patch and Winograd kernels (csrc/nbe_kernels_h3.hip, csrc/nbe_kernels.hip):
the first layer (stem_h3_kernel), 2x up-sampling (up_h3_kernel, eight parities in one launch) and the 2x2x2 stride-2
layers and unfused 1x1x1 skips (conv_h3_kernel<MODE_DOWN / MODE_FLAT1>, conv_mfma_kernel in strict float32).  Every
shape below is chosen from the tiling of the kernel that runs it; tests/test_stream_cases.py holds the tables to the
edges they were chosen for.

The flat kernels (conv_h3_kernel, up_h3_kernel, conv_mfma_kernel)
  * a tile is TILE_VOX = 256 flat positions (nbe_kernels.h:49; UP_XV, nbe_kernels_h3.hip:371);
  * Q = Dv Hv Wv for MODE_DOWN (output positions), else Q = ((Dv - 1) H + Hv - 1) W + Wv: positions of the INPUT pitch
    (H, W) up to the last valid one, rows and planes beyond (Hv, Wv) masked in the epilogue (nbe_kernels.hip:247-248;
    the masks: nbe_kernels_h3.hip:336, :348, :482);
  * ntiles = ceil(Q / 256) (nbe_kernels.hip:279), workgroup b runs tile xcd_tile(b, ntiles)
    (nbe_kernels_internal.h:71-74): workgroups go round the 8 XCDs, and each XCD takes a contiguous run of tiles, the
    first ntiles & 7 XCDs one tile more;
  * conv_h3_kernel: wave w owns positions 64 (w >> 1) + 32 jt + lane % 32 of its tile (nbe_kernels_h3.hip:335);
  * up_h3_kernel: a tile is two halves of 128 positions, each four wave quarters of 32: position
    q0 + 128 half + 32 (wave >> 1) + lane % 32 (nbe_kernels_h3.hip:442, :479); the input's nchunk = cin_pad / 16 <= 4
    chunks of 16 channels stay resident in LDS (nbe_kernels.hip:260, nbe_kernels_h3.hip:372, :500).

The stem (stem_h3_kernel)
  * a tile is 1 row x 128 columns of one output plane (ST_ROWS, ST_COLS: nbe_kernels_h3.hip:1863), tnx = ceil(Wv / 128),
    nt = Dv Hv tnx, grid = min(nt, 512) (nbe_kernels_h3.hip:2065-2070);
  * workgroup b walks tiles b, b + grid, ...; iteration `it` stages its patch in buffer it & 1
    (nbe_kernels_h3.hip:1938, :1949-1951);
  * wave w owns columns 32 w .. 32 w + 31 of the tile (nbe_kernels_h3.hip:1947, :2000)."""

import collections
import zlib

import numpy as np

TILE = 256                     # TILE_VOX, UP_XV
HALF, QUARTER = 128, 32        # up_h3_kernel: positions of a tile half, of a wave quarter
XCDS = 8
STEM_COLS, STEM_GRID, STEM_WAVE = 128, 512, 32
K = {"conv3": 3, "skip": 1, "down": 2, "up": 2}

Case = collections.namedtuple("Case", "name kind cin cout dims crop has_dx rep why")


# ---- the tiling, restated ---------------------------------------------------------------------------------------------------
def out_dims(kind, dims, crop=0):
    """(Dv, Hv, Wv) of the launch: the output extents (up: the input's, each position gives eight outputs)"""
    D, H, W = dims
    if kind == "conv3":
        return D - 2, H - 2, W - 2
    if kind == "skip":
        return D - 2 * crop, H - 2 * crop, W - 2 * crop
    if kind == "down":
        return D // 2, H // 2, W // 2
    return D, H, W


def flat_q(kind, dims, crop=0):
    Dv, Hv, Wv = out_dims(kind, dims, crop)
    if kind == "down":
        return Dv * Hv * Wv
    return ((Dv - 1) * dims[1] + Hv - 1) * dims[2] + Wv


def ntiles(q):
    return (q + TILE - 1) // TILE


def xcd_tile(b, nt):
    qd, rm, xcd = nt >> 3, nt & 7, b & 7
    return (xcd * (qd + 1) if xcd < rm else rm * (qd + 1) + (xcd - rm) * qd) + (b >> 3)


def nchunk(cin):
    return (cin + 15) // 16


def up_place(q):
    """(tile, half, wave quarter, lane) of flat position q in up_h3_kernel"""
    r = q % TILE
    return q // TILE, r // HALF, (r % HALF) // QUARTER, r % QUARTER


StemTiling = collections.namedtuple("StemTiling", "Dv Hv Wv tnx nt grid walks")


def stem_tiling(dims):
    """walks: the most tiles one persistent workgroup runs"""
    Dv, Hv, Wv = out_dims("conv3", dims)
    tnx = (Wv + STEM_COLS - 1) // STEM_COLS
    nt = Dv * Hv * tnx
    grid = min(nt, STEM_GRID)
    return StemTiling(Dv, Hv, Wv, tnx, nt, grid, (nt + grid - 1) // grid)


def stem_place(tl, z, y, x):
    """(tile, iteration of its workgroup, patch buffer, wave) of output voxel (z, y, x)"""
    tile = (z * tl.Hv + y) * tl.tnx + x // STEM_COLS
    return tile, tile // tl.grid, (tile // tl.grid) & 1, (x % STEM_COLS) // STEM_WAVE


# ---- the cases ---------------------------------------------------------------------------------------------------------
# rep: the case stands for a tiling situation (a residue class of Q or of Wv, a tiles-per-workgroup class) and also runs on the
# five (arithmetic, velocity) combinations beside f16x3 with velocity

def _stem(name, cin, cout, dims, rep, why):
    return Case("stem-" + name, "conv3", cin, cout, dims, 0, False, rep, why)


STEM = [
    _stem("w1", 3, 64, (3, 3, 3), False, "one output: 127 of 128 columns masked, three waves idle"),
    _stem("w31", 2, 24, (4, 5, 33), False, "one column short of a wave"),
    _stem("w32", 1, 8, (3, 4, 34), False, "exactly one wave"),
    _stem("w33", 3, 24, (5, 3, 35), True, "one column into the second wave; ragged tile, one tile per workgroup"),
    _stem("w64", 2, 64, (3, 3, 66), False, "ends on the second wave boundary"),
    _stem("w96", 1, 24, (3, 4, 98), False, "ends on the third wave boundary"),
    _stem("w127", 3, 8, (4, 4, 129), False, "one column short of a tile"),
    _stem("w128", 2, 64, (5, 5, 130), True, "exactly one tile per row: no masked column"),
    _stem("w129", 3, 64, (3, 5, 131), True, "tnx = 2, the second tile holds one column"),
    _stem("w257", 1, 24, (4, 3, 259), False, "tnx = 3"),
    _stem("nt512", 3, 24, (4, 130, 132), False, "2 x 128 x 2 = 512 tiles: the last size at which every workgroup runs one tile"),
    _stem("nt513", 3, 64, (5, 173, 35), True, "3 x 171 x 1 = 513 tiles: workgroup 0 alone runs a second tile, in patch buffer 1"),
    _stem("nt1548", 3, 8, (6, 131, 259), True, "4 x 129 x 3 = 1548 tiles: workgroups 0..11 walk four tiles, the rest three: "
                                               "a patch buffer is used again"),
]


def _up(name, cin, cout, dims, rep, why):
    return Case("up-" + name, "up", cin, cout, dims, 0, True, rep, why)


_UP_ROW_CH = {1: (8, 64), 31: (16, 24), 32: (24, 8), 33: (48, 64), 127: (64, 24), 128: (8, 8), 129: (16, 64),
              255: (64, 64), 256: (24, 24), 257: (48, 8)}
UP = [_up("row%d" % n, ci, co, (1, 1, n), n >= 255, "a single row of %d positions" % n) for n, (ci, co) in _UP_ROW_CH.items()]
UP += [
    _up("3x7x13", 64, 64, (3, 7, 13), False, "273 positions: rows of 13 straddle the tile boundary, 17 positions in the last tile"),
    _up("5x9x11", 24, 64, (5, 9, 11), False, "495 positions"),
    _up("4x16x16", 48, 24, (4, 16, 16), False, "1024 positions: four whole tiles, no masked lane"),
    _up("9x15x17", 64, 64, (9, 15, 17), True, "2295 positions: nine tiles, XCD 0 runs two"),
    _up("7tiles", 16, 8, (4, 11, 40), False, "1760 positions: seven tiles (XCD 7 idle), the last holds seven whole quarters"),
    _up("15tiles", 64, 24, (6, 24, 26), False, "3744 positions: 15 tiles, seven XCDs run two; the last holds five whole quarters"),
    _up("17tiles", 8, 64, (4, 8, 131), False, "4192 positions: 17 tiles, XCD 0 runs three; the last holds three whole quarters"),
    _up("q64", 24, 24, (4, 4, 4), False, "64 positions: two whole quarters"),
    _up("q192", 48, 64, (2, 3, 32), False, "192 positions: six whole quarters, two of them in the second half"),
]


def _down(name, c, dims, rep, why):
    return Case("down-" + name, "down", c, c, dims, 0, True, rep, why)


DOWN = [
    _down("q1", 64, (2, 2, 2), False, "Q = 1: 255 clamped entries of inbase"),
    _down("q255", 24, (2, 2, 510), True, "Q = 255"),
    _down("q256", 64, (2, 2, 512), True, "Q = 256: one whole tile"),
    _down("q257", 8, (2, 2, 514), True, "Q = 257: a second tile with one position"),
    _down("q129", 24, (2, 6, 86), False, "Q = 1 x 3 x 43 = 129: one position into the third pair of waves (64 positions each)"),
    _down("q2322", 64, (6, 18, 172), True, "Q = 3 x 9 x 86 = 2322: ten tiles, XCDs 0 and 1 run two"),
    _down("q2048", 24, (16, 32, 32), False, "Q = 8 x 16 x 16 = 2048 = 8 x 256: one whole tile per XCD"),
    _down("odd", 64, (5, 7, 9), True, "odd input extents: the VALID stride-2 sum floors to (2, 3, 4), the last plane, row and column are unread"),
]


def _skip(name, cin, cout, dims, rep, why):
    return Case("skip-" + name, "skip", cin, cout, dims, 2, cin > 3, rep, why)


SKIP = [
    _skip("q255", 128, 64, (5, 5, 259), True, "Q = 255 (one cropped row of 255); a decoder's 2m -> m"),
    _skip("q256", 64, 3, (5, 5, 260), True, "Q = 256; the head's 64 -> 3"),
    _skip("q257", 3, 64, (5, 5, 261), True, "Q = 257; conv_l00's 3 -> 64 without input tangent"),
    _skip("pitch-128-64", 128, 64, (6, 7, 45), True, "Q = (1 x 7 + 2) x 45 + 41 = 446 of the input's pitch: rows and a plane gap masked"),
    _skip("pitch-64-3", 64, 3, (6, 7, 45), False, "the same pitched count, 64 -> 3"),
    _skip("pitch-3-64", 3, 64, (7, 6, 40), False, "Q = (2 x 6 + 1) x 40 + 36 = 556, no input tangent"),
]

CASES = STEM + UP + DOWN + SKIP
FLAT = UP + DOWN + SKIP


# ---- seeded operands ---------------------------------------------------------------------------------------------------------
def rand(rng, *shape):
    return rng.standard_normal(shape).astype(np.float32)


def operands(case):
    """x, dx (None without input tangent), w, dw, b of a case, float32, seeded by its name"""
    rng = np.random.default_rng(zlib.crc32(case.name.encode()))
    k = K[case.kind]
    x = rand(rng, case.cin, *case.dims)
    dx = rand(rng, case.cin, *case.dims) if case.has_dx else None
    w = rand(rng, case.cout, case.cin, k, k, k) / np.sqrt(case.cin * k ** 3)
    dw = rand(rng, case.cout, case.cin, k, k, k) / np.sqrt(case.cin * k ** 3)
    b = 0.1 * rand(rng, case.cout)
    return x, dx, w.astype(np.float32), dw.astype(np.float32), b
