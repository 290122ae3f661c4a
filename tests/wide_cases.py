"""Case table of tests/test_gpu_wide_blocks.py: the network ABOVE width 64, where most of the fast paths stop and the engine's
planners choose the fall-back kernels.  What decides the launches of a block is restated here from the sources (file:line of
csrc/), one function per decision; the tiling is the restatement of tests/patch_cases.py, tests/fused_cases.py and
tests/stream_cases.py (imported, never copied).  tests/test_wide_cases.py holds the table to its limits on the CPU and walks
every 3x3x3 row through tools/conv_select_walk.hip.

What a loaded network packs per layer (nbe_engine_weights.cpp)
  packs_narrow      :30-32   f16x3 with velocity, a 3x3x3 or skip layer with cout <= 4 that is not conv_l00's first layer:
                             conv_r01/conv_1 and conv_r01/skip.  run_conv uses the packing only for a gauged launch
                             (nbe_engine_net.cpp:97).
  packs_wino        :34-36   a 3x3x3 layer behind the first: f16x3 without the narrow packing and 4 cin_pad / 16 <= 32 stages
                             (h3w_stages_fit, nbe_conv_select.h:61: cin_pad <= 128), or wino_f16_layer
  packs_wino_skip   :38-41   a skip: the same f16x3 condition, or (style tree, not conv_l00's) wino_f16_layer
  wino_f16_layer    nbe_engine_net.cpp:78-80   float16 with velocity, cin_pad a multiple of 32 and 4 cin_pad / 32 <= 32 stages
  packs_stem        :43-45   half precision, conv_l00/conv_0 with cin <= 3 and cout <= 64: above width 64 the first layer has
                             no stem packing and runs on conv_h3p (f16x3 with velocity, float16) or conv_h2q<SPLIT>
How the tangents are wired (nbe_engine_weights.cpp)
  wire_gauge        :155-211 every conv_1 and every conv_0 but conv_l00's is gauged (g6, :185-186).  A block's skip may run
                             inside conv_1 (fskip) where, f16x3 (:189-194), the narrow packing of conv_1 comes with the skip's and
                             3 cin_pad(conv_1) / 16 + cin_pad(skip) / 16 <= NBE_MAX_GROUPS = 64; float16 (:196-201), both have a
                             Winograd-z packing, the same cout tiles and 2 cin_pad(skip) / 32 <= NBE_MAX_WSKIP = 16.
                             :204-205: a gauged layer with 3 cin_pad / 16 > 64 turns the gauge off for the whole network,
                             whatever the arithmetic (float32 included), without a message.
  wire_novel        :131-150 displacement-only f16x3: every block fuses or none does; a block needs Winograd-z packings of
                             conv_1 and of the skip and 2 cin_pad(skip) / 16 <= 16
  pack_wino         :111-127 wino_ok: f16x3 (with velocity: only where the gauge is active) or float16 with velocity and an
                             active gauge; c->fuse follows it without velocity and for float16
What the schedule asks for (nbe_engine_net.cpp)
  block_fused       :159-161 c->fuse, fskip, and for displacement only and float16 a launch that can be the Winograd-z kernel:
                             NBE_WINO not 0 and an even number of result planes
  two_source_width  :165     mid a multiple of 16 (float16: 32, two_source_chunk, nbe_conv_select.h:64)
  up8_launch        :84      half precision and cin_pad / 16 <= 4 (up8_fits, nbe_conv_select.h:58): above width 64 every up_*
                             block is eight conv_h3_kernel<FLAT1> launches, one per parity (upblock :303-309)
Which kernel a launch gets (conv_select, nbe_conv_select.h:114-162)
  h3nz_ok           :91-94   at most 4 chunks of conv_1 and of the skip: from width 72 on the head runs conv_h3g_kernel<NARROW>
  h3g_ok            :87-89   3 nchunk + nskip <= 64 entries of ConvKArgs::gs
  h3w_ok            :97-110  a Winograd-z packing, NBE_WINO not 0, an even plane count, no residual on f16x3, 4 nchunk <= 32 and
                             2 nskip <= 16 (float16: in 32-channel stages, every chunk count and source switch even)
"""

import collections

import block_ref as B
from patch_cases import nchunk, nct, tiling, tiles_of, MAX_WSTAGES, F16_CHUNKS, CHUNK   # noqa: F401
from fused_cases import MAX_WSKIP, FORMS as _FUSED_FORMS, Form
from stream_cases import xcd_tile   # noqa: F401

MAX_GROUPS = 64                                # NBE_MAX_GROUPS, nbe_kernels.h:43
UP_MAXCH = HNZ_MAXCH = 4                       # nbe_conv_select.h:21-22
STEM_MAX_COUT = 64                             # packs_stem, nbe_engine_weights.cpp:44

# launch forms: fused_cases' four and strict float32
#   w  f16x3 with velocity     g  the same under NBE_WINO=0     n  f16x3, displacement only     h  float16     s  float32
FORMS = dict(_FUSED_FORMS, s=Form("f32", True, True))
ALL = "wgnhs"

WIDTHS = {
    72: "ragged chunk (pads to 80): no two-source form; head on NARROW with 5 + 5 chunks; decoders 144 -> 144 -> 72 on conv_h3g "
        "with 9 chunks and 3 cout tiles, the last ragged; encoders on conv_h3w with an odd nskip of 5; float16 has no Winograd-z "
        "form (80 and 144 are no multiples of 32)",
    80: "whole chunks: the f16x3 two-source form on conv_h3g switches at chunk 5; the float16 decoders run 5 stages with fused "
        "skips of 5; the float16 two-source form is refused",
    96: "float16 only: two-source form with 3 + 3 stages, encoders with 3",
    128: "32 stages, 16 skip entries and 64 groups, each met exactly; head on NARROW with 8 + 8 chunks",
    136: "one past the group table: decoder blocks unfused (a skip launch, then a residual conv_h3g), every other block fused; "
         "encoders (144 channels) leave conv_h3w",
    176: "gauge off: every layer on the three-product kernels, every gauge vector zero",
}
FORMS_OF = {72: ALL, 80: ALL, 96: "h", 128: ALL, 136: ALL, 176: ALL}
# the blocks whose launches differ from the width below: the three decoders, the head block, one encoder block, one up_*
SOME = ('conv_r2', 'conv_r1', 'conv_r00', 'conv_r01', 'conv_l01', 'up_r1')
BLOCKS_OF = {72: B.BLOCKS, 80: SOME, 96: SOME, 128: B.BLOCKS, 136: SOME, 176: SOME}


def pad16(c):
    return nchunk(c) * CHUNK


# ---- layers of a block -----------------------------------------------------------------------------------------------------------
Layer = collections.namedtuple("Layer", "block name kind cin cout first g6")


def layer(block, name, mid):
    """expected_shape (nbe_engine_weights.cpp:91-105) and the gauged flag of wire_gauge (:185-186)"""
    cin, cmid, cout = B.channels(block, mid)
    if name == "skip":
        return Layer(block, name, "skip", cin, cout, block == 'conv_l00', False)
    if block.startswith('down') or block.startswith('up'):
        return Layer(block, name, "down" if block.startswith('down') else "up", mid, mid, False, False)
    if name == "conv_0":
        return Layer(block, name, "conv3", cin, cmid, block == 'conv_l00', block != 'conv_l00')
    return Layer(block, name, "conv3", cmid, cout, False, True)


RES = tuple(b for b in B.BLOCKS if b.startswith('conv_'))


# ---- what a layer packs ------------------------------------------------------------------------------------------------------------
def packs_narrow(f, L):
    return f.prec == "f16x3" and f.vel and L.kind in ("conv3", "skip") and L.cout <= 4 and not L.first


def wino_f16_layer(f, cin):
    return f.prec == "f16" and f.vel and pad16(cin) % (CHUNK * F16_CHUNKS) == 0 and 4 * (pad16(cin) // (CHUNK * F16_CHUNKS)) <= MAX_WSTAGES


def _x3_wino(f, L):
    return f.prec == "f16x3" and not packs_narrow(f, L) and 4 * nchunk(L.cin) <= MAX_WSTAGES


def packs_wino(f, L):
    return L.kind == "conv3" and not L.first and (_x3_wino(f, L) or wino_f16_layer(f, L.cin))


def packs_wino_skip(f, L):
    return L.kind == "skip" and (_x3_wino(f, L) or (not L.first and wino_f16_layer(f, L.cin)))


def packs_stem(f, L):
    return f.prec != "f32" and L.kind == "conv3" and L.first and L.cin <= 3 and L.cout <= STEM_MAX_COUT


# ---- the wiring ------------------------------------------------------------------------------------------------------------------
def gauge_active(mid, f, gauge=True):
    """wire_gauge :204-205 (and NBE_GAUGE, nbe_engine_weights.cpp:393-394): the widest gauged layers are the decoders', 2 mid"""
    if not (f.vel and gauge):
        return False
    return all(3 * nchunk(layer(b, l, mid).cin) <= MAX_GROUPS for b in RES for l in ("conv_0", "conv_1") if layer(b, l, mid).g6)


def wino_ok(mid, f, gauge=True, wino_on=True):
    """pack_wino :113 and run_conv's policy (nbe_engine_net.cpp:100): may a launch of this context be the Winograd-z kernel?"""
    if not wino_on:
        return False
    ga = gauge_active(mid, f, gauge)
    return (f.prec == "f16x3" and (ga if f.vel else True)) or (f.prec == "f16" and f.vel and ga)


def novel_fuse(mid, f):
    """wire_novel: all blocks or none"""
    if f.vel or f.prec != "f16x3":
        return False
    return all(packs_wino(f, layer(b, "conv_1", mid)) and packs_wino_skip(f, layer(b, "skip", mid)) and
               2 * nchunk(layer(b, "skip", mid).cin) <= MAX_WSKIP for b in RES)


def fskip(block, mid, f, gauge=True):
    """does the block's conv_1 own its skip (Layer::fskip)?  wire_gauge :189-201, wire_novel :143-144"""
    L1, Ls = layer(block, "conv_1", mid), layer(block, "skip", mid)
    if not f.vel:
        return novel_fuse(mid, f)
    if not gauge:                                                # wire_gauge does not run (NBE_GAUGE=0)
        return False
    if f.prec == "f16x3":
        return (not packs_narrow(f, L1) or packs_narrow(f, Ls)) and 3 * nchunk(L1.cin) + nchunk(Ls.cin) <= MAX_GROUPS
    if f.prec == "f16":
        return (packs_wino(f, L1) and packs_wino_skip(f, Ls) and nct(L1.cout) == nct(Ls.cout) and
                2 * (pad16(Ls.cin) // (CHUNK * F16_CHUNKS)) <= MAX_WSKIP)
    return False


def expect_fused(block, mid, prec, vel, gauge, nres, wino_on):
    """block_fused (nbe_engine_net.cpp:159-161) for every width; for mid <= 64 it is test_gpu_blocks.expect_fused
    (tests/test_wide_cases.py compares them over the whole matrix)"""
    f = Form(prec, vel, wino_on)
    if prec == "f32":
        return False                                             # c->fuse needs a half-precision context (nbe_engine.cpp:264)
    if vel:
        fuse = gauge_active(mid, f, gauge) and (prec != "f16" or wino_ok(mid, f, gauge, True))
    else:
        fuse = novel_fuse(mid, f)                                # with wino_ok: the weights' range, not modelled
    if not (fuse and fskip(block, mid, f, gauge)):
        return False
    wino_only = not vel or prec == "f16"
    return not wino_only or (wino_on and nres % 2 == 0)


def two_source_width(mid, prec):
    return mid % (CHUNK * F16_CHUNKS if prec == "f16" else CHUNK) == 0


def up8_launch(mid, f):
    return f.prec != "f32" and nchunk(mid) <= UP_MAXCH


# ---- conv_select for the launches of a block ---------------------------------------------------------------------------------------
def h3w_ok(f, ww, wws, dv0, nch, nsk, res, novel, split=None, s_split=None, nodx=False):
    """nbe_conv_select.h:97-110; the counts in 16-channel chunks, split / s_split the chunk at which the sources switch"""
    f16 = f.prec == "f16"
    if f16:
        if novel or nch % 2 or (split is not None and split % 2):
            return False
        if nsk and (nsk % 2 or (s_split is not None and s_split % 2) or nodx):
            return False
        nch, nsk = nch // F16_CHUNKS, nsk // F16_CHUNKS
    if not ww or (not f16 and res) or dv0 % 2 or 4 * nch > MAX_WSTAGES:
        return False
    if nsk and (not wws or 2 * nsk > MAX_WSKIP):
        return False
    return True


def h3g_ok(nch, nsk):
    return 3 * nch + nsk <= MAX_GROUPS


def h3nz_ok(cout, nch, nsk, res, nodx):
    return cout <= 4 and not res and not nodx and nch <= HNZ_MAXCH and nsk <= HNZ_MAXCH


_M = {"conv3": "FLAT3", "skip": "FLAT1", "up": "FLAT1", "down": "DOWN"}


def label(kernel, f, L, has_dx):
    """conv_label, nbe_conv_select.h:166-188"""
    m, vel = _M[L.kind], f.vel
    fixed = {"stem": "stem_h3<FLAT3,vel,nodx>" if vel else "stem_h3<FLAT3,novel>",
             "up8": "up_h3<8 parities,vel,dx>" if vel else "up_h3<8 parities,novel>",
             "h3w_f16x3": "conv_h3w<FLAT3,vel,dx>", "h3w_novel": "conv_h3w<FLAT3,novel>", "h3w_f16": "conv_h1w<FLAT3,vel,dx>",
             "h3g_wide": "conv_h3g<%s,vel,dx>" % m, "h3g_narrow": "conv_h3n<%s,vel,dx>" % m, "h3nz": "conv_h3n<%s,vel,dx>" % m,
             "h2q_f16_g": "conv_h1g<%s,vel,dx>" % m}
    if kernel in fixed:
        return fixed[kernel]
    tang = "%s,%s" % ("vel" if vel else "novel", "dx" if (vel and has_dx) else "nodx")
    if kernel in ("mfma", "mfma_g"):
        ni = 2 if L.cout > 32 else 1                             # layer_geometry, nbe_engine_weights.cpp:15
        return "conv_mfma_g<%s,vel,dx,ni%d>" % (m, ni) if kernel == "mfma_g" else "conv_mfma<%s,%s,ni%d>" % (m, tang, ni)
    return "%s<%s,%s>" % ("conv_h1" if f.prec == "f16" else "conv_h3", m, tang)


def select3(f, mid, L, dv0, has_dx, gauge=True, wino_on=True, res=False, skip=None, two=False, s_two=False):
    """kernel of a 3x3x3 launch of layer L on dv0 planes.  skip: the fused skip's layer; two / s_two: the input's / the
    skip's sources switch at mid channels"""
    ga = gauge_active(mid, f, gauge)
    beta = ga and L.g6 and has_dx                                # run_conv, nbe_engine_net.cpp:90-92
    if f.prec == "f32":                                          # :118-121
        return "mfma_g" if beta else "mfma"
    narrow = beta and packs_narrow(f, L)                         # :97
    wok = wino_ok(mid, f, gauge, wino_on)
    ww = wok and not narrow and packs_wino(f, L)
    wws = wok and skip is not None and packs_wino_skip(f, skip)
    nch, nsk = nchunk(L.cin), (nchunk(skip.cin) if skip else 0)
    split, s_split = (mid // CHUNK if two else None), (mid // CHUNK if s_two else None)
    nodx = skip is not None and skip.first
    x3 = f.prec == "f16x3"
    if packs_stem(f, L) and not (f.vel and has_dx) and not res and not nsk and not beta:     # :124-125
        return "stem"
    if (nsk or two) and not (beta and x3):                                                 # :128-132
        if x3 and not f.vel:
            return "h3w_novel" if h3w_ok(f, ww, wws, dv0, nch, nsk, res, True, split, s_split, nodx) else "none"
        if not x3 and f.vel and has_dx and beta:
            return "h3w_f16" if h3w_ok(f, ww, wws, dv0, nch, nsk, res, False, split, s_split, nodx) else "none"
        return "none"
    if beta:                                                                               # :133-145
        if x3:
            if narrow:
                if h3nz_ok(L.cout, nch, nsk, res, nodx):
                    return "h3nz"
                return "h3g_narrow" if h3g_ok(nch, nsk) else "none"
            if h3w_ok(f, ww, wws, dv0, nch, nsk, res, False, split, s_split, nodx):
                return "h3w_f16x3"
            return "h3g_wide" if h3g_ok(nch, nsk) else "none"
        return "h3w_f16" if h3w_ok(f, ww, wws, dv0, nch, nsk, res, False, split, s_split, nodx) else "h2q_f16_g"
    if x3 and f.vel and has_dx:                                                            # :146-155
        return "h3q"
    if x3 and not f.vel:
        return "h3w_novel" if h3w_ok(f, ww, wws, dv0, nch, nsk, res, True) else "h2q_split"
    if not x3 and f.vel and has_dx:
        return "h2q_f16"
    return "h3p"


# ---- the launches of a block -----------------------------------------------------------------------------------------------------
Launch = collections.namedtuple("Launch", "layer kernel label dv cin cout nskip split res")


def _form(form):
    return FORMS[form] if isinstance(form, str) else form


def sources(block, mid, form, shape, gauge=True):
    """run_case runs a decoder block from two tensors as well where the block fuses and whole chunks (stages) allow"""
    f = _form(form)
    fused = expect_fused(block, mid, f.prec, f.vel, gauge, shape[0] - 4, f.wino)
    return ("cat", "two") if (block in B.DECODERS and two_source_width(mid, f.prec) and fused) else ("cat",)


def launches(block, mid, form, shape, src="cat", gauge=True):
    """the launches of nbe_test_block in order (resblock_part, nbe_engine_net.cpp:183-223; upblock :294-315; downblock);
    form: a letter of FORMS or a Form(prec, vel, wino)"""
    f = _form(form)
    D, H, W, pad = shape
    if block.startswith('down'):
        L = layer(block, "conv_0", mid)
        k = "mfma" if f.prec == "f32" else "h3_down"
        return [Launch("conv_0", k, label(k, f, L, True), (D // 2, H // 2, W // 2), mid, mid, 0, None, False)]
    if block.startswith('up'):
        L = layer(block, "conv_0", mid)
        if up8_launch(mid, f):
            return [Launch("conv_0", "up8", label("up8", f, L, True), (D, H, W), mid, mid, 0, None, False)]
        k = "mfma" if f.prec == "f32" else "h3_flat1"
        return [Launch("conv_0", k, label(k, f, L, True), (D, H, W), mid, mid, 0, None, False)] * 8
    sy = 0 if pad else 2
    nres = D - 4
    fused = expect_fused(block, mid, f.prec, f.vel, gauge, nres, f.wino)
    two = src == "two"
    assert not two or (fused and block in B.DECODERS and two_source_width(mid, f.prec))
    L0, L1, Ls = (layer(block, n, mid) for n in ("conv_0", "conv_1", "skip"))
    has_dx = block != 'conv_l00'
    dv0, dv1 = (D - 2, H - sy, W - sy), (nres, H - 2 * sy, W - 2 * sy)
    split = mid // CHUNK if two else None
    out = []
    if not fused:
        k = "mfma" if f.prec == "f32" else "h3_flat1"
        out.append(Launch("skip", k, label(k, f, Ls, has_dx), dv1, Ls.cin, Ls.cout, 0, None, False))
    k = select3(f, mid, L0, dv0[0], has_dx, gauge, f.wino, two=two)
    out.append(Launch("conv_0", k, label(k, f, L0, has_dx), dv0, L0.cin, L0.cout, 0, split, False))
    k = select3(f, mid, L1, dv1[0], True, gauge, f.wino, res=not fused, skip=Ls if fused else None, s_two=two)
    out.append(Launch("conv_1", k, label(k, f, L1, True), dv1, L1.cin, L1.cout, nchunk(Ls.cin) if fused else 0, split if fused else None,
                      not fused))
    assert all(la.kernel != "none" for la in out), (block, mid, form, shape, out)
    return out


def labels(block, mid, form, shape, gauge=True):
    """{profile label: launches} of one run_case call: a residual block once per source form, an up_* block twice (into a
    tensor of its own and into the second half of a concat tensor), a down_* block once"""
    n = collections.Counter()
    if block not in RES:
        for la in launches(block, mid, form, shape, "cat", gauge):
            n[la.label] += 2 if block.startswith('up') else 1
        return dict(n)
    for src in sources(block, mid, form, shape, gauge):
        for la in launches(block, mid, form, shape, src, gauge):
            n[la.label] += 1
    return dict(n)


def paths(block, mid, form, shape, src="cat", gauge=True):
    """the exact path word of nbe_test_block (run_conv, nbe_engine_net.cpp:110-114)"""
    p = set()
    for la in launches(block, mid, form, shape, src, gauge):
        if la.nskip:
            p.add("skip_fused")
            if block == 'conv_l00':
                p.add("skip_nodx")
            if la.split is not None:
                p.add("two_source_skip")
        if la.layer == "conv_0" and la.split is not None:
            p.add("two_source")
        if la.kernel.startswith("h3w"):
            p.add("wino_1" if la.layer == "conv_1" else "wino_0")
        if la.kernel in ("h3g_narrow", "h3nz"):
            p.add("narrow")
        if la.kernel == "up8":
            p.add("up8")
    return p


# ---- the shapes --------------------------------------------------------------------------------------------------------------------
def shapes(block, form):
    """[(D, H, W, pad)] of the block input.  Residual blocks: 2 and 3 result planes of 9 x 33 (one row and one column into the
    last tiles; an even plane count is what the Winograd-z kernel needs, an odd one what takes every launch off it) and for the
    level-0 blocks 2 planes periodic in y and x.  The g form is the w form under NBE_WINO=0: no launch of an odd plane count has
    a Winograd-z form, so it runs the even shapes only.  up_* / down_*: the smallest of test_gpu_blocks.shapes (k = 13), and a
    small periodic one at level 0."""
    lvl0 = B.LEVEL[block] == 0
    if block.startswith('down'):
        return [(2, B.input_size(block, 13), B.input_size(block, 13), 0)] + ([(2, 16, 24, 1)] if lvl0 else [])
    if block.startswith('up'):
        return [(1, B.input_size(block, 13), B.input_size(block, 13), 0)] + ([(1, 8, 12, 1)] if lvl0 else [])
    out = [(6, 13, 37, 0)] + ([] if form == "g" else [(7, 13, 37, 0)])
    return out + ([(6, 9, 33, 1)] if lvl0 else [])


# (mid, block, form) of the parity matrix
MATRIX = [(mid, b, f) for mid in WIDTHS for b in BLOCKS_OF[mid] for f in FORMS_OF[mid]]


def walk_rows(block, mid, form, shape, src="cat", gauge=True):
    """[(launch, case line of tools/conv_select_walk.hip)] of the launches of a block: what launch_conv hands conv_select"""
    f = _form(form)
    ga = gauge_active(mid, f, gauge)
    wok = wino_ok(mid, f, gauge, f.wino)
    out = []
    for la in launches(block, mid, form, shape, src, gauge):
        L = layer(block, la.layer, mid)
        has_dx = la.layer == "conv_1" or block != 'conv_l00'
        kv = ["prec=%s" % f.prec, "vel=%d" % f.vel, "dx=%d" % has_dx, "cin=%d" % L.cin, "cout=%d" % L.cout, "Dv=%d" % la.dv[0]]
        if f.prec == "f32":
            kv.append("ni=%d" % (2 if L.cout > 32 else 1))
        if L.kind != "conv3":
            kv.append("mode=%s" % ("down" if L.kind == "down" else "flat1"))
            if L.kind == "up":
                kv += ["osz=2"] + (["up8=1"] if la.kernel == "up8" else [])
            out.append((la, " ".join(kv)))
            continue
        beta = ga and L.g6 and has_dx
        narrow = beta and packs_narrow(f, L)
        if narrow:
            kv += ["cout_t=16", "ctiles=1"]
        if beta:
            kv.append("beta=1")
        if wok and not narrow and packs_wino(f, L):
            kv.append("ww=1")
        if packs_stem(f, L):
            kv.append("stem=1")
        if la.res:
            kv.append("res=1")
        if la.nskip:
            Ls = layer(block, "skip", mid)
            kv.append("skip=%d" % pad16(Ls.cin))
            if wok and packs_wino_skip(f, Ls):
                kv.append("wws=1")
            if Ls.first:
                kv.append("nodx=1")
            if la.split is not None:
                kv.append("s_csplit=%d" % (la.split * CHUNK))
        if la.layer == "conv_0" and la.split is not None:
            kv.append("csplit=%d" % (la.split * CHUNK))
        out.append((la, " ".join(kv)))
    return out
