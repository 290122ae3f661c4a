"""The case table of tests/fused_cases.py held to its purpose: every tile edge that the fused conv_1 + skip launches (and the
conv_0 launches in front of them) were to be taken to is named here, so that the table cannot be thinned out unnoticed.  CPU
only: the tiling is the restatement of patch_cases.py, the fusing rule is compared with test_gpu_blocks.expect_fused, and the
block oracle is evaluated on one small case per block (both of its backends)."""

import collections

import numpy as np
import pytest

import block_ref as B
import fused_cases as F
import test_gpu_blocks as TB
from oracle import layers as L

ROWS, COLS = {7, 8, 9, 15, 16, 17}, {31, 32, 33, 63, 64, 65}
ROWS_N = ROWS | {23, 24, 25}
GRID_SIZES = {1, 7, 8, 9, 15, 17}


def _all(layer):
    """{form: [(case, launch, tiling)]} of the given layer's patch-kernel launches, both sources of a two-source case"""
    out = collections.defaultdict(list)
    for c, f in F.PARITY:
        for src in F.sources(c, f):
            la = F.launches(c, f, src)[layer]
            if la.kernel != "stem":
                out[f].append((c, la, F.launch_tiling(la)))
    return out


def test_names_are_unique_and_every_case_says_why():
    names = [c.name for c in F.CASES]
    assert len(set(names)) == len(names) and all(len(c.why) > 5 for c in F.CASES)
    for c in F.CASES:
        assert set(c.forms) <= set(F.ALL) and ("w" in c.forms or "g" in c.forms), c.name
        assert ("w" in c.forms) == (c.dv[0] % 2 == 0), c.name            # an odd plane count is the g form of the same operands
        assert c.dv[0] % 2 == 0 or c.forms == "g", c.name
        assert not c.pad or B.LEVEL[c.block] == 0, c.name                # periodic yx exists at level 0 only
        assert "h" not in c.forms or (c.mid in (32, 64) and c.block != "conv_l00"), c.name
        D, H, W, pad = F.shape(c)
        assert D >= 5 and B.channels(c.block, c.mid)[1] <= 128          # the per-layer classes hold for K <= 27 * 128 + 128
    assert len(F.PARITY) == sum(len(c.forms) for c in F.CASES)


def test_kernels_and_labels_of_every_launch():
    """the four instantiations, where the table says they run"""
    want = {"w": "h3w_f16x3", "g": "h3g_wide", "n": "h3w_novel", "h": "h3w_f16"}
    for c, f in F.PARITY:
        for src in F.sources(c, f):
            c0, c1 = F.launches(c, f, src)
            assert c1.kernel == want[f] and c1.nskip > 0, (c.name, f)
            assert c0.kernel == ("stem" if c.block == "conv_l00" else want[f]), (c.name, f)
            assert (c0.dv[0], c1.dv[0]) == (c.dv[0] + 2, c.dv[0])
            assert c0.dv[1:] == (c.dv[1:] if c.pad else (c.dv[1] + 2, c.dv[2] + 2))
            assert F.paths(c, f, src) >= {"skip_fused"} and ("wino_1" in F.paths(c, f, src)) == (f != "g")
        lab = F.labels(c, f)
        assert sum(lab.values()) == 2 * len(F.sources(c, f)) and len(lab) == (2 if c.block == "conv_l00" else 1), (c.name, f)
    m = lambda name, f, src="cat": F.launches(F.BY_NAME[name], f, src)[1]
    # the chunk loop of the skip: nskip 1, 2, 4, 8; the switch at 1 and at 4 (float16: stages 2, 4, switching at 2)
    assert [m(n, "w").nskip for n in ("l00-m64", "r00-m16", "l01-m24", "l01-m64", "r00-m64")] == [1, 2, 2, 4, 8]
    assert (m("r00-m16", "w", "two").split, m("r00-m64", "w", "two").split, m("r00-m64", "n", "two").split) == (1, 4, 4)
    assert (m("l01-m64", "h").nskip, m("r00-m64", "h").nskip, m("r00-m64", "h", "two").split) == (2, 4, 2)
    assert m("r00-m16", "w").cout == 16 and m("l01-m24", "w").cout == 24 and F.nct(16) == F.nct(64) == 1
    assert F.paths(F.BY_NAME["l00-m64"], "w", "cat") == {"skip_fused", "skip_nodx", "wino_1"}
    assert F.paths(F.BY_NAME["r00-m64"], "g", "two") == {"skip_fused", "two_source", "two_source_skip"}
    assert F.paths(F.BY_NAME["r00-m64"], "h", "two") == {"skip_fused", "two_source", "two_source_skip", "wino_0", "wino_1"}
    assert F.labels(F.BY_NAME["l00-m64"], "n") == {"stem_h3<FLAT3,novel>": 1, "conv_h3w<FLAT3,novel>": 1}
    assert F.labels(F.BY_NAME["r00-m64"], "w") == {"conv_h3w<FLAT3,vel,dx>": 4}
    assert F.labels(F.BY_NAME["z17"], "g") == {"conv_h3g<FLAT3,vel,dx>": 2}
    for name in ("r00-m64", "r00-m16", "p9x33", "r00-m16-z18"):
        c = F.BY_NAME[name]
        assert all(F.sources(c, f) == ("cat", "two") for f in c.forms), name


@pytest.mark.parametrize("layer", [1, 0], ids=["conv_1", "conv_0"])
def test_table_holds_the_row_and_column_edges(layer):
    """every listed extent in every form, for the launch's OWN extents (conv_0: the hidden tensor's)"""
    per = _all(layer)
    for f in F.ALL:
        rows, cols = {la.dv[1] for _, la, _ in per[f]}, {la.dv[2] for _, la, _ in per[f]}
        assert rows >= (ROWS_N if f == "n" else ROWS) and cols >= COLS, (f, sorted(rows), sorted(cols))
        # extents of exactly one tile, and the tile counts at the edges
        one = 16 if f == "n" else 8
        assert any(la.dv[1:] == (one, 32) and t.tny == t.tnx == 1 for _, la, t in per[f]), f
        assert {t.tnx for _, _, t in per[f]} >= {1, 2, 3} and {t.tny for _, _, t in per[f]} >= {1, 2}
    if layer == 1:
        # the hidden tensor on a tile edge where the result is not
        for f in F.ALL:
            for name, hid in (("e6x30", (8, 32)), ("e14x62", (16, 64))):
                c0, c1 = F.launches(F.BY_NAME[name], f)
                assert c0.dv[1:] == hid and c1.dv[1] % 8 and c1.dv[2] % 32
        # periodic: both launches on the result's extents
        for name, f, ext in (("p8x32", "w", (8, 32)), ("p9x33", "h", (9, 33)), ("p16x64", "n", (16, 64)), ("p8x32", "g", (8, 32))):
            c0, c1 = F.launches(F.BY_NAME[name], f)
            assert c0.dv[1:] == c1.dv[1:] == ext and F.shape(F.BY_NAME[name])[1:] == ext + (1,)
        assert F.launch_tiling(F.launches(F.BY_NAME["p16x64"], "n")[1])[1:4] == (1, 2, 2)


def test_second_row_block_of_the_displacement_only_form():
    """ook2: rows of the second block stored per tile row, in conv_1 and in conv_0"""
    for layer, need in ((1, {0, 1, 7, 8}), (0, {0, 1, 7, 8})):
        seen = collections.defaultdict(set)
        for c, la, t in _all(layer)["n"]:
            assert t.rows == 16
            for ty in range(t.tny):
                seen[F.second_block_rows(16 * ty, la.dv[1])].add(c.name)
        assert set(seen) >= need, (layer, sorted(seen))
    used = lambda name: [F.second_block_rows(16 * ty, F.BY_NAME[name].dv[1]) for ty in range(F.tiles_of(F.BY_NAME[name].dv[1], 16))]
    assert used("e8x32") == [0] and used("e9x33") == [1] and used("e15x63") == [7] and used("e16x64") == [8]
    assert used("e23x31") == [8, 0] and used("e24x32") == [8, 0] and used("e25x33") == [8, 1] and used("e17x65") == [8, 0]
    assert all("n" in F.BY_NAME[n].forms for n in ("e8x32", "e9x33", "e15x63", "e16x64", "e23x31", "e24x32", "e25x33"))


def _branches(la):
    """(whole-block tiles with blk > 0, remainder-branch tiles, remainder pairs) of a conv_h3w launch"""
    t = F.launch_tiling(la)
    zb = F.zblock(la.dv[0])
    per_blk = zb * t.tny * t.tnx
    places = [F.decode_pairs(i, la.dv[0], t.tny, t.tnx) for i in range(t.ntiles)]
    later = sum(1 for i, p in enumerate(places) if not p[3] and i >= per_blk)
    return later, sum(1 for p in places if p[3]), (la.dv[0] // 2) % zb


def test_table_holds_the_plane_counts_and_the_branches_of_the_tile_decode():
    for layer in (1, 0):
        per = _all(layer)
        for f in "wnh":
            planes = {la.dv[0] for _, la, _ in per[f]}
            assert planes >= ({2, 4, 16, 18, 22, 32} if layer else {4, 16, 18, 22, 32}), (layer, f, sorted(planes))
        g = {la.dv[0] for _, la, _ in per["g"]}
        assert g >= ({2, 4, 16, 18, 22, 32, 3, 17} if layer else {4, 16, 18, 22, 32, 5, 19}), (layer, sorted(g))
    # (tiles of whole blocks behind the first, remainder tiles, remainder pairs) per launch: 2 x 2 tiles per pair (1 x 2 for n)
    want = {"z16": ((0, 4, 1), (0, 0, 0)), "z18": ((0, 8, 2), (0, 4, 1)), "z22": ((0, 16, 4), (0, 12, 3)),
            "z32": ((32, 4, 1), (32, 0, 0))}
    for name, (b0, b1) in want.items():
        c = F.BY_NAME[name]
        assert set(c.forms) == set(F.ALL)
        for f in "wh":
            c0, c1 = F.launches(c, f)
            assert (_branches(c0), _branches(c1)) == (b0, b1), (name, f)
        half = lambda b: (b[0] // 2, b[1] // 2, b[2])
        c0, c1 = F.launches(c, "n")
        assert (_branches(c0), _branches(c1)) == (half(b0), half(b1)), name
        assert F.zblock(c1.dv[0]) == F.zblock(c0.dv[0]) == 8
    for name, b0 in (("z14", (0, 0, 0)), ("z20", (0, 12, 3)), ("z30", (32, 0, 0))):
        assert _branches(F.launches(F.BY_NAME[name], "w")[0]) == b0, name
    c0, c1 = F.launches(F.BY_NAME["r00-m16-z18"], "w", "two")
    assert _branches(c1) == (0, 4, 1) and c1.split == 1
    assert _branches(F.launches(F.BY_NAME["grid17"], "w")[1]) == (8, 1, 1)       # 17 pairs of one tile: two blocks and one pair
    # odd plane counts: no launch of the block has a Winograd-z form, NBE_WINO is left alone
    for name in ("z3", "z17"):
        c = F.BY_NAME[name]
        assert F.wino_env(c, "g") and [la.kernel for la in F.launches(c, "g")] == ["h3g_wide", "h3g_wide"]
        assert [la.dv[0] % 2 for la in F.launches(c, "g")] == [1, 1]
    assert not F.wino_env(F.BY_NAME["z16"], "g")


def test_table_holds_the_grids():
    per = _all(1)
    for f in F.ALL:
        grids = {t.grid for _, _, t in per[f]}
        assert grids >= GRID_SIZES, (f, sorted(grids))
    g = lambda name, f: F.launch_tiling(F.launches(F.BY_NAME[name], f)[1]).grid
    assert [g(n, "w") for n in ("e8x32", "grid7", "l01-m64", "grid9", "grid15", "grid17")] == [1, 7, 8, 9, 15, 17]
    assert [g(n, "h") for n in ("e8x32", "grid7", "l01-m64", "grid9", "grid15", "grid17")] == [1, 7, 8, 9, 15, 17]
    assert [g(n, "n") for n in ("e16x32", "grid7", "n-grid8", "n-grid9", "n-grid15", "grid17")] == [1, 7, 8, 9, 15, 17]
    assert [g(n, "g") for n in ("g-grid1", "g-grid7", "e9x33", "g-grid9", "g-grid15", "g-grid17")] == [1, 7, 8, 9, 15, 17]


@pytest.mark.parametrize("case", F.CASES, ids=[c.name for c in F.CASES])
def test_restated_decodes_are_bijections(case):
    """decode_pairs (decode_z) composed with xcd_tile visits every (plane pair or plane, ty, tx, cout tile) exactly once, in
    both launches of every form; every result row and column lies in exactly one tile"""
    for f in case.forms:
        for la in F.launches(case, f):
            t = F.launch_tiling(la)
            if t is None:
                continue
            pairs = la.kernel.startswith("h3w")
            nz = la.dv[0] // (2 if pairs else 1)
            got = F.walk(la.kernel, la.dv, la.cout)
            want = {(z, ty, tx, ct) for z in range(nz) for ty in range(t.tny) for tx in range(t.tnx) for ct in range(t.nct)}
            assert len(got) == len(want) == t.grid and set(got) == want, (case.name, f, la.layer)
            assert (t.tny - 1) * t.rows < la.dv[1] <= t.tny * t.rows and (t.tnx - 1) * F.HP_COLS < la.dv[2] <= t.tnx * F.HP_COLS
            assert sorted(F.xcd_tile(b, t.grid) for b in range(t.grid)) == list(range(t.grid))


def test_restated_fusing_rule_agrees_with_expect_fused():
    for c in F.CASES:
        for f, form in F.FORMS.items():
            for wino_on in (True, False):
                if f == "g" and wino_on and c.dv[0] % 2 == 0:
                    continue                                             # the g form of an even plane count is NBE_WINO=0
                mine = F.fused(c, f) if wino_on == F.wino_env(c, f) else None
                if mine is None:
                    continue
                assert mine == TB.expect_fused(c.block, c.mid, form.prec, form.vel, True, c.dv[0], wino_on), (c.name, f)
    assert all(F.fused(c, f) for c, f in F.PARITY)                       # every (case, form) of the table is a fused launch
    # and the forms a case leaves out where the block does not fuse there
    assert not F.fused(F.BY_NAME["l00-m64"], "h") and not F.fused(F.BY_NAME["r00-m16"]._replace(mid=8), "h")
    assert not F.fused(F.BY_NAME["z17"]._replace(forms="n"), "n")


ORACLE = [("conv_l00", 64, (5, 5, 7, 0)), ("conv_l01", 24, (6, 5, 6, 0)), ("conv_r00", 16, (6, 6, 5, 0)), ("conv_l01", 16, (5, 3, 4, 1)),
          ("conv_r00", 16, (6, 3, 3, 1))]


@pytest.mark.parametrize("block,mid,shape", ORACLE, ids=["%s-m%d-pad%d" % (b, m, s[3]) for b, m, s in ORACLE])
def test_block_oracle_evaluates_the_smallest_shapes_and_its_backends_agree(block, mid, shape):
    """stage1 / stage2 on the smallest inputs the hook takes (one result plane; one result row where periodic), for every
    block of the table and both paddings, with velocity and without, float32 and float16 operand rounding"""
    assert {b for b, _, _ in ORACLE} == {c.block for c in F.CASES}
    D, H, W, pad = shape
    sy = 0 if pad else 2
    p, s = TB.params_of(mid), TB.s64()
    g = B.gauges(p, s, block, mid)
    for half in (False, True):
        x, dxs = TB.make_input(block, mid, "f16" if half else "f16x3", True, shape, g[0])
        x, dxs = x.astype(np.float64), None if dxs is None else dxs.astype(np.float64)
        res = {}
        for be in ("numpy", "torch"):
            with L.backend(be):
                S1 = B.stage1(p, s, block, x, dxs, mid, pad=pad, half=half)
                h, dh = S1.result()
                S2 = B.stage2(p, s, block, x, dxs, h, dh, mid, pad=pad, half=half)
                res[be] = (h, dh) + S2.result()
                yd, _ = B.stage2(p, s, block, x, None, h, None, mid, pad=pad, vel=False, half=half).result()
                assert np.array_equal(yd, res[be][2])
        cmid, cout = B.channels(block, mid)[1:]
        assert res["numpy"][0].shape == (cmid, D - 2, H - sy, W - sy) and res["numpy"][2].shape == (cout, D - 4, H - 2 * sy, W - 2 * sy)
        for a, b in zip(res["numpy"], res["torch"]):
            assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 1e-12 * float(np.sqrt(np.mean(a ** 2)))
