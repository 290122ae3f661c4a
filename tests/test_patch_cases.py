"""The case table of tests/patch_cases.py held to its purpose: every tile edge of the 3x3x3 patch kernels and of the
Winograd-z kernel that the table was chosen for is named here, so that the table cannot be thinned out unnoticed.  CPU only:
the tiling is the restatement in patch_cases.py, the oracle is evaluated on every case (both of its backends)."""

import collections

import numpy as np
import pytest

import patch_cases as P
from oracle import layers as L

GAUGED, DIRECT = P.BASE_FORMS
NOVEL = P.Form("f16x3", "novel", True)
F16G = P.Form("f16", "gauged", True)


def _launches(case):
    """[(form, kernel, tiling)] of the patch-kernel launches of a case"""
    out = []
    for f in P.forms(case):
        k = P.select(f, case.cin, case.dv, case.res)[0]
        if k in P.KERNELS:
            out.append((f, k, P.tiling(k, case.dv, case.cout)))
    return out


def test_names_are_unique_and_every_case_says_why():
    names = [c.name for c in P.CASES]
    assert len(set(names)) == len(names)
    assert all(len(c.why) > 5 for c in P.CASES)
    assert all(8 <= c.cin <= 128 for c in P.CASES)               # the per-layer classes hold for K <= 27 * 128 + 128
    assert not any(c.rep and c.res for c in P.CASES)


def test_table_holds_the_row_and_column_edges():
    two = {c.dv[1:] for c in P.CASES if c.dv[0] == 2}
    assert two >= {(1, 1), (7, 31), (8, 32), (9, 33), (15, 17), (16, 16), (17, 15), (8, 65), (25, 32)}
    assert {h for h, _ in two} >= {7, 8, 9, 15, 16, 17} and {w for _, w in two} >= {15, 16, 17, 31, 32, 33}
    assert {c.dv for c in P.CASES} >= {(1, 9, 33), (3, 9, 33)}
    for c in P.CASES:
        if c.dv[0] == 2 and c.dv[1:] in ((1, 1), (7, 31), (8, 32), (9, 33), (15, 17), (16, 16), (17, 15), (8, 65), (25, 32)):
            assert (c.cin, c.cout) == (16, 24) or c.name.startswith(("nct", "cout")) or c.name.endswith("-c32")
    tl = lambda name, k: P.tiling(k, P.BY_NAME[name].dv, P.BY_NAME[name].cout)
    assert tl("e8x65", "h3w_f16x3").tnx == 3 and tl("e25x32", "h3w_f16x3").tny == 4
    assert (tl("e9x33", "h3w_f16x3").ntiles, tl("e9x33", "h3g_wide").ntiles) == (4, 8)
    # the second row block of the displacement-only form: wholly masked, partly used, whole, and one row of a second tile
    used = lambda name: [P.second_block_rows(16 * ty, P.BY_NAME[name].dv[1]) for ty in range(tl(name, "h3w_novel").tny)]
    assert used("e8x32") == [0] and used("e7x31") == [0] and used("e9x33") == [1] and used("e15x17") == [7]
    assert used("e16x16") == [8] and used("e17x15") == [8, 0] and used("e25x32") == [8, 1]
    assert {c.name for c in P.CASES if c.rep} >= {"e8x32", "e9x33", "e17x15", "e25x32", "z16", "z18", "z22", "z34",
                                                 "grid7", "grid9", "cout72-2t", "cin48", "cin128"}


def test_table_holds_the_tile_orders():
    """rem 1 and 3, two whole blocks, and the remainder-branch tiles of each: the figures of DESIGN.md section 2c"""
    want = {  # name: (8-row tiles, their grid, remainder tiles; 16-row tiles, remainder tiles; direct 8-row tiles)
        "z16": (32, 32, 0, 16, 0, 16 * 2 * 2), "z18": (36, 72, 4, 18, 2, 18 * 2 * 2),
        "z22": (66, 66, 18, 44, 12, 22 * 3 * 2), "z34": (102, 102, 6, 51, 3, 34 * 2 * 3)}
    rems, blocks = set(), set()
    for name, (nt8, grid8, rem8, nt16, rem16, ntd) in want.items():
        c = P.BY_NAME[name]
        t8, t16 = P.tiling("h3w_f16x3", c.dv, c.cout), P.tiling("h3w_novel", c.dv, c.cout)
        assert (t8.ntiles, t8.grid, t8.remainder, t16.ntiles, t16.remainder) == (nt8, grid8, rem8, nt16, rem16), name
        assert P.tiling("h3g_wide", c.dv, c.cout).ntiles == ntd
        assert P.select(GAUGED, c.cin, c.dv)[0] == "h3w_f16x3" and P.select(NOVEL, c.cin, c.dv)[0] == "h3w_novel"
        npair = c.dv[0] // 2
        rems.add(npair % P.zblock(c.dv[0]))
        blocks.add(npair // P.zblock(c.dv[0]))
    assert rems >= {0, 1, 3} and blocks >= {1, 2}
    z22, z34, z18 = P.BY_NAME["z22"], P.BY_NAME["z34"], P.BY_NAME["z18"]
    assert P.tiling("h3w_f16x3", z22.dv, 64).grid & 7 == 2 and P.tiling("h3w_novel", z22.dv, 64).grid & 7 == 4
    assert P.tiling("h3w_f16x3", z34.dv, 24).grid & 7 == 6
    assert P.tiling("h3w_f16x3", z18.dv, z18.cout).nct == 2          # the remainder branch beside two cout tiles
    assert (z18.cin, z22.cin, z22.cout) == (64, 64, 64)


def test_table_holds_the_grids():
    wino, direct = set(), set()
    for c in P.CASES:
        for f, k, t in _launches(c):
            (wino if k.startswith("h3w") else direct).add(t.grid)
    assert wino >= {1, 7, 8, 9, 15, 17} and direct >= {1, 7, 8, 9, 15, 17}
    g = lambda name, k: P.tiling(k, P.BY_NAME[name].dv, P.BY_NAME[name].cout).grid
    assert [g(n, "h3w_f16x3") for n in ("e1x1", "grid7", "cin16", "grid9", "grid15", "grid17")] == [1, 7, 8, 9, 15, 17]
    assert [g(n, "h3g_wide") for n in ("d-grid1", "d-grid7", "e9x33", "d-grid9", "d-grid15", "d-grid17")] == [1, 7, 8, 9, 15, 17]
    # two cout tiles with an odd number of tiles, on the Winograd-z and on the direct kernels
    odd = [(k, t) for c in P.CASES for _, k, t in _launches(c) if t.nct == 2 and t.ntiles % 2 == 1]
    assert any(k.startswith("h3w") for k, _ in odd) and any(not k.startswith("h3w") for k, _ in odd)
    # a second cout tile of one whole and of one ragged channel group, on a two-tile shape
    two = {c.cout for c in P.CASES if P.tiling("h3w_f16x3", c.dv, c.cout).ntiles == 2 and c.dv[0] == 2}
    assert two >= {68, 72} and P.cout_groups(68) == P.cout_groups(72) == 9 and P.nct(64) == 1 and P.nct(65) == 2


def test_table_holds_the_channel_counts():
    at = {(c.cin, c.cout) for c in P.CASES if c.dv == (4, 9, 33)}
    assert at >= {(ci, 64) for ci in (8, 16, 24, 48, 64, 96, 128)} | {(64, co) for co in (3, 8, 24, 64, 68, 128)} | {(128, 128)}
    assert 4 * P.nchunk(128) == P.MAX_WSTAGES and any(c.cin == 128 and c.rep for c in P.CASES)
    # every chunk count on the kernel whose stage table it fills, counted over the launches select() maps to that kernel:
    # conv_h3w f16x3 runs 4 stages per chunk, the float16 form one stage per two chunks
    chunks = collections.defaultdict(set)
    for c in P.CASES:
        for f in P.forms(c):
            chunks[P.select(f, c.cin, c.dv, c.res)[0]].add(P.nchunk(c.cin))
    assert chunks["h3w_f16x3"] >= {1, 2, 3, 4, 6, 8} and chunks["h3g_wide"] >= {1, 2, 3, 4, 6, 8}
    assert chunks["h3w_novel"] >= {1, 3, 6, 8} and chunks["h3q"] >= {1, 3, 6, 8}
    stages = {n // P.F16_CHUNKS for n in chunks["h3w_f16"]}
    assert all(n % P.F16_CHUNKS == 0 for n in chunks["h3w_f16"]) and stages >= {1, 2, 3, 4}
    assert {n % 2 for n in chunks["h2q_f16_g"]} == {0, 1}          # odd counts by refusal, even ones under NBE_WINO=0
    # the float16 Winograd-z form at a ragged tile, a fourth tile row and two blocks of the tile order
    f16w = {c.dv for c in P.CASES if F16G in P.forms(c) and P.select(F16G, c.cin, c.dv, c.res)[0] == "h3w_f16"}
    assert f16w >= {(2, 9, 33), (2, 25, 32), (34, 9, 65), (22, 17, 33), (18, 9, 33)}
    # an odd chunk count: the float16 gauged launch goes to conv_h2q_kernel<false, true>, an even one to conv_h3w
    f16 = {c.name: P.select(F16G, c.cin, c.dv, c.res)[0] for c in P.CASES if F16G in P.forms(c)}
    assert f16["cin48"] == "h2q_f16_g" and f16["e9x33"] == "h2q_f16_g" and f16["cin128"] == "h3w_f16" and f16["z22"] == "h3w_f16"
    assert sum(1 for c in P.CASES if not c.act) >= 2 and sum(1 for c in P.CASES if c.res) >= 3
    res = [c for c in P.CASES if c.res]
    assert any(P.select(F16G, c.cin, c.dv, True)[0] == "h3w_f16" for c in res)
    assert all(P.select(F16G._replace(wino=False), c.cin, c.dv, True)[0] == "h2q_f16_g" for c in res)
    assert all(P.select(GAUGED, c.cin, c.dv, True)[0] == "h3g_wide" for c in res)    # the f16x3 Winograd-z form has no residual


def test_every_patch_kernel_is_reached_and_odd_plane_counts_stay_direct():
    ran = collections.Counter(P.select(f, c.cin, c.dv, c.res)[0] for c in P.CASES for f in P.forms(c))
    assert set(ran) == set(P.KERNELS) | {"mfma", "mfma_g"}, ran
    for c in P.CASES:
        if c.dv[0] % 2:
            assert {P.select(f, c.cin, c.dv, c.res)[0] for f in P.forms(c)} == {"h3g_wide"}
        fs = P.forms(c)
        assert GAUGED in fs and (DIRECT in fs) == (P.select(GAUGED, c.cin, c.dv, c.res)[0] == "h3w_f16x3")
        if c.rep:
            assert {P.select(f, c.cin, c.dv)[0] for f in fs} >= {"h3w_f16x3", "h3g_wide", "h3q", "h3w_novel", "h2q_split",
                                                                 "h2q_f16", "h3p", "mfma", "mfma_g"}


def test_selection_follows_conv_select():
    s = lambda prec, tangent, wino, cin, dv, res=False: P.select(P.Form(prec, tangent, wino), cin, dv, res)[0]
    assert s("f16x3", "gauged", True, 128, (2, 1, 1)) == "h3w_f16x3" and s("f16x3", "gauged", False, 128, (2, 1, 1)) == "h3g_wide"
    assert s("f16x3", "gauged", True, 64, (3, 1, 1)) == "h3g_wide" and s("f16x3", "gauged", True, 64, (2, 1, 1), True) == "h3g_wide"
    assert s("f16x3", "novel", True, 64, (2, 1, 1)) == "h3w_novel" and s("f16x3", "novel", True, 64, (5, 1, 1)) == "h2q_split"
    assert s("f16x3", "vel", True, 64, (2, 1, 1)) == "h3q"        # the hook packs no Winograd-z form for a plain tangent
    assert s("f16", "gauged", True, 32, (2, 1, 1)) == "h3w_f16" and s("f16", "gauged", True, 32, (2, 1, 1), True) == "h3w_f16"
    assert s("f16", "gauged", True, 16, (2, 1, 1)) == "h2q_f16_g" and s("f16", "gauged", True, 32, (1, 1, 1)) == "h2q_f16_g"
    assert s("f16", "vel", True, 32, (2, 1, 1)) == "h2q_f16" and s("f16", "novel", True, 32, (2, 1, 1)) == "h3p"
    assert P.select(P.Form("f32", "gauged", True), 16, (2, 1, 1))[1].startswith("conv_mfma_g<")


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_restated_decodes_are_bijections(case):
    """every (plane or plane pair, ty, tx, cout tile) exactly once, for every kernel geometry, whichever form runs the case"""
    for k, g in P.KERNELS.items():
        if g.pairs and case.dv[0] % 2:
            continue
        t = P.tiling(k, case.dv, case.cout)
        nz = case.dv[0] // g.zper
        got = P.walk(k, case.dv, case.cout)
        want = {(z, ty, tx, ct) for z in range(nz) for ty in range(t.tny) for tx in range(t.tnx) for ct in range(t.nct)}
        assert len(got) == len(want) == t.ntiles * t.nct and set(got) == want, (case.name, k)
        # every output row and column lies in exactly one tile
        assert (t.tny - 1) * t.rows < case.dv[1] <= t.tny * t.rows and (t.tnx - 1) * P.HP_COLS < case.dv[2] <= t.tnx * P.HP_COLS
        if g.pairs:
            tiles = [P.decode_pairs(i, case.dv[0], t.tny, t.tnx) for i in range(t.ntiles)]
            assert sum(1 for p in tiles if p[3]) == t.remainder == (nz % P.zblock(case.dv[0])) * t.tny * t.tnx
            assert all((zp >= nz - nz % P.zblock(case.dv[0])) == rem for zp, _, _, rem in tiles)


@pytest.mark.parametrize("case", P.CASES, ids=[c.name for c in P.CASES])
def test_oracle_evaluates_the_case_and_its_backends_agree(case):
    o = P.operands(case)
    x, dx, w, dw, b = (a.astype(np.float64) for a in (o.x, o.dx, o.w, o.dw, o.b))
    assert np.allclose((w ** 2).sum(axis=(1, 2, 3, 4)), 1.0, rtol=1e-6)
    y, dy = L.conv_layer_vel("conv3", x, dx, w, dw, b)
    with L.backend('torch'):
        yt, dyt = L.conv_layer_vel("conv3", x, dx, w, dw, b)
    assert y.shape == dy.shape == (case.cout,) + case.dv
    assert np.all(np.isfinite(y)) and np.all(np.isfinite(dy))
    rms = lambda a: float(np.sqrt(np.mean(a ** 2)))
    assert np.abs(y - yt).max() <= 1e-12 * rms(y) and np.abs(dy - dyt).max() <= 1e-12 * rms(dy)
    assert np.array_equal(L.conv_layer("conv3", x, w, b), y)
    assert (o.r is not None) == case.res and (o.r is None or o.r.shape == y.shape)
