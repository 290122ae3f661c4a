"""The table of tests/wide_cases.py held to its purpose on the CPU: every limit above width 64 that the widths were chosen for is
named here, so that the table cannot be thinned out unnoticed; every launch of the table is walked through conv_select itself
(tools/conv_select_walk.hip); the rows that overlap tests/test_conv_select.py agree with it; and the generalised fusing rule is
test_gpu_blocks.expect_fused wherever that one is defined (mid <= 64)."""

import itertools
import os
import subprocess

import numpy as np
import pytest

import block_ref as B
import test_conv_select as CS
import test_gpu_blocks as TB
import wide_cases as W
from oracle import layers as L

X3V, X3G, X3N, H1V, F32 = (W.FORMS[f] for f in "wgnhs")
EVEN, ODD = (6, 13, 37, 0), (7, 13, 37, 0)


def la(block, mid, form, shape=EVEN, src="cat"):
    return W.launches(block, mid, form, shape, src)


def test_every_width_says_why_and_the_matrix_is_what_the_issue_lists():
    assert list(W.WIDTHS) == [72, 80, 96, 128, 136, 176] and all(len(w) > 20 for w in W.WIDTHS.values())
    assert len(set(W.MATRIX)) == len(W.MATRIX)
    for mid in (72, 128):
        assert W.BLOCKS_OF[mid] == B.BLOCKS and W.FORMS_OF[mid] == "wgnhs"
    for mid in (80, 136, 176):
        assert set(W.BLOCKS_OF[mid]) == set(B.DECODERS) | {'conv_r01', 'conv_l01', 'up_r1'} and W.FORMS_OF[mid] == "wgnhs"
    assert W.FORMS_OF[96] == "h" and W.BLOCKS_OF[96] == W.BLOCKS_OF[80]
    for b in B.BLOCKS:
        for f in W.ALL:
            sh = W.shapes(b, f)
            assert (any(s[3] for s in sh)) == (B.LEVEL[b] == 0), b       # one periodic-yx case at level 0
            if b in W.RES:
                assert {s[0] - 4 for s in sh if not s[3]} == ({2} if f == "g" else {2, 3})
                assert all((s[1] - (0 if s[3] else 4), s[2] - (0 if s[3] else 4)) == (9, 33) for s in sh)


def test_head_kernel_limit():
    """h3nz_ok: 4 chunks of conv_1 and of the skip.  On it at width 64, one past at 72; the other widths 5 .. 11"""
    k = lambda mid: la('conv_r01', mid, "w")[-1]
    assert [W.nchunk(m) for m in (64, 72, 80, 128, 136)] == [4, 5, 5, 8, 9] and W.HNZ_MAXCH == 4
    assert k(64).kernel == "h3nz" and all(k(m).kernel == "h3g_narrow" for m in (72, 80, 128, 136))
    assert [(k(m).nskip, W.nchunk(k(m).cin)) for m in (72, 128)] == [(5, 5), (8, 8)]
    assert k(64).label == k(72).label == "conv_h3n<FLAT3,vel,dx>"           # one label, one path bit for both kernels
    assert "narrow" in W.paths('conv_r01', 136, "w", ODD) and k(176).kernel == "h3q"
    assert all(3 * W.nchunk(m) + W.nchunk(m) <= W.MAX_GROUPS for m in W.WIDTHS)


def test_up8_limit():
    """up8_fits: cin_pad / 16 <= 4.  On it at 64, one past at 72: eight launches per block in every half-precision form"""
    for f in "wnh":
        assert [x.kernel for x in la('up_r1', 64, f, (1, 6, 6, 0))] == ["up8"]
        for mid in W.WIDTHS:
            got = la('up_r1', mid, f, (1, 6, 6, 0))
            assert len(got) == 8 and {x.kernel for x in got} == {"h3_flat1"} and W.paths('up_r1', mid, f, (1, 6, 6, 0)) == set()
    assert W.labels('up_r0', 72, "w", (1, 8, 8, 0)) == {"conv_h3<FLAT1,vel,dx>": 16}
    assert W.labels('up_r0', 72, "h", (1, 8, 8, 0)) == {"conv_h1<FLAT1,vel,dx>": 16}
    assert W.labels('up_r0', 72, "s", (1, 8, 8, 0)) == {"conv_mfma<FLAT1,vel,dx,ni2>": 16}
    assert W.labels('down_l0', 72, "w", (2, 96, 96, 0)) == {"conv_h3<DOWN,vel,dx>": 1}


def test_winograd_z_limits_of_f16x3():
    """NBE_MAX_WSTAGES = 32 (8 chunks) and NBE_MAX_WSKIP = 16 (8 chunks): on them at 128 in the encoders (and at 64 in the
    decoders), one past at 136 (and at 72 in the decoders: 9 chunks)"""
    enc = lambda mid, f="w": [x.kernel for x in la('conv_l01', mid, f)]
    assert enc(128) == ["h3w_f16x3", "h3w_f16x3"] and la('conv_l01', 128, "w")[1].nskip == 8 and 4 * W.nchunk(128) == W.MAX_WSTAGES
    assert 2 * W.nchunk(128) == W.MAX_WSKIP
    assert enc(136) == ["h3g_wide", "h3g_wide"] and W.nchunk(136) == 9
    assert enc(72) == enc(80) == ["h3w_f16x3", "h3w_f16x3"] and la('conv_l01', 72, "w")[1].nskip == 5        # an odd nskip
    assert [x.kernel for x in la('conv_r00', 64, "w")] == ["h3w_f16x3", "h3w_f16x3"]
    for mid in (72, 80, 128):
        c0, c1 = la('conv_r00', mid, "w")
        assert (c0.kernel, c1.kernel) == ("h3g_wide", "h3g_wide") and c1.nskip == W.nchunk(2 * mid) >= 9
    assert [W.nchunk(2 * m) for m in (72, 80, 128)] == [9, 10, 16]
    assert (W.nct(144), W.nct(272), 144 % 64, 272 % 64) == (3, 5, 16, 16)                                  # ragged last cout tiles
    # an odd plane count or NBE_WINO=0 takes every launch off the kernel
    assert [x.kernel for x in la('conv_l01', 128, "w", ODD)] == enc(128, "g") == ["h3g_wide", "h3g_wide"]
    # displacement only: no block fuses above 64 (all or none), conv_0 keeps the form where it has a packing
    assert W.novel_fuse(64, X3N) and not any(W.novel_fuse(m, X3N) for m in W.WIDTHS)
    assert enc(128, "n") == ["h3_flat1", "h3w_novel", "h2q_split"] and enc(136, "n") == ["h3_flat1", "h2q_split", "h2q_split"]
    assert W.paths('conv_l01', 128, "n", EVEN) == {"wino_0"} and W.paths('conv_l01', 128, "n", ODD) == set()


def test_winograd_z_limits_of_float16():
    """whole 32-channel stages, at most 32 / 4 = 8 of them, a skip of at most 8: met exactly by the decoders at 128; 5 stages
    (an odd count) at 80; 3 + 3 at 96; no form at 72 and 136 (80, 144, 272 channels)"""
    dec = lambda mid, shape=EVEN, src="cat": la('conv_r1', mid, "h", shape, src)
    assert [x.kernel for x in dec(128)] == ["h3w_f16", "h3w_f16"] and dec(128)[1].nskip // 2 == 8 == W.MAX_WSKIP // 2
    assert 4 * (256 // 32) == W.MAX_WSTAGES
    assert [x.kernel for x in dec(80)] == ["h3w_f16", "h3w_f16"] and W.nchunk(160) // 2 == 5
    assert W.sources('conv_r1', 80, "h", EVEN) == ("cat",) and W.sources('conv_r1', 80, "w", EVEN) == ("cat", "two")
    assert W.sources('conv_r1', 96, "h", EVEN) == W.sources('conv_r1', 128, "h", EVEN) == ("cat", "two")
    assert dec(96, src="two")[0].split == 6 and dec(96, src="two")[1].split == 6 and [x.nskip for x in la('conv_l01', 96, "h")] == [0, 6]
    for mid in (72, 136):
        assert [x.kernel for x in dec(mid)] == ["h3_flat1", "h2q_f16_g", "h2q_f16_g"] and not W.expect_fused('conv_r1', mid, "f16", True, True, 2, True)
    assert [x.kernel for x in la('conv_l01', 80, "h")] == ["h3_flat1", "h2q_f16_g", "h2q_f16_g"]             # 80 is no multiple of 32
    assert [x.kernel for x in dec(128, ODD)] == ["h3_flat1", "h2q_f16_g", "h2q_f16_g"]
    assert [x.kernel for x in dec(176)] == ["h3_flat1", "h2q_f16", "h2q_f16"]                                 # gauge off
    # conv_l00: its skip reads the input field; conv_1 keeps the Winograd-z form with a residual
    assert [x.kernel for x in la('conv_l00', 128, "h")] == ["h3_flat1", "h3p", "h3w_f16"] and la('conv_l00', 128, "h")[2].res


def test_group_table_limits():
    """NBE_MAX_GROUPS = 64: filled exactly by a fused decoder conv_1 at 128 (3 * 16 + 16), exceeded at 136 (68): the decoders run
    unfused there and every other block fused; 3 * 22 = 66 groups of the decoders' conv_0 at 176 turn the gauge off"""
    g = lambda mid: 3 * W.nchunk(2 * mid) + W.nchunk(2 * mid)
    assert [g(m) for m in (80, 128, 136)] == [40, 64, 68] and W.MAX_GROUPS == 64
    for d in B.DECODERS:
        assert W.fskip(d, 128, X3V) and not W.fskip(d, 136, X3V)
        assert [x.kernel for x in la(d, 136, "w")] == ["h3_flat1", "h3g_wide", "h3g_wide"] and la(d, 136, "w")[2].res
        assert W.paths(d, 136, "w", EVEN) == set() and W.sources(d, 136, "w", EVEN) == ("cat",)
        assert W.paths(d, 128, "w", EVEN, "two") == {"skip_fused", "two_source", "two_source_skip"}
    for b in W.RES:
        if b not in B.DECODERS:
            assert W.expect_fused(b, 136, "f16x3", True, True, 3, True) and W.fskip(b, 136, X3V), b
    assert [3 * W.nchunk(2 * m) for m in (128, 136, 176)] == [48, 51, 66]
    for f in (X3V, X3G, H1V, F32):
        assert [W.gauge_active(m, f) for m in W.WIDTHS] == [True] * 5 + [False]
        assert not W.gauge_active(72, f, gauge=False)
    assert not any(W.gauge_active(m, X3N) for m in W.WIDTHS)
    for f in "wghs":
        for b in W.BLOCKS_OF[176]:
            for shape in W.shapes(b, f):
                assert not W.paths(b, 176, f, shape), (b, f)
                assert {x.kernel for x in W.launches(b, 176, f, shape)} <= {"h3q", "h2q_f16", "mfma", "h3_flat1"}
    assert W.labels('conv_r00', 176, "w", EVEN) == {"conv_h3<FLAT1,vel,dx>": 1, "conv_h3<FLAT3,vel,dx>": 2}
    assert W.labels('conv_r01', 176, "s", EVEN) == {"conv_mfma<FLAT1,vel,dx,ni1>": 1, "conv_mfma<FLAT3,vel,dx,ni2>": 1, "conv_mfma<FLAT3,vel,dx,ni1>": 1}


def test_first_layer_has_no_stem_packing_above_64():
    assert la('conv_l00', 64, "w")[0].kernel == "stem"
    assert [(f, la('conv_l00', 72, f)[-2].kernel, la('conv_l00', 72, f)[-2].label) for f in "wnh"] == [
        ("w", "h3p", "conv_h3<FLAT3,vel,nodx>"), ("n", "h2q_split", "conv_h3<FLAT3,novel,nodx>"), ("h", "h3p", "conv_h1<FLAT3,vel,nodx>")]
    assert W.paths('conv_l00', 128, "w", EVEN) == {"skip_fused", "skip_nodx", "wino_1"}


def test_two_source_widths():
    assert [W.two_source_width(m, "f16x3") for m in W.WIDTHS] == [False, True, True, True, False, True]
    assert [W.two_source_width(m, "f16") for m in W.WIDTHS] == [False, False, True, True, False, False]
    c0, c1 = la('conv_r00', 80, "w", src="two")
    assert (c0.split, c1.split, c1.nskip) == (5, 5, 10) and c0.kernel == c1.kernel == "h3g_wide"
    assert W.sources('conv_r00', 72, "w", EVEN) == ("cat",) and W.sources('conv_r00', 176, "w", EVEN) == ("cat",)


# rows of tests/test_conv_select.py that a launch of this table restates: (row, block, mid, form, shape, launch)
OVERLAP = [("x3v_head_skip80", 'conv_r01', 80, "w", EVEN, -1), ("x3v_cin128", 'conv_l01', 128, "w", EVEN, 0),
           ("x3v_skip128", 'conv_l01', 128, "w", EVEN, 1), ("x3v_cin144_fallback", 'conv_l01', 136, "w", EVEN, 0),
           ("x3v_skip144_fallback", 'conv_l01', 136, "w", EVEN, 1), ("x3v_conv0_odd_Dv", 'conv_l01', 72, "w", ODD, 0),
           ("x3v_conv1_fused_wino_off", 'conv_l01', 72, "g", EVEN, 1), ("x3v_conv1_unfused_res", 'conv_r1', 136, "w", EVEN, 2),
           ("x3v_up_parity_cin80", 'up_r1', 80, "w", (1, 6, 6, 0), 0), ("x3v_skip", 'conv_r1', 136, "w", EVEN, 0),
           ("x3v_nogauge_conv", 'conv_l01', 176, "w", EVEN, 1), ("x3v_first_no_stem", 'conv_l00', 72, "w", EVEN, 0),
           ("x3n_cin144_fallback", 'conv_l01', 136, "n", EVEN, 1), ("x3n_conv", 'conv_l01', 128, "n", EVEN, 1),
           ("x3n_conv_res", 'conv_l01', 128, "n", EVEN, 2), ("h1v_cin256", 'conv_r1', 128, "h", EVEN, 0),
           ("h1v_conv1_fused", 'conv_r1', 128, "h", EVEN, 1), ("h1v_conv0_two_source", 'conv_r1', 128, "h", EVEN, 0),
           ("h1v_conv0_odd_Dv", 'conv_r1', 128, "h", ODD, 1), ("h1v_nogauge_conv", 'conv_l01', 176, "h", EVEN, 1),
           ("h1v_first_no_stem", 'conv_l00', 72, "h", EVEN, 1), ("f32v_conv_gauged", 'conv_l01', 72, "s", EVEN, 1),
           ("f32v_conv", 'conv_l01', 176, "s", EVEN, 1), ("f32v_skip", 'conv_l01', 72, "s", EVEN, 0)]


@pytest.mark.parametrize("row,block,mid,form,shape,i", OVERLAP, ids=[o[0] for o in OVERLAP])
def test_rows_agree_with_the_rows_of_test_conv_select(row, block, mid, form, shape, i):
    t = {r[0]: r for r in CS.TABLE}[row]
    src = "two" if "two_source" in row else "cat"
    x = W.launches(block, mid, form, shape, src)[i]
    assert (x.kernel, x.label) == (t[2], t[3]), (row, x)


@pytest.mark.skipif(not os.path.exists(CS.HIPCC), reason="needs hipcc")
def test_every_launch_of_the_table_is_what_conv_select_answers(tmp_path):
    """every launch of every (width, block, form, shape, source) as a case of tools/conv_select_walk.hip: the kernel and the
    profile label conv_select / conv_label give for what launch_conv would hand them"""
    prog = str(tmp_path / "conv_select_walk")
    r = subprocess.run([CS.HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", prog,
                        os.path.join(CS.ROOT, "tools", "conv_select_walk.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    want, lines, case = {}, [], {}
    for mid, block, form in W.MATRIX + [(64, b, f) for b in B.BLOCKS for f in W.ALL]:
        for shape in W.shapes(block, form):
            for src in W.sources(block, mid, form, shape, W.gauge_active(mid, W.FORMS[form]) or not W.FORMS[form].vel):
                for n, (x, line) in enumerate(W.walk_rows(block, mid, form, shape, src)):
                    name = "m%d-%s-%s-%s-%s-%d" % (mid, block, form, "x".join(map(str, shape)), src, n)
                    want[name] = (x.kernel, x.label)
                    lines.append("%s %s\n" % (name, line))
                    case[name] = line
    assert len(want) == len(lines) > 1500
    r = subprocess.run([prog], input="".join(lines), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    got = dict((f[0], (f[1], f[2])) for f in (ln.split("\t") for ln in r.stdout.splitlines()))
    bad = [(n, case[n], got.get(n), want[n]) for n in want if got.get(n) != want[n]]
    assert not bad, bad[:10]
    kernels = {k for k, _ in want.values()}
    assert kernels >= {"h3g_narrow", "h3nz", "h3g_wide", "h3w_f16x3", "h3w_novel", "h3w_f16", "h2q_f16_g", "h2q_f16", "h2q_split",
                       "h3q", "h3p", "stem", "up8", "h3_flat1", "h3_down", "mfma", "mfma_g"} and "none" not in kernels


def test_expect_fused_generalises_the_rule_of_test_gpu_blocks():
    """identical for every width the older rule is stated for"""
    n = 0
    for block, mid, prec, vel, gauge, nres, wino_on in itertools.product(W.RES, TB.MIDS, TB.PRECS, (True, False), (True, False),
                                                                       (1, 2, 3, 4), (True, False)):
        assert W.expect_fused(block, mid, prec, vel, gauge, nres, wino_on) == TB.expect_fused(block, mid, prec, vel, gauge, nres, wino_on), \
            (block, mid, prec, vel, gauge, nres, wino_on)
        n += 1
    assert n == 9 * 5 * 3 * 2 * 2 * 4 * 2
    # and above: what the issue lists
    assert all(W.expect_fused(b, 72, "f16x3", True, True, 3, False) for b in W.RES)
    assert not any(W.expect_fused(b, 72, "f16x3", False, True, 2, True) or W.expect_fused(b, 72, "f16", True, True, 2, True) for b in W.RES)
    assert [W.expect_fused('conv_r1', m, "f16", True, True, 2, True) for m in W.WIDTHS] == [False, True, True, True, False, False]
    assert [W.expect_fused('conv_l1', m, "f16", True, True, 2, True) for m in W.WIDTHS] == [False, False, True, True, False, False]
    assert not W.expect_fused('conv_l00', 128, "f16", True, True, 2, True) and not W.expect_fused('conv_r1', 128, "f16", True, True, 3, True)
    assert not any(W.expect_fused(b, 176, p, True, True, 2, True) for b in W.RES for p in TB.PRECS)


def test_block_oracle_at_the_widest_layer():
    """conv_r00 at width 176 (352 -> 352 -> 176, K = 27 * 352 + 352) on the smallest input the hook takes: both backends of
    the oracle agree, with the three-product form the engine runs there (gauged = False, zero gauges)"""
    mid, block, shape = 176, 'conv_r00', (5, 5, 6, 0)
    p, s = TB.params_of(mid), TB.s64()
    g = tuple(np.zeros_like(t) for t in B.gauges(p, s, block, mid))
    x, dxs = TB.make_input(block, mid, "f16x3", True, shape, g[0])
    x, dxs = x.astype(np.float64), dxs.astype(np.float64)
    res = {}
    for be in ("numpy", "torch"):
        with L.backend(be):
            h, dh = B.stage1(p, s, block, x, dxs, mid, g=g, gauged=False).result()
            res[be] = (h, dh) + B.stage2(p, s, block, x, dxs, h, dh, mid, g=g, gauged=False, fused=False).result()
    assert res["numpy"][0].shape == (352, 3, 3, 4) and res["numpy"][2].shape == (176, 1, 1, 2)
    for a, b in zip(res["numpy"], res["torch"]):
        assert np.all(np.isfinite(a)) and np.abs(a - b).max() <= 1e-12 * float(np.sqrt(np.mean(a ** 2)))
