"""CPU: which kernel a convolution launch gets (conv_select, csrc/nbe_conv_select.h) and the profile label it is given
(conv_label), walked by tools/conv_select_walk.hip and held to the table below.

The table was read from the try-and-fall-back chain that conv_select replaced -- the sources of commit 42febe8, cited per
row as file:line -- not from the new function:
  h3    csrc/nbe_kernels_h3.hip    launch_conv_h3 2090-2141, launch_up_h3 500, launch_h3q 1083, launch_h3g 1471-1473,
                                   launch_h2q 1801, launch_stem 2068
  wino  csrc/nbe_kernels_wino.h    launch_h3w 889-905
  head  csrc/nbe_kernels_head.h    launch_h3nz 272-276
  k     csrc/nbe_kernels.hip       launch_conv 280-302
  net   csrc/nbe_engine_net.cpp    conv_name 77-89, run_conv 113-123
A launch that the Winograd-z launcher refused for a reason run_conv did not model (more than NBE_MAX_WSTAGES stages, more than
NBE_MAX_WSKIP skip entries, a plane stride of 2^32 bytes) ran the direct kernel under the label conv_h3w / conv_h1w there; here
it carries the label of the kernel that runs (rows marked "fallback").  The program is built here without sanitizers; the
recipe with them is at its head."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"

pytestmark = pytest.mark.skipif(not os.path.exists(HIPCC), reason="needs hipcc")

P28 = 1 << 28            # voxels: 2^32 bytes between planes
BELOW = P28 - (1 << 17)  # 2^32 - 2^21 bytes: with ten rows of W = 32 voxels still under 2^32 - 2^20

G = "beta=1"                               # gauged input tangent
GW = "beta=1 ww=1"                         # ... and the Winograd-z kernel allowed
SK = "skip=64 wws=1"                       # a fused skip of 64 channels with its Winograd-z weights
HEAD = "cout=3 cout_t=16 ctiles=1 beta=1"  # conv_r01/conv_1 in the narrow packing

# (name, case, kernel, label, where the parent says so)
TABLE = [
    # ---- f16x3, velocity: the U-Net's layer forms -------------------------------------------------------------------------
    ("x3v_first_stem", "cin=3 dx=0 stem=1", "stem", "stem_h3<FLAT3,vel,nodx>", "h3:2093-2095 net:80"),
    ("x3v_first_stem_72couts", "cin=3 dx=0 stem=1 cout=72", "none", "none", "h3:2068"),
    ("x3v_first_no_stem", "cin=3 dx=0", "h3p", "conv_h3<FLAT3,vel,nodx>", "h3:2128 net:85"),
    ("x3v_conv0", GW, "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "h3:2113 net:122"),
    ("x3v_conv0_wino_off", G, "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "h3:2113-2114 net:82"),
    ("x3v_conv0_odd_Dv", GW + " Dv=7", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:901 h3:2114 net:113"),
    ("x3v_conv0_two_source", GW + " cin=128 csplit=64", "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "h3:2099 h3:2113"),
    ("x3v_conv0_two_source_wino_off", G + " cin=128 csplit=64", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "h3:2099 h3:2114"),
    ("x3v_conv1_fused", GW + " " + SK, "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:902 h3:2113"),
    ("x3v_conv1_fused_no_wws", GW + " skip=64", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:902 h3:2114 net:113"),
    ("x3v_conv1_fused_wino_off", G + " skip=64", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "h3:2114"),
    ("x3v_conv1_fused_odd_Dv", GW + " " + SK + " Dv=5", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:901 h3:2114"),
    ("x3v_conv1_fused_nodx", GW + " " + SK + " nodx=1", "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:897 (float16 only) h3:2113"),
    ("x3v_conv1_fused_two_source_skip", GW + " skip=128 wws=1 s_csplit=64", "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:902 h3:2113"),
    ("x3v_conv1_unfused_res", GW + " res=1", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:901 h3:2114 net:113"),
    ("x3v_skip", "mode=flat1", "h3_flat1", "conv_h3<FLAT1,vel,dx>", "h3:2138 net:85"),
    ("x3v_skip_first", "mode=flat1 cin=3 dx=0", "h3_flat1", "conv_h3<FLAT1,vel,nodx>", "h3:2138 net:85"),
    ("x3v_down", "mode=down", "h3_down", "conv_h3<DOWN,vel,dx>", "h3:2140 net:85"),
    ("x3v_up8_cin64", "mode=flat1 up8=1 osz=2", "up8", "up_h3<8 parities,vel,dx>", "h3:2134 net:78"),
    ("x3v_up8_cin80", "mode=flat1 up8=1 osz=2 cin=80", "none", "none", "h3:500"),
    ("x3v_up8_no_dx", "mode=flat1 up8=1 osz=2 dx=0", "none", "none", "h3:2136"),
    ("x3v_up_parity_cin80", "mode=flat1 osz=2 cin=80", "h3_flat1", "conv_h3<FLAT1,vel,dx>", "h3:2138"),
    ("x3v_head_3couts", HEAD + " skip=64", "h3nz", "conv_h3n<FLAT3,vel,dx>", "head:275-276 h3:2110 net:82"),
    ("x3v_head_3couts_two_source", HEAD + " cin=128 csplit=64", "h3g_narrow", "conv_h3n<FLAT3,vel,dx>", "head:276 h3:2111"),
    ("x3v_head_8couts", "cout=8 cout_t=16 ctiles=1 beta=1 skip=64", "h3g_narrow", "conv_h3n<FLAT3,vel,dx>", "head:275 h3:2111"),
    ("x3v_head_res", HEAD + " res=1", "h3g_narrow", "conv_h3n<FLAT3,vel,dx>", "head:275 h3:2111"),
    ("x3v_head_skip_nodx", HEAD + " skip=64 nodx=1", "h3g_narrow", "conv_h3n<FLAT3,vel,dx>", "head:275 h3:2111"),
    ("x3v_head_cin80", HEAD + " cin=80", "h3g_narrow", "conv_h3n<FLAT3,vel,dx>", "head:276 (HNZ_MAXCH) h3:2111"),
    ("x3v_head_skip80", HEAD + " skip=80", "h3g_narrow", "conv_h3n<FLAT3,vel,dx>", "head:276 (HNZ_MAXCH) h3:2111"),
    ("x3v_head_two_tiles", "cout=24 cout_t=16 ctiles=1 beta=1", "none", "none", "head:275 h3:1471"),
    # ---- f16x3, velocity: the limits ----------------------------------------------------------------------------------------
    ("x3v_cin128", GW + " cin=128", "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:901 (NBE_MAX_WSTAGES)"),
    ("x3v_cin144_fallback", GW + " cin=144", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:901 (NBE_MAX_WSTAGES) h3:2114; fallback"),
    ("x3v_skip128", GW + " skip=128 wws=1", "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:902 (NBE_MAX_WSKIP)"),
    ("x3v_skip144_fallback", GW + " skip=144 wws=1", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:902 (NBE_MAX_WSKIP) h3:2114; fallback"),
    ("x3v_groups_64", G + " cin=336 skip=16", "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "h3:1473 (NBE_MAX_GROUPS)"),
    ("x3v_groups_65", G + " cin=336 skip=32", "none", "none", "h3:1473 (NBE_MAX_GROUPS)"),
    ("x3v_pstride_below", GW + " pstride=%d" % BELOW, "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:905"),
    ("x3v_pstride_2p32_fallback", GW + " pstride=%d" % P28, "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:905 h3:2114; fallback"),
    ("x3v_pstride2_unused", GW + " pstride2=%d" % P28, "h3w_f16x3", "conv_h3w<FLAT3,vel,dx>", "wino:905 (second source only where read)"),
    ("x3v_pstride2_2p32_fallback", GW + " cin=128 csplit=64 pstride2=%d" % P28, "h3g_wide", "conv_h3g<FLAT3,vel,dx>", "wino:905 h3:2114; fallback"),
    ("x3v_cout_tiles_mismatch", G + " ctiles=2", "none", "none", "h3:1471"),
    ("x3v_gauged_cropped", GW + " in_off=5", "none", "none", "h3:2107"),
    ("x3v_gauged_strided", G + " osz=2", "none", "none", "h3:2107"),
    ("x3v_gauged_flat1", "mode=flat1 beta=1", "none", "none", "h3:2107"),
    ("x3v_gauged_no_dx", "beta=1 dx=0", "none", "none", "h3:2107"),
    # ---- f16x3, velocity, gauge off -------------------------------------------------------------------------------------------
    ("x3v_nogauge_conv", "ww=1", "h3q", "conv_h3<FLAT3,vel,dx>", "h3:2121 net:85"),
    ("x3v_nogauge_res", "res=1", "h3q", "conv_h3<FLAT3,vel,dx>", "h3:2121"),
    ("x3v_nogauge_cropped", "in_off=5", "none", "none", "h3:2120"),
    ("x3v_nogauge_strided", "osz=2", "none", "none", "h3:2120"),
    ("x3v_nogauge_fused", "skip=64", "none", "none", "h3:2099-2104"),
    ("x3v_nogauge_two_source", "cin=128 csplit=64", "none", "none", "h3:2099-2104"),
    # ---- f16x3, displacement only ---------------------------------------------------------------------------------------------
    ("x3n_first_stem", "vel=0 dx=0 cin=3 stem=1", "stem", "stem_h3<FLAT3,novel>", "h3:2095 net:80"),
    ("x3n_conv", "vel=0 ww=1", "h3w_novel", "conv_h3w<FLAT3,novel>", "h3:2122 net:122"),
    ("x3n_conv_wino_off", "vel=0", "h2q_split", "conv_h3<FLAT3,novel,nodx>", "h3:2123 net:85"),
    ("x3n_conv_odd_Dv", "vel=0 ww=1 Dv=9", "h2q_split", "conv_h3<FLAT3,novel,nodx>", "wino:901 h3:2123"),
    ("x3n_conv_res", "vel=0 ww=1 res=1", "h2q_split", "conv_h3<FLAT3,novel,nodx>", "wino:901 h3:2123"),
    ("x3n_fused", "vel=0 ww=1 " + SK, "h3w_novel", "conv_h3w<FLAT3,novel>", "h3:2100-2101"),
    ("x3n_fused_two_source", "vel=0 ww=1 cin=128 csplit=64 skip=128 wws=1 s_csplit=64", "h3w_novel", "conv_h3w<FLAT3,novel>", "h3:2100-2101"),
    ("x3n_fused_wino_off", "vel=0 skip=64", "none", "none", "h3:2100-2104"),
    ("x3n_fused_odd_Dv", "vel=0 ww=1 " + SK + " Dv=7", "none", "none", "wino:901 h3:2101"),
    ("x3n_cin144_fallback", "vel=0 ww=1 cin=144", "h2q_split", "conv_h3<FLAT3,novel,nodx>", "wino:901 (NBE_MAX_WSTAGES) h3:2123; fallback"),
    ("x3n_pstride_2p32_fallback", "vel=0 ww=1 pstride=%d" % P28, "h2q_split", "conv_h3<FLAT3,novel,nodx>", "wino:905 h3:2123; fallback"),
    ("x3n_head", "vel=0 ww=1 cout=3", "h3w_novel", "conv_h3w<FLAT3,novel>", "h3:2122"),
    ("x3n_skip", "vel=0 mode=flat1", "h3_flat1", "conv_h3<FLAT1,novel,nodx>", "h3:2138 net:85"),
    ("x3n_down", "vel=0 mode=down", "h3_down", "conv_h3<DOWN,novel,nodx>", "h3:2140 net:85"),
    ("x3n_up8", "vel=0 mode=flat1 up8=1 osz=2", "up8", "up_h3<8 parities,novel>", "h3:2135 net:78"),
    ("x3n_cropped", "vel=0 in_off=3", "none", "none", "h3:2120"),
    # ---- float16, velocity ------------------------------------------------------------------------------------------------------
    ("h1v_first_stem", "prec=f16 cin=3 dx=0 stem=1", "stem", "stem_h3<FLAT3,vel,nodx>", "h3:2096 net:80"),
    ("h1v_first_no_stem", "prec=f16 cin=3 dx=0", "h3p", "conv_h1<FLAT3,vel,nodx>", "h3:2129 net:85"),
    ("h1v_conv0", "prec=f16 " + GW, "h3w_f16", "conv_h1w<FLAT3,vel,dx>", "h3:2116 net:122"),
    ("h1v_conv0_wino_off", "prec=f16 " + G, "h2q_f16_g", "conv_h1g<FLAT3,vel,dx>", "h3:2117 net:82"),
    ("h1v_conv0_odd_Dv", "prec=f16 " + GW + " Dv=7", "h2q_f16_g", "conv_h1g<FLAT3,vel,dx>", "wino:901 h3:2117"),
    ("h1v_conv1_unfused_res", "prec=f16 " + GW + " res=1", "h3w_f16", "conv_h1w<FLAT3,vel,dx>", "wino:901 (float16 keeps F_RES) h3:2116"),
    ("h1v_conv0_cin48", "prec=f16 " + GW + " cin=48", "h2q_f16_g", "conv_h1g<FLAT3,vel,dx>", "wino:896 h3:2117"),
    ("h1v_conv0_two_source", "prec=f16 " + GW + " cin=128 csplit=64", "h3w_f16", "conv_h1w<FLAT3,vel,dx>", "h3:2102-2103"),
    ("h1v_conv0_two_source_csplit48", "prec=f16 " + GW + " cin=96 csplit=48", "none", "none", "wino:896 h3:2103"),
    ("h1v_conv0_two_source_wino_off", "prec=f16 " + G + " cin=128 csplit=64", "none", "none", "h3:2102-2104"),
    ("h1v_conv1_fused", "prec=f16 " + GW + " " + SK, "h3w_f16", "conv_h1w<FLAT3,vel,dx>", "h3:2102-2103"),
    ("h1v_conv1_fused_nodx", "prec=f16 " + GW + " " + SK + " nodx=1", "none", "none", "wino:897 h3:2103"),
    ("h1v_conv1_fused_skip48", "prec=f16 " + GW + " skip=48 wws=1", "none", "none", "wino:897 h3:2103"),
    ("h1v_conv1_fused_odd_Dv", "prec=f16 " + GW + " " + SK + " Dv=7", "none", "none", "wino:901 h3:2103"),
    ("h1v_cin256", "prec=f16 " + GW + " cin=256", "h3w_f16", "conv_h1w<FLAT3,vel,dx>", "wino:898-901 (NBE_MAX_WSTAGES)"),
    ("h1v_cin288_fallback", "prec=f16 " + GW + " cin=288", "h2q_f16_g", "conv_h1g<FLAT3,vel,dx>", "wino:901 (NBE_MAX_WSTAGES) h3:2117; fallback"),
    ("h1v_skip288", "prec=f16 " + GW + " skip=288 wws=1", "none", "none", "wino:902 (NBE_MAX_WSKIP) h3:2103"),
    ("h1v_pstride_2p32_fallback", "prec=f16 " + GW + " pstride=%d" % P28, "h2q_f16_g", "conv_h1g<FLAT3,vel,dx>", "wino:905 h3:2117; fallback"),
    ("h1v_head", "prec=f16 " + GW + " cout=3", "h3w_f16", "conv_h1w<FLAT3,vel,dx>", "h3:2116"),
    ("h1v_nogauge_conv", "prec=f16 ww=1", "h2q_f16", "conv_h1<FLAT3,vel,dx>", "h3:2124 net:85"),
    ("h1v_skip", "prec=f16 mode=flat1", "h3_flat1", "conv_h1<FLAT1,vel,dx>", "h3:2138 net:85"),
    ("h1v_down", "prec=f16 mode=down", "h3_down", "conv_h1<DOWN,vel,dx>", "h3:2140 net:85"),
    ("h1v_up8", "prec=f16 mode=flat1 up8=1 osz=2", "up8", "up_h3<8 parities,vel,dx>", "h3:2134 net:78"),
    ("h1v_up8_cin80", "prec=f16 mode=flat1 up8=1 osz=2 cin=80", "none", "none", "h3:500"),
    ("h1v_gauged_cropped", "prec=f16 " + GW + " in_off=2", "none", "none", "h3:2107"),
    # ---- float16, displacement only -------------------------------------------------------------------------------------------
    ("h1n_first_stem", "prec=f16 vel=0 dx=0 cin=3 stem=1", "stem", "stem_h3<FLAT3,novel>", "h3:2096 net:80"),
    ("h1n_conv", "prec=f16 vel=0 ww=1", "h3p", "conv_h1<FLAT3,novel,nodx>", "h3:2127 net:85"),
    ("h1n_conv_res_odd_Dv", "prec=f16 vel=0 res=1 Dv=7", "h3p", "conv_h1<FLAT3,novel,nodx>", "h3:2127"),
    ("h1n_fused", "prec=f16 vel=0 ww=1 " + SK, "none", "none", "h3:2099-2104"),
    ("h1n_skip", "prec=f16 vel=0 mode=flat1", "h3_flat1", "conv_h1<FLAT1,novel,nodx>", "h3:2138 net:85"),
    ("h1n_down", "prec=f16 vel=0 mode=down", "h3_down", "conv_h1<DOWN,novel,nodx>", "h3:2140 net:85"),
    ("h1n_up8", "prec=f16 vel=0 mode=flat1 up8=1 osz=2", "up8", "up_h3<8 parities,novel>", "h3:2135 net:78"),
    ("h1n_strided", "prec=f16 vel=0 osz=2", "none", "none", "h3:2120"),
    # ---- strict float32 ---------------------------------------------------------------------------------------------------------
    ("f32v_first", "prec=f32 cin=3 dx=0", "mfma", "conv_mfma<FLAT3,vel,nodx,ni2>", "k:298 net:87"),
    ("f32v_conv", "prec=f32", "mfma", "conv_mfma<FLAT3,vel,dx,ni2>", "k:298 net:87"),
    ("f32v_conv_gauged", "prec=f32 beta=1", "mfma_g", "conv_mfma_g<FLAT3,vel,dx,ni2>", "k:282-286 net:83"),
    ("f32v_conv_gauged_odd_Dv_res", "prec=f32 beta=1 ww=1 Dv=7 res=1", "mfma_g", "conv_mfma_g<FLAT3,vel,dx,ni2>", "k:282-286"),
    ("f32v_head_gauged", "prec=f32 beta=1 cout=3 ni=1", "mfma_g", "conv_mfma_g<FLAT3,vel,dx,ni1>", "k:285 net:83"),
    ("f32v_gauged_flat1", "prec=f32 beta=1 mode=flat1", "none", "none", "k:283"),
    ("f32v_gauged_no_dx", "prec=f32 beta=1 dx=0", "none", "none", "k:283"),
    ("f32v_cropped", "prec=f32 in_off=5", "mfma", "conv_mfma<FLAT3,vel,dx,ni2>", "k:298"),
    ("f32v_skip", "prec=f32 mode=flat1", "mfma", "conv_mfma<FLAT1,vel,dx,ni2>", "k:299 net:87"),
    ("f32v_up_parity", "prec=f32 mode=flat1 osz=2", "mfma", "conv_mfma<FLAT1,vel,dx,ni2>", "k:299"),
    ("f32v_down", "prec=f32 mode=down", "mfma", "conv_mfma<DOWN,vel,dx,ni2>", "k:300 net:87"),
    ("f32n_conv", "prec=f32 vel=0", "mfma", "conv_mfma<FLAT3,novel,nodx,ni2>", "k:298 net:87"),
    ("f32n_head", "prec=f32 vel=0 cout=3 ni=1", "mfma", "conv_mfma<FLAT3,novel,nodx,ni1>", "k:298 net:87"),
    ("f32n_down", "prec=f32 vel=0 mode=down", "mfma", "conv_mfma<DOWN,novel,nodx,ni2>", "k:300 net:87"),
]


@pytest.fixture(scope="module")
def walked(tmp_path_factory):
    prog = str(tmp_path_factory.mktemp("conv_select_walk") / "conv_select_walk")
    r = subprocess.run([HIPCC, "-x", "hip", "--offload-arch=gfx950", "-O1", "-std=c++17", "-o", prog,
                        os.path.join(ROOT, "tools", "conv_select_walk.hip")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    cases = "".join("%s %s\n" % (name, case) for name, case, _, _, _ in TABLE)
    r = subprocess.run([prog], input=cases, capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    out = dict((f[0], (f[1], f[2])) for f in (line.split("\t") for line in r.stdout.splitlines()))
    assert len(out) == len(TABLE) == len(set(t[0] for t in TABLE))
    return out


@pytest.mark.parametrize("name, case, kernel, label, where", TABLE, ids=[t[0] for t in TABLE])
def test_kernel_and_label(walked, name, case, kernel, label, where):
    assert walked[name] == (kernel, label), "%s [%s]: the parent launches %s (%s)" % (name, case, kernel, where)


def test_design_table_is_the_walk(walked):
    """DESIGN.md section 4, "Which kernel runs a layer": every row of its table (form | case | kernel | label) is a case of
    this table with the same answer."""
    rows = []
    for line in open(os.path.join(ROOT, "DESIGN.md")):
        f = [c.strip().strip("`") for c in line.strip().strip("|").split("|")]
        if len(f) == 4 and f[1] and any(f[1] == t[1] for t in TABLE):
            rows.append(f)
    assert len(rows) >= 30
    by_case = dict((t[1], walked[t[0]]) for t in TABLE)
    for form, case, kernel, label in rows:
        assert by_case[case] == (kernel, label), (form, case)
