"""GPU parity, block by block, of PREMODULATED trees: the cases, checks, shapes and tolerance classes of test_gpu_blocks.py
(run_case with a tree kind; nothing is copied) on contexts loaded through nbe_load_premod_weights.

Such a context does not share the delicate part of the style path; csrc/nbe_engine_weights.cpp has its own: the gauge is
recovered from the float32 (W, dW) pairs (wire_gauge_premod: alternating least squares, accepted under 2e-6 max|dW|, alpha
centred on the middle of its range), the tangent weights of the skips and the down-sampling layers are folded on the host
(`fold`: dW - W (.) a_in, and - beta_1 (.) W_s for a skip that runs inside conv_1), and the fusion rules differ (below).
The oracle is block_ref.Premod: the tree's own arrays read as float64, the centred gauge table from the style parameters
alone (block_ref.centred through GAUGE_IN / GAUGE_OUT), float16 operands rounded as the engine stores them for such a tree.
The tree is made at exactly the style vector of the style tests (test_gpu_blocks.s64()); oracle.params.premodulate[_vel]
take (z, Om) and a growth factor of their own, so it is made layer by layer (block_ref.Premod).

The vectors the engine returns are held to the centred float64 table within 4 x PREMOD_GAUGE_DEV: the largest deviation
from that table of a NumPy restatement of the recognition (block_ref.recognise: the fit, the check and the centring in
float64 on the float32 pairs, the result stored as float32 as the engine stores it), over every gauged layer of the tested
trees -- the rule the style tests use with GAUGE_DEV.  tests/test_block_ref.py holds the restatement itself on the CPU."""

import time

import numpy as np
import pytest

import block_ref as B
import test_gpu_blocks as TB
from oracle import layers as L
from test_gpu_blocks import PRECS, RES, TOL, Tree, TREES, engines, run_case, shapes  # noqa: F401 (engines: the fixture)

pytestmark = pytest.mark.gpu

MIDS = (8, 16, 32, 64)
BAD = ("conv_l1", "conv_0", (1, 2, 0, 1, 2), 1e-3)     # test_gpu_model.py::test_premodulated_pairs_are_recognised
_PREMOD = {}
T0 = [None]


def premod_of(mid, vel=True):
    if (mid, vel) not in _PREMOD:
        _PREMOD[(mid, vel)] = B.Premod(TB.params_of(mid), TB.s64(), vel=vel)
    return _PREMOD[(mid, vel)]


def perturbed_of(mid, vel=True):
    """one dweight element moved by 1e-3 max|dweight|: the pair no longer factorises"""
    if (mid, "bad") not in _PREMOD:
        blk, lay, at, eps = BAD
        dw = np.array(premod_of(mid).tree['params'][blk][lay]['dweight'], copy=True)
        dw[at] += eps * np.abs(dw).max()
        _PREMOD[(mid, "bad")] = premod_of(mid).replaced(blk, lay, 'dweight', dw)
    return _PREMOD[(mid, "bad")]


def _premod_gauge_deviation():
    return max(r['dev'] for mid in MIDS for r in B.recognition(premod_of(mid)).values())


PREMOD_GAUGE_DEV = _premod_gauge_deviation()
print("premodulated gauge vectors: the float64 restatement of the recognition deviates from the centred table by %.2e" % PREMOD_GAUGE_DEV)


def expect_fused(block, mid, prec, vel, gauge, nres, wino_on):
    """block_fused() for a premodulated tree, restated from csrc/nbe_engine_weights.cpp: wire_gauge_premod ends with fuse =
    gauge && f16x3, so f16x3 with velocity fuses every block of a recognised tree, and the float16 model none
    (packs_wino_skip gives it the skips' Winograd-z packs with a style tree only, so wire_gauge leaves fskip unset); float32
    never; displacement-only f16x3 goes through wire_novel as a style tree does and fuses inside the Winograd-z kernel, on
    an even number of result planes."""
    if prec == "f16x3" and vel:
        return gauge
    if prec == "f16x3":
        return wino_on and nres % 2 == 0
    return False


TREES["premod"] = Tree(premod_of, expect_fused, PREMOD_GAUGE_DEV, premodulated=True)
TREES["premod_bad"] = Tree(perturbed_of, expect_fused, PREMOD_GAUGE_DEV, premodulated=True, gauge_active=False)
TREES["premod_bad"].worst = TREES["premod"].worst


def _start():
    if T0[0] is None:
        T0[0] = time.time()


@pytest.mark.parametrize("prec", PRECS)
@pytest.mark.parametrize("mid", MIDS)
@pytest.mark.parametrize("block", B.BLOCKS)
def test_block(engines, block, mid, prec):
    """velocity trees (modulate_emulator_parameters_vel): every block, every arithmetic"""
    _start()
    e = engines(mid, prec, True, tree="premod")
    assert int(e.query("gauge_active")) == 1
    head = block == 'conv_r01' and prec == "f16x3"
    if head:
        e.profile_reset(); e.profile_enable(True)
    try:
        with L.backend('torch'):
            for shape in shapes(block, full=False):
                for r in run_case(e, block, mid, prec, True, shape, tree="premod").values():
                    assert ("narrow" in r["paths"]) == head, r["paths"]
                    if prec != "f16x3":                              # the float16 model and float32 fuse none
                        assert not r["paths"] & {"skip_fused", "skip_nodx", "two_source", "two_source_skip"}, r["paths"]
    finally:
        if head:
            e.profile_enable(False)
    if head:
        names = [k["kernel"] for k in e.profile_read()]
        assert any(n.startswith("conv_h3n") for n in names), names


@pytest.mark.parametrize("mid", [16, 64])
@pytest.mark.parametrize("block", B.BLOCKS)
def test_block_displacement_only(engines, block, mid):
    """displacement-only trees (modulate_emulator_parameters) on f16x3: packed for the Winograd-z kernel when they load"""
    _start()
    e = engines(mid, "f16x3", False, tree="premod")
    with L.backend('torch'):
        for shape in shapes(block, full=False):
            run_case(e, block, mid, "f16x3", False, shape, tree="premod")


@pytest.mark.parametrize("prec", ["f16x3", "f16"])
@pytest.mark.parametrize("block", ["conv_l1", "down_l0", "conv_r00", "conv_r01"])
def test_block_falls_back_when_a_pair_does_not_factorise(engines, block, prec):
    """one perturbed dweight element: the whole network stays on the three-product kernels, plain tangents, nothing fused,
    every gauge vector zero; the oracle uses the perturbed dW as given (conv_r00: the concat form, there is no other)"""
    _start()
    mid = 16
    e = engines(mid, prec, True, tree="premod_bad")                  # NBE_GAUGE stays unset: the tree itself switches the gauge off
    assert int(e.query("gauge_active")) == 0
    with L.backend('torch'):
        for shape in shapes(block, full=False)[:2]:
            out = run_case(e, block, mid, prec, True, shape, gauge=False, tree="premod_bad")
            assert set(out) == ({"cat"} if block in RES else {"own"})
            for r in out.values():
                assert not r["gauge_in"].any() and not r["gauge_out"].any() and (r["gauge_hidden"] is None or not r["gauge_hidden"].any())
                assert not r["paths"] & {"skip_fused", "two_source", "narrow", "wino_0", "wino_1"}, r["paths"]


def test_zz_worst_cases():
    """prints the worst figure per stage, arithmetic and tolerance class of this run (DESIGN.md section 2c records them)"""
    print("\n  premodulated trees: stage | arithmetic | class | worst rel-L2 (bound) | worst max/RMS (bound)")
    for (stage, arith, cls), (e2, em) in sorted(TREES["premod"].worst.items()):
        print("  %-26s | %-10s | %-4s | %.2e (%.0e) | %.2e (%.0e)" % (stage, arith, cls, e2, TOL[cls][0], em, TOL[cls][1]))
    print("  gauge vectors: the restated recognition deviates from the centred float64 table by %.2e; bound 4x" % PREMOD_GAUGE_DEV)
    if T0[0] is not None:
        print("  wall time of this module so far: %.0f s" % (time.time() - T0[0]))
