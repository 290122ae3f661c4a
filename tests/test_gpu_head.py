"""The head kernel (csrc/nbe_kernels_head.h, conv_h3nz_kernel: conv_r01/conv_1, 64 -> 3, with the block's fused skip; one pass
along z, dz in the MFMA rows) against the float64 oracle, and its position independence.

Parity runs conv_r01 through the production schedule (nbe_test_block) the way test_gpu_blocks.run_case does: stage 2 is
conv_1 + skip on the hidden tensor the engine returned, every voxel held to the per-layer class of tests/layer_checks.py
(RTOL_L2 = 5e-6, RTOL_MAX = 1e-4).  Shapes are the smallest that reach every path of the kernel: one, two and three
16-channel chunks with a ragged or zero-padded last one (mid 64, 24, 8); 1, 2, 3 and 5 result planes (shorter than the
three-plane window of the running sum, and odd); 37 result planes, five more than the launcher's longest run of 32, so
that two runs of different length (19 and 18) meet; 9 x 33 outputs (one more than the 8 x 32 tile) and 5 x 7 (less than one
tile); one periodic-yx case."""

import numpy as np
import pytest

import test_gpu_blocks as TB
from oracle import layers as L

pytestmark = pytest.mark.gpu

ZRUN = 32                                                        # HNZ_ZRUN of csrc/nbe_kernels_head.h


@pytest.fixture(scope="module")
def engines(engine_factory):
    made = {}

    def get(mid):
        if mid not in made:
            e = engine_factory(mid_chan=mid, precision="f16x3", compute_vel=True)
            e.load_params(TB.params_of(mid), False)
            e.set_cosmology(TB.OM, TB.DZ)
            assert bool(e.query("gauge_active"))
            made[mid] = e
        return made[mid]
    return get


def _shape(planes, hv, wv):
    return (planes + 4, hv + 4, wv + 4, 0)


CASES = [(mid, _shape(n, *(yx[(i + j) % 2]))) for j, mid in enumerate((64, 24, 8))
         for i, n in enumerate((1, 2, 3, 5)) for yx in [((9, 33), (5, 7))]]
CASES += [(64, _shape(ZRUN + 5, 8, 32)),                          # runs of 19 and 18 planes, one tile wide
          (64, (6, 48, 56, 1)), (8, (6, 48, 56, 1))]             # periodic yx


@pytest.mark.parametrize("mid,shape", CASES, ids=["mid%d-%dx%dx%d-pad%d" % ((m,) + s) for m, s in CASES])
def test_head_against_oracle(engines, mid, shape):
    e = engines(mid)
    e.profile_enable(True)
    e.profile_reset()
    try:
        with L.backend('torch'):
            out = TB.run_case(e, 'conv_r01', mid, "f16x3", True, shape)
        prof = e.profile_read()
    finally:
        e.profile_enable(False)
    for r in out.values():
        assert "narrow" in r["paths"], r["paths"]
    assert any(p["kernel"].startswith("conv_h3n") for p in prof), [p["kernel"] for p in prof]


@pytest.mark.parametrize("mid", [64, 24])
def test_head_is_position_independent(engines, mid, monkeypatch):
    """NBE_WINO=0 (read per launch): the direct conv_0 is position independent, so the hidden tensors of a volume and of its
    sub-volumes agree bit for bit, and the head must give the same bits for a voxel wherever its tile and its run begin:
    37 result planes are runs of 19 + 18, 36 (z offset 1) of 18 + 18, 34 (z offset 3) of 17 + 17; the y / x offsets 3 and 5
    move every voxel to another row and column of its 8 x 32 tile."""
    monkeypatch.setenv("NBE_WINO", "0")
    e = engines(mid)
    rng = np.random.default_rng(mid)
    x = rng.standard_normal((mid, ZRUN + 9, 18, 42)).astype(np.float32)
    dx = rng.standard_normal(x.shape).astype(np.float32)
    full = e.test_block('conv_r01', x, dx=dx)
    assert "narrow" in full["paths"] and not full["paths"] & {"wino_0", "wino_1"}, full["paths"]
    for a, b, c in ((1, 3, 5), (3, 3, 5)):
        sub = e.test_block('conv_r01', np.ascontiguousarray(x[:, a:, b:, c:]), dx=np.ascontiguousarray(dx[:, a:, b:, c:]))
        assert "narrow" in sub["paths"]
        for k in ("h", "dh"):
            assert np.array_equal(sub[k], full[k][:, a:, b:, c:]), "hidden tensors differ in %s at offset %s" % (k, (a, b, c))
        for k in ("y", "dy"):
            assert sub[k].shape == full[k][:, a:, b:, c:].shape
            assert np.array_equal(sub[k], full[k][:, a:, b:, c:]), "%s depends on where the volume begins (offset %s)" % (k, (a, b, c))
