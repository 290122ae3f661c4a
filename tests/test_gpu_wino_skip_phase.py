"""The skip phase of conv_h3w_kernel (the fused 1x1x1 skip of a block's conv_1): its weights resident in LDS, its B operands
read straight from global memory.  Blocks go through the engine's block hook against the float64 oracle of
tests/block_ref.py, with the checks, tolerances and path assertions of test_gpu_blocks.run_case; the shapes are the
smallest on which the phase's addressing can go wrong:

* four result planes (two plane pairs) of 17 x 41 voxels -- not a multiple of the 8 x 32 tile, three tiles along y and two
  along x -- once padded (the input shrinks by 2 per side) and once periodic in y and x (the result keeps the input's size);
* every shape of the chunk loop: nskip 1 (conv_l00: 3 channels padded to 16, no tangent; mid 16), 2 (conv_r00 at mid 16, the
  sources switching at chunk 1), 3 (conv_r00 at mid 24: odd, through the loop and its tail), 4 (conv_l01 at mid 64) and 8
  (conv_r00 at mid 64, switching at chunk 4), i.e. chunks in both halves of the resident weight image;
* output channel counts that do not fill a 64-channel tile (mid 16, 24);
* the three forms of the kernel: f16x3 with velocity, displacement only, and the float16 model where its blocks fuse.

Position independence is checked bit for bit: the same block input embedded in a larger tensor, shifted by (2 planes, 3
rows, 5 columns), gives the same bits on the common voxels (the kernel pairs planes from the first one: an even shift along
z keeps the pairing; the surroundings repeat the input's own values, so the call's range shift is the same).  The
displacement-only form also pairs two blocks of eight rows in one workgroup, and its two accumulator sets sum their products
in different orders: there a row's bits depend on which block of a 16-row tile it falls into, in conv_0 as in conv_1, so that
form is shifted by 16 rows instead of 3."""

import numpy as np
import pytest

import block_ref as B
import test_gpu_blocks as TB
from test_gpu_blocks import engines  # noqa: F401  (the module-scoped engine cache, as a fixture of this module)
from oracle import layers as L

pytestmark = pytest.mark.gpu

PADDED, PERIODIC = (8, 21, 45, 0), (8, 17, 41, 1)                # (D, H, W, pad): a result of 4 planes x 17 x 41 either way

#        block       mid  arithmetic  velocity
CASES = [('conv_l00', 64, "f16x3", True),                         # nskip 1, F_SKIP_NODX
         ('conv_l01', 64, "f16x3", True),                         # nskip 4
         ('conv_r00', 64, "f16x3", True),                         # nskip 8, two sources switching at chunk 4
         ('conv_r00', 16, "f16x3", True),                         # nskip 2, switching at chunk 1; 16 output channels
         ('conv_r00', 24, "f16x3", True),                         # nskip 3 (odd); 24 output channels
         ('conv_l01', 24, "f16x3", True),                         # nskip 2 of 24 channels padded to 32
         ('conv_l00', 64, "f16x3", False),                        # displacement only: two row blocks per workgroup
         ('conv_l01', 64, "f16x3", False),
         ('conv_r00', 64, "f16x3", False),
         ('conv_r00', 24, "f16x3", False),
         ('conv_l01', 64, "f16", True),                           # the float16 model: 32-channel chunks, nskip 2
         ('conv_l01', 32, "f16", True),                           # nskip 1
         ('conv_r00', 32, "f16", True)]                           # nskip 2, switching at chunk 1


@pytest.mark.parametrize("shape", [PADDED, PERIODIC], ids=["padded", "periodic_yx"])
@pytest.mark.parametrize("block,mid,prec,vel", CASES)
def test_fused_skip_against_the_oracle(engines, block, mid, prec, vel, shape):  # noqa: F811
    e = engines(mid, prec, vel)
    with L.backend('torch'):
        out = TB.run_case(e, block, mid, prec, vel, shape)
    two = block in B.DECODERS and mid % (32 if prec == "f16" else 16) == 0
    assert set(out) == ({"cat", "two"} if two else {"cat"})
    for r in out.values():
        assert {"skip_fused", "wino_1"} <= r["paths"], r["paths"]     # the skip ran inside the Winograd-z kernel


def _embed(a, lead, trail):
    """a inside a larger tensor whose surroundings repeat a's own values (the same max |x|: the same range shift)"""
    return None if a is None else np.ascontiguousarray(np.pad(a, ((0, 0),) + tuple(zip(lead, trail)), mode='wrap'))


@pytest.mark.parametrize("block,mid,prec,vel,two,lead", [('conv_l01', 64, "f16x3", True, False, (2, 3, 5)),
                                                         ('conv_r00', 16, "f16x3", True, True, (2, 3, 5)),
                                                         ('conv_l00', 64, "f16x3", True, False, (2, 3, 5)),
                                                         ('conv_l01', 64, "f16x3", False, False, (2, 16, 5)),
                                                         ('conv_l01', 64, "f16", True, False, (2, 3, 5))])
def test_position_independence(engines, block, mid, prec, vel, two, lead):  # noqa: F811
    e = engines(mid, prec, vel)
    D, H, W, _ = PADDED
    g_in = B.gauges(TB.params_of(mid), TB.s64(), block, mid)[0]
    x, dxs = TB.make_input(block, mid, prec, vel, PADDED, g_in)
    trail = (0, 1, 3)
    X, DXS = _embed(x, lead, trail), _embed(dxs, lead, trail)
    assert np.abs(X).max() == np.abs(x).max()

    def run(a, da):
        if two:
            return e.test_block(block, a[:mid], dx=None if da is None else da[:mid], x2=a[mid:], dx2=None if da is None else da[mid:],
                                two_source=True)
        return e.test_block(block, a, dx=da)
    small, big = run(x, dxs), run(X, DXS)
    assert {"skip_fused", "wino_1"} <= small["paths"] and small["paths"] == big["paths"], (small["paths"], big["paths"])
    dz, dy, dx = lead
    for k, crop in (("h", 1), ("dh", 1), ("y", 2), ("dy", 2)):    # the hidden tensor shrinks by 1 per side, the result by 2
        if small[k] is None:
            continue
        n = small[k].shape
        common = big[k][:, dz:dz + n[1], dy:dy + n[2], dx:dx + n[3]]
        assert common.shape == n and n[2:] == (H - 2 * crop, W - 2 * crop)
        assert np.array_equal(common, small[k]), "%s %s: %d of %d values differ after the shift" % (
            block, k, int((common != small[k]).sum()), common.size)
