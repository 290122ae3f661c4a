"""Per-layer tolerances and checks shared by the layer-level and the block-level GPU parity tests (test_gpu_layers.py,
test_gpu_blocks.py).  One layer of at most K = 27 * 128 + 128 products per output is held to these; where they come from
is written in test_gpu_layers.py's docstring."""

import numpy as np

from conftest import rel_l2, max_over_rms

RTOL_L2 = 5e-6
RTOL_MAX = 1e-4


RTOL_L2_F16 = 5e-4
RTOL_MAX_F16 = 5e-3


def _chk(got, want, what, half=False):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert np.all(np.isfinite(got)), what
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    t2, tm = (RTOL_L2_F16, RTOL_MAX_F16) if half else (RTOL_L2, RTOL_MAX)
    assert e2 <= t2 and em <= tm, "%s: rel_l2=%.3e max/rms=%.3e" % (what, e2, em)


# the float16 model's Winograd-z form: U_xi and V = a +- b are rounded to float16 once more (measured: 4.6e-4 / 3.9e-3;
# the direct kernel on the same operands 2.1e-4)
RTOL_L2_F16W = 7e-4
RTOL_MAX_F16W = 7e-3


def _chk_f16w(got, want, what, pre=None, dpre=None):
    """pre / dpre: the oracle's pre-activation value and tangent.  The tangent of LeakyReLU jumps by a factor of 100 where
    the value changes sign, and this form's value carries ~3e-4 of rounding before the activation: voxels whose oracle
    pre-activation lies within 1e-2 RMS of zero may take either branch (each within the plain tolerance of that branch);
    every other voxel meets the plain tolerances."""
    assert got.shape == want.shape and np.all(np.isfinite(got)), what
    if pre is not None:
        rms = float(np.sqrt(np.mean(want.astype(np.float64) ** 2)))
        near = np.abs(pre) <= 1e-2 * float(np.sqrt(np.mean(pre ** 2)))
        either = np.minimum(np.abs(got - dpre), np.abs(got - 0.01 * dpre))
        assert float(either[near].max(initial=0.0)) <= RTOL_MAX_F16W * rms, "%s: a voxel at the kink on neither branch" % what
        got, want = got[~near], want[~near]
    e2, em = rel_l2(got, want), max_over_rms(got, want)
    assert e2 <= RTOL_L2_F16W and em <= RTOL_MAX_F16W, "%s: rel_l2=%.3e max/rms=%.3e" % (what, e2, em)
    return e2, em


def _h(a, half):
    """operand as the float16 engine sees it"""
    return a if (a is None or not half) else a.astype(np.float16).astype(np.float32)
