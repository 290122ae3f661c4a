"""The block-level oracle (tests/block_ref.py) against the oracle of the whole model: CPU only."""

import numpy as np
import pytest

import block_ref as B
from oracle import layers as L, model as M, params as P

OM, DZ = 0.27, 0.7731811501855036


def _case(block, mid, rng, n=9):
    cin, _, _ = B.channels(block, mid)
    d = (8, 8, 10) if block.startswith('down') else (4, 5, 6) if block.startswith('up') else (n - 2, n, n + 1)
    x = rng.standard_normal((cin,) + d)
    dx = None if block == 'conv_l00' else rng.standard_normal((cin,) + d)
    return x, dx


@pytest.mark.parametrize("mid", [8, 16])
@pytest.mark.parametrize("block", B.BLOCKS)
def test_stagewise_gauged_evaluation_is_the_model_block(block, mid):
    """stage 1 + stage 2 on stored tangents, un-gauged = oracle.model's block on plain tangents, to 1e-12"""
    p = P.synthetic_params(seed=11, mid_chan=mid)
    s = L.style_vector(OM, DZ)
    rng = np.random.default_rng(mid + len(block))
    x, dx = _case(block, mid, rng)
    g_in, g_hid, g_out = B.gauges(p, s, block, mid)
    dxs = None if dx is None else dx + g_in[:, None, None, None] * x
    W = M._Weights(p, False, True, s, np.float64, 1e-8)
    W.branch_hook = None
    for pad in ((0,) if block in M.RESAMPLE_BLOCKS else (0, 1)):
        y, dys = B.block(p, s, block, x, dxs, mid, pad=pad)
        xx, dd = (x, dx) if not pad else (B._wrap(x, 2), B._wrap(dx, 2))
        if block in M.RESAMPLE_BLOCKS:
            y_o, dy_o = M.resample_block(W, True, block, xx.copy(), dd.copy())
        else:
            y_o, dy_o = M.resnet_block(W, True, block, xx.copy(), None if dd is None else dd.copy())
        dy = dys - g_out[:, None, None, None] * y
        assert y.shape == y_o.shape
        assert np.abs(y - y_o).max() <= 1e-12 * np.abs(y_o).max()
        assert np.abs(dy - dy_o).max() <= 1e-12 * max(np.abs(dy_o).max(), np.abs(dys).max())


@pytest.mark.parametrize("mid", [8, 16, 24, 32, 64])
def test_gauge_table_reproduces_the_tangent_weights(mid):
    """dW of modulate_weights_vel = W (.) (alpha[ci] + beta[co]) with alpha from the parameters alone"""
    p = P.synthetic_params(seed=3, mid_chan=mid)
    s = L.style_vector(OM, DZ)
    worst = amax = 0.0
    for blk, bp in p['params'].items():
        for lay, lp in bp.items():
            first = blk == 'conv_l00' and lay in ('conv_0', 'skip')
            w, dw = L.modulate_weights_vel(lp['style_weight'], lp['style_bias'], lp['weight'], s, first)
            a, be = B.alpha(lp, s), B.beta(lp, s, first)
            amax = max(amax, float(np.abs(a).max()))
            err = np.abs(dw - w * (a[None, :, None, None, None] + be[:, None, None, None, None])).max() / np.abs(dw).max()
            worst = max(worst, float(err))
            w16, dw16, _ = B.modulated(lp, s, first, half=True)
            assert np.array_equal(w16, w.astype(np.float16).astype(np.float64))
            assert np.abs(dw16 - dw).max() <= 2.0 ** -10 * np.abs(dw).max() * 4
    print("mid %d: worst |dW - W (alpha + beta)| / max|dW| = %.2e, max |alpha| = %.2f" % (mid, worst, amax))
    assert worst <= 1e-12


def test_gauge_wiring_is_consistent():
    """a tensor's gauge is the same seen from its producer and from its consumer, along the wiring of the U-Net"""
    mid = 16
    p = P.synthetic_params(seed=5, mid_chan=mid)
    s = L.style_vector(OM, DZ)
    g = {b: B.gauges(p, s, b, mid) for b in B.BLOCKS}
    m = mid
    for prod, cons, sl in [('conv_l00', 'conv_l01', slice(0, m)), ('conv_l01', 'down_l0', slice(0, m)), ('conv_l01', 'conv_r00', slice(0, m)),
                           ('down_l0', 'conv_l1', slice(0, m)), ('conv_l1', 'down_l1', slice(0, m)), ('conv_l1', 'conv_r1', slice(0, m)),
                           ('down_l1', 'conv_l2', slice(0, m)), ('conv_l2', 'down_l2', slice(0, m)), ('conv_l2', 'conv_r2', slice(0, m)),
                           ('down_l2', 'conv_c', slice(0, m)), ('conv_c', 'up_r2', slice(0, m)), ('up_r2', 'conv_r2', slice(m, 2 * m)),
                           ('conv_r2', 'up_r1', slice(0, m)), ('up_r1', 'conv_r1', slice(m, 2 * m)), ('conv_r1', 'up_r0', slice(0, m)),
                           ('up_r0', 'conv_r00', slice(m, 2 * m)), ('conv_r00', 'conv_r01', slice(0, m))]:
        assert np.array_equal(g[prod][2], g[cons][0][sl]), (prod, cons)
    assert not g['conv_r01'][2].any() and not g['conv_l00'][0].any()


@pytest.mark.parametrize("n", [104, 112])
def test_production_shape_table_matches_the_model(n):
    """block_ref.input_size / output_size against the activation shapes of oracle.model.forward"""
    mid = 8
    p = P.synthetic_params(seed=3, mid_chan=mid)
    seen = {}

    def hook(name, pre):
        seen[name] = pre.shape[1:]
        return None
    x = np.random.default_rng(1).standard_normal((1, 3, n, n, n)).astype(np.float32)
    with L.backend('torch'):
        d, v = M.forward(p, x, OM, DZ, 1.0, dtype=np.float32, branch_hook=hook)
    k = n // 8
    for b in B.BLOCKS:
        ni = B.input_size(b, k)
        if b in M.RESAMPLE_BLOCKS:
            assert seen[b + '/conv_0'] == (B.output_size(b, ni),) * 3, b
        else:
            assert seen[b + '/conv_0'] == (ni - 2,) * 3, b
            if b != 'conv_r01':
                assert seen[b + '/conv_1'] == (B.output_size(b, ni),) * 3, b
    assert d.shape[2:] == (B.output_size('conv_r01', B.input_size('conv_r01', k)),) * 3 == (n - 96,) * 3


# ---- premodulated trees (block_ref.Premod) ------------------------------------------------------------------------------

@pytest.mark.parametrize("mid", [8, 16])
@pytest.mark.parametrize("block", B.BLOCKS)
def test_premodulated_evaluation_is_the_style_one(block, mid):
    """the stage-wise evaluation chained over a block, on the arrays of a premodulated tree (kept in float64) with tangents
    stored in the centred gauges, un-gauged = the style evaluation with the style gauges, to 1e-12"""
    p = P.synthetic_params(seed=11, mid_chan=mid)
    s = L.style_vector(OM, DZ)
    pm = B.Premod(p, s, dtype=np.float64)
    rng = np.random.default_rng(mid + len(block))
    x, dx = _case(block, mid, rng)
    gs, gp = B.gauges(p, s, block, mid), B.gauges(pm, s, block, mid)
    if B.GAUGE_IN[block] is not None:
        assert np.abs(gs[0] - gp[0]).max() > 1e-3                # the two tables do differ: by the centre of the reader's alpha
        assert np.ptp(gs[0] - gp[0]) <= 1e-15
    put = lambda g: None if dx is None else dx + g[:, None, None, None] * x
    for pad in ((0,) if block in M.RESAMPLE_BLOCKS else (0, 1)):
        y_s, dys_s = B.block(p, s, block, x, put(gs[0]), mid, pad=pad)
        y_p, dys_p = B.block(pm, s, block, x, put(gp[0]), mid, pad=pad)
        dy_s, dy_p = dys_s - gs[2][:, None, None, None] * y_s, dys_p - gp[2][:, None, None, None] * y_p
        assert np.abs(y_p - y_s).max() <= 1e-12 * np.abs(y_s).max()
        assert np.abs(dy_p - dy_s).max() <= 1e-12 * max(np.abs(dy_s).max(), np.abs(dys_s).max(), np.abs(dys_p).max())
    # displacement only: the tree of the plain modulation gives the same primal
    y_d, none = B.block(B.Premod(p, s, vel=False, dtype=np.float64), s, block, x, None, mid, vel=False)
    assert none is None and np.abs(y_d - B.block(p, s, block, x, None, mid, vel=False)[0]).max() <= 1e-12 * np.abs(y_s).max()


@pytest.mark.parametrize("shift", [0.0, 0.37, -5.0, "centre"])
def test_gauge_shift_leaves_the_plain_tangent_unchanged(shift):
    """a gauged layer computes W.dx~ + beta (.) (W.x) on dx~ = dx + alpha (.) x: (alpha + c, beta - c) is the same layer for
    every constant c -- the centring of a premodulated tree among them -- and gives the tangent of (W, dW)"""
    mid = 8
    p = P.synthetic_params(seed=7, mid_chan=mid)
    s = L.style_vector(OM, DZ)
    rng = np.random.default_rng(2)
    for blk, lay in B.gauged_layers():
        lp = p['params'][blk][lay]
        w, dw = L.modulate_weights_vel(lp['style_weight'], lp['style_bias'], lp['weight'], s, False)
        a, be = B.alpha(lp, s), B.beta(lp, s, False)
        if shift == "centre":
            a_c, be_c = B.centred(lp, s)
            c = a_c[0] - a[0]
            assert np.abs(a + c - a_c).max() <= 1e-15 and np.abs(be - c - be_c).max() <= 1e-15
            assert abs(a_c.min() + a_c.max()) <= 1e-15
        else:
            c = shift
        x, dx = rng.standard_normal((2, w.shape[1], 4, 5, 6))
        _, dy = L.conv_layer_vel('conv3', x, dx, w, dw, np.zeros(w.shape[0]))
        dxs = dx + (a + c)[:, None, None, None] * x
        got = L.conv3(dxs, w) + (be - c)[:, None, None, None] * L.conv3(x, w)
        assert np.abs(got - dy).max() <= 1e-12 * max(np.abs(dy).max(), np.abs(dxs).max()), (blk, lay)


def test_recognition_restated_reproduces_the_centred_table():
    """block_ref.recognise -- the engine's alternating fit, its element-wise check and its centring, in NumPy float64 -- on the
    float32 pair of every gauged layer of the trees tests/test_gpu_blocks_premod.py loads: the fit converges well inside the
    200 sweeps, every pair passes the 2e-6 max|dW| acceptance and the |alpha| <= 64 rule (so the engine must run gauged), and
    the result is the centred table of the parameters.  Bound on that: an element of dW / W carries at most 2 * 2^-24
    (alpha + beta) of float32 rounding, a weighted mean of such errors no more, twice that for the coupling of the two fits,
    and 2^-24 max(|alpha|, |beta|) for the float32 the engine stores.  The perturbed pair of the fall-back cases fails the
    acceptance."""
    import test_gpu_blocks_premod as TP
    worst = 0.0
    for mid in TP.MIDS:
        pm = TP.premod_of(mid)
        R = B.recognition(pm)
        assert set(R) == set(B.gauged_layers()) and len(R) == 17
        for (blk, lay), r in R.items():
            a_c, b_c = B.centred(pm.style[blk][lay], pm.s)
            bound = 4 * 2.0 ** -24 * np.abs(a_c[None, :] + b_c[:, None]).max() + 2.0 ** -24 * max(np.abs(a_c).max(), np.abs(b_c).max())
            assert r['sweeps'] < 100, (mid, blk, lay, r['sweeps'])
            assert r['res'] <= 2e-6 * r['dmax'] and r['amax'] <= 64.0, (mid, blk, lay, r['res'] / r['dmax'], r['amax'])
            assert r['dev'] <= bound, (mid, blk, lay, r['dev'], bound)
            worst = max(worst, r['dev'])
        print("mid %d: sweeps <= %d, residual <= %.2e max|dW| (accepted under 2e-6), max |alpha| %.3f, deviation %.2e (%.2e before the float32 store)" % (
            mid, max(r['sweeps'] for r in R.values()), max(r['res'] / r['dmax'] for r in R.values()), max(r['amax'] for r in R.values()),
            max(r['dev'] for r in R.values()), max(r['dev64'] for r in R.values())))
        blk, lay = TP.BAD[:2]
        bad = TP.perturbed_of(mid).tree['params'][blk][lay]
        r = B.recognise(bad['weight'], bad['dweight'])
        assert r['res'] > 100 * 2e-6 * r['dmax'], (mid, r['res'] / r['dmax'])
    assert worst == TP.PREMOD_GAUGE_DEV
    print("PREMOD_GAUGE_DEV = %.3e" % TP.PREMOD_GAUGE_DEV)
