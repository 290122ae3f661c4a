"""Float64 oracle of ONE block of the U-Net as the engine runs it (nbe_test_block): pure NumPy on oracle.layers.

The engine stores every tangent in the gauge of the one 3x3x3 layer that reads the tensor, dx~ = dx + a (.) x with
a = alpha of that layer, and a residual block runs as two launches with a hidden tensor in between.
This module gives
  * the gauge of every tensor of the network from the parameters alone (GAUGE_IN / GAUGE_OUT below: the wiring written
    out, never read from the engine),
  * a stage-wise evaluation of a block on stored (gauged) tangents: stage 1 = conv_0 + activation -> hidden, stage 2 =
    conv_1 on a GIVEN hidden tensor + skip [+ activation] -> result, each one layer deep,
  * the sizes the network hands every block for an input of 8 k voxels per axis.

Weights come from a source: a style tree, modulated here (the functions' `params`), or a Premod -- the premodulated tree
of a style tree, whose float32 (W, dW) arrays are read as float64 and never modulated again, with the centred gauge table
the engine recovers from such pairs (centred below), again from the parameters alone.
"""

import numpy as np

from oracle import layers as L
from oracle.model import RESNET_BLOCKS, RESAMPLE_BLOCKS, BLOCK_SEQ

BLOCKS = ('conv_l00', 'conv_l01', 'down_l0', 'conv_l1', 'down_l1', 'conv_l2', 'down_l2', 'conv_c',
          'up_r2', 'conv_r2', 'up_r1', 'conv_r1', 'up_r0', 'conv_r00', 'conv_r01')
DECODERS = ('conv_r2', 'conv_r1', 'conv_r00')
LEVEL = {'conv_l00': 0, 'conv_l01': 0, 'down_l0': 0, 'up_r0': 0, 'conv_r00': 0, 'conv_r01': 0,
         'conv_l1': 1, 'down_l1': 1, 'up_r1': 1, 'conv_r1': 1,
         'conv_l2': 2, 'down_l2': 2, 'up_r2': 2, 'conv_r2': 2, 'conv_c': 3}

# ---- gauge table ------------------------------------------------------------------------------------------------------
# (consumer block, first channel, or None for gauge 0): the tensor is stored in the gauge alpha[first : first + C] of the
# consumer's conv_0.  'm' stands for mid_chan.
GAUGE_IN = {
    'conv_l00': None,                       # the input field has no tangent
    'conv_l01': ('conv_l01', 0), 'conv_l1': ('conv_l1', 0), 'conv_l2': ('conv_l2', 0), 'conv_c': ('conv_c', 0),
    'conv_r2': ('conv_r2', 0), 'conv_r1': ('conv_r1', 0), 'conv_r00': ('conv_r00', 0), 'conv_r01': ('conv_r01', 0),
    # the down-sampling layers read the encoder outputs, which are stored for the decoder blocks' first halves
    'down_l0': ('conv_r00', 0), 'down_l1': ('conv_r1', 0), 'down_l2': ('conv_r2', 0),
    # the up-sampling layers read conv_c / conv_r2 / conv_r1, whose outputs have gauge 0
    'up_r2': None, 'up_r1': None, 'up_r0': None,
}
GAUGE_OUT = {
    'conv_l00': ('conv_l01', 0),
    'conv_l01': ('conv_r00', 0), 'conv_l1': ('conv_r1', 0), 'conv_l2': ('conv_r2', 0),
    'down_l0': ('conv_l1', 0), 'down_l1': ('conv_l2', 0), 'down_l2': ('conv_c', 0),
    'up_r2': ('conv_r2', 'm'), 'up_r1': ('conv_r1', 'm'), 'up_r0': ('conv_r00', 'm'),
    'conv_r00': ('conv_r01', 0),
    'conv_c': None, 'conv_r2': None, 'conv_r1': None, 'conv_r01': None,
}
# the hidden tensor of a residual block is stored in the gauge of the block's own conv_1


def _tree(params):
    if isinstance(params, Premod):
        return params.style
    return params['params'] if 'params' in params else params


def alpha(lp, s):
    """alpha[ci] = (d s_mod / d Dz) / s_mod of a style-modulated layer, in the dtype of s"""
    dt = s.dtype
    sw, sb = np.asarray(lp['style_weight'], dtype=dt), np.asarray(lp['style_bias'], dtype=dt)
    return sw[:, 1] / (sw @ s + sb)


def channels(block, mid, in_chan=3, out_chan=3):
    """(cin, cmid, cout) of a block"""
    if block in RESAMPLE_BLOCKS:
        return mid, None, mid
    cin = in_chan if block == 'conv_l00' else 2 * mid if block in DECODERS else mid
    cout = out_chan if block == 'conv_r01' else mid
    return cin, max(cin, cout), cout


def gauges(params, s, block, mid):
    """(input, hidden, output) gauge vectors of a block's tensors in the dtype of s (hidden: None for a resampling block);
    of a Premod: the centred table"""
    p = _tree(params)
    cin, cmid, cout = channels(block, mid, p['conv_l00']['conv_0']['weight'].shape[1], p['conv_r01']['conv_1']['weight'].shape[0])

    def vec(rule, n):
        if rule is None:
            return np.zeros(n, s.dtype)
        off = mid if rule[1] == 'm' else rule[1]
        return al(p[rule[0]]['conv_0'], s)[off:off + n]
    al = (lambda lp, s: centred(lp, s, False, params.eps)[0]) if isinstance(params, Premod) else alpha
    hid = al(p[block]['conv_1'], s) if block in RESNET_BLOCKS else None
    return vec(GAUGE_IN[block], cin), hid, vec(GAUGE_OUT[block], cout)


def modulated(lp, s, first, eps=1e-8, half=False):
    """(W, dW, b) of a layer in float64 from the gauge form dW = W (.) (alpha[ci] + beta[co]); half: W as the float16
    engine stores it (W rounded to float16, the factors exact)."""
    w_n, dw_n = L.modulate_weights_vel(lp['style_weight'], lp['style_bias'], lp['weight'], s, first, eps)
    b = np.asarray(lp['bias'], dtype=s.dtype)
    if not half:
        return w_n, dw_n, b
    a, be = alpha(lp, s), beta(lp, s, first, eps)
    w16 = w_n.astype(np.float16).astype(s.dtype)
    return w16, w16 * (a[None, :, None, None, None] + be[:, None, None, None, None]), b


def beta(lp, s, first, eps=1e-8):
    """beta[co] of dW = W (.) (alpha[ci] + beta[co]): the derivative of the demodulation (+ 1 / Dz in the first layer)"""
    dt = s.dtype
    sw, sb = np.asarray(lp['style_weight'], dtype=dt), np.asarray(lp['style_bias'], dtype=dt)
    w0 = np.asarray(lp['weight'], dtype=dt)
    w = w0 * (sw @ s + sb)[None, :, None, None, None]
    dws = w0 * sw[:, 1][None, :, None, None, None]
    be = -np.sum(w * dws, axis=(1, 2, 3, 4)) / (np.sum(w * w, axis=(1, 2, 3, 4)) + dt.type(eps))
    return be + 1.0 / (s[1] + 1.0) if first else be


# ---- premodulated trees -------------------------------------------------------------------------------------------------
# The engine is handed float32 (W, dW) pairs and recovers dW = W (.) (alpha[ci] + beta[co]) from the numbers
# (wire_gauge_premod).  alpha + c, beta - c is the same pair for any constant c; the engine settles it by centring alpha on
# the middle of its range.  Every 3x3x3 layer whose input has a tangent is gauged: every conv_1, every conv_0 but conv_l00's.

def centred(lp, s, first=False, eps=1e-8):
    """(a_c, beta_c) = (alpha - mid, beta + mid), mid = (min alpha + max alpha) / 2: the gauge of a premodulated layer"""
    a, be = alpha(lp, s), beta(lp, s, first, eps)
    mid = 0.5 * (a.min() + a.max())
    return a - mid, be + mid


def gauged_layers():
    """[(block, layer)] of the layers whose (alpha, beta) the engine recovers from a premodulated tree"""
    return [(b, l) for b in BLOCKS if b in RESNET_BLOCKS for l in ('conv_0', 'conv_1') if (b, l) != ('conv_l00', 'conv_0')]


def _first(blk, lay):
    return blk == 'conv_l00' and lay in ('conv_0', 'skip')


class Premod:
    """The premodulated tree of a style tree at the style vector s, as a source of weights: .tree is what the engine loads
    (float32 as the package's modulate_emulator_parameters[_vel] returns it: weight, dweight with vel, bias), made layer by
    layer with oracle.layers.modulate_weights[_vel] in the dtype of s; .style is the style tree the gauge table comes from.
    The evaluation reads .tree as float64 and modulates nothing."""
    def __init__(self, params, s, vel=True, eps=1e-8, dtype=np.float32):
        """dtype: what the tree is cast to (float64: the arrays of the modulation itself, for identities to rounding)"""
        self.style, self.s, self.vel, self.eps = _tree(params), s, vel, eps
        tree = {}
        for blk, bp in self.style.items():
            for lay, lp in bp.items():
                leaf = {'bias': np.asarray(lp['bias'], dtype=dtype)}
                if vel:
                    w, dw = L.modulate_weights_vel(lp['style_weight'], lp['style_bias'], lp['weight'], s, _first(blk, lay), eps)
                    leaf['dweight'] = dw.astype(dtype)
                else:
                    w = L.modulate_weights(lp['style_weight'], lp['style_bias'], lp['weight'], s, eps)
                leaf['weight'] = w.astype(dtype)
                tree.setdefault(blk, {})[lay] = leaf
        self.tree = {'params': tree}

    def replaced(self, blk, lay, name, array):
        """the same source with one array of .tree replaced (a hand-made or perturbed pair: used as given)"""
        q = Premod.__new__(Premod)
        q.style, q.s, q.vel, q.eps = self.style, self.s, self.vel, self.eps
        q.tree = {'params': {b: {l: dict(lp) for l, lp in bp.items()} for b, bp in self.tree['params'].items()}}
        q.tree['params'][blk][lay][name] = np.asarray(array, dtype=self.tree['params'][blk][lay][name].dtype)
        return q


def recognise(w, dw, iters=200):
    """Float64 restatement of the engine's recognition of one premodulated (W, dW) pair (wire_gauge_premod): the
    alternating weighted least-squares fit of dW = W (.) (a[ci] + b[co]) from (0, 0) -- a from the current b, then b from the
    new a, until neither moves by 1e-13 or `iters` sweeps --, the element-wise residual max |dW - W (a + b)| with the largest
    |dW|, and the centring.  Returns a dict: alpha, beta (centred, float64), res, dmax, sweeps, amax = max centred alpha."""
    co, ci = w.shape[:2]
    W, D = np.asarray(w, np.float64).reshape(co, ci, -1), np.asarray(dw, np.float64).reshape(co, ci, -1)
    S, T = (W * W).sum(axis=2), (W * D).sum(axis=2)              # sums over the taps, per (o, i)
    den_a, den_b = S.sum(axis=0), S.sum(axis=1)
    a, b = np.zeros(ci), np.zeros(co)
    for sweep in range(1, iters + 1):
        an = np.where(den_a > 0, (T.sum(axis=0) - b @ S) / np.where(den_a > 0, den_a, 1.0), 0.0)
        bn = np.where(den_b > 0, (T.sum(axis=1) - S @ an) / np.where(den_b > 0, den_b, 1.0), 0.0)
        change = max(np.abs(an - a).max(), np.abs(bn - b).max())
        a, b = an, bn
        if change < 1e-13:
            break
    res = float(np.abs(D - W * (a[None, :, None] + b[:, None, None])).max())
    mid = 0.5 * (a.min() + a.max())
    return {'alpha': a - mid, 'beta': b + mid, 'res': res, 'dmax': float(np.abs(D).max()), 'sweeps': sweep,
            'amax': float(a.max() - mid)}


def recognition(premod):
    """recognise() over every gauged layer of a Premod: {(block, layer): its dict, with 'dev' = the largest deviation of the
    recovered (alpha, beta), stored as float32 as the engine stores them, from the centred float64 table}"""
    out = {}
    for blk, lay in gauged_layers():
        lp = premod.tree['params'][blk][lay]
        r = recognise(lp['weight'], lp['dweight'])
        a_c, b_c = centred(premod.style[blk][lay], premod.s, _first(blk, lay), premod.eps)
        f32 = lambda v: v.astype(np.float32).astype(np.float64)
        r['dev'] = float(max(np.abs(f32(r['alpha']) - a_c).max(), np.abs(f32(r['beta']) - b_c).max()))
        r['dev64'] = float(max(np.abs(r['alpha'] - a_c).max(), np.abs(r['beta'] - b_c).max()))
        out[(blk, lay)] = r
    return out


def _source(params, s, blk, lay):
    """(W, dW, b, beta) of a layer in float64 (dW None without velocity; beta a function, evaluated for gauged float16
    layers only): a style tree is modulated at s, a Premod's arrays are read as they are, with the centred beta"""
    first = _first(blk, lay)
    if isinstance(params, Premod):
        lp, ls = params.tree['params'][blk][lay], params.style[blk][lay]
        dt = s.dtype
        dw = np.asarray(lp['dweight'], dtype=dt) if 'dweight' in lp else None
        return np.asarray(lp['weight'], dtype=dt), dw, np.asarray(lp['bias'], dtype=dt), lambda: centred(ls, s, first, params.eps)[1]
    lp = _tree(params)[blk][lay]
    w, dw = L.modulate_weights_vel(lp['style_weight'], lp['style_bias'], lp['weight'], s, first)
    return w, dw, np.asarray(lp['bias'], dtype=s.dtype), lambda: beta(lp, s, first)


# ---- stage-wise evaluation --------------------------------------------------------------------------------------------

def _wrap(a, n):
    return None if a is None else np.pad(a, ((0, 0), (0, 0), (n, n), (n, n)), mode='wrap')


def _gx(g, x):
    return g[:, None, None, None] * x


def _act(p, dp, act, branch):
    if not act:
        return p, dp
    return L.leaky_relu_vel(p, dp, branch=branch)


class Stage:
    """One stage before its activation: pre-activation p with plain tangent dp.  result(branch) applies the activation (the
    tangent on the given branch; None: the oracle's own, p > 0) and returns (y, dy~) with dy~ = dy + g_out (.) y as stored."""
    def __init__(self, p, dp, act, g_out, vel):
        self.p, self.dp, self.act, self.g_out, self.vel = p, dp, act, g_out, vel

    def result(self, branch=None):
        if not self.vel:
            return (L.leaky_relu(self.p) if self.act else self.p), None
        y, dy = _act(self.p, self.dp, self.act, branch)
        return y, dy + _gx(self.g_out, y)


def _f16(a):
    return a.astype(np.float16).astype(np.float64)


def _layer(params, blk, lay, s, kind, x, dxs, g_in, vel, half, gauged):
    """y and the PLAIN output tangent of one layer on the STORED input tangent dxs = dx + g_in (.) x (None: no tangent).
    half: the operands as the float16 engine stores them -- W rounded to float16; a gauged 3x3x3 layer (its input is
    stored in its own alpha) computes W.dx~ + beta (.) (W.x) from that same W; every other layer keeps a tangent weight of
    its own with the input's gauge folded in, dW - W (.) g_in, rounded to float16.
    A Premod is stored the same way (load_weights, fold and pack_wino of csrc/nbe_engine_weights.cpp): the tree's float32
    W packed to float16; a gauged layer's tangent weight is W16 (.) beta_c, its float32 dW never read; every other layer
    f16(dW - W (.) g_in) with the centred g_in -- the skips and the down-sampling layers folded on the host from the float32
    W, the up-sampling layers and conv_l00's (g_in = 0) packed as they come; and since such a tree fuses no skip on the
    float16 model, each skip is read back as a float16 residual (stage2, fused = False)."""
    w, dw, b, be = _source(params, s, blk, lay)
    if half:
        w16 = _f16(w)
    if not vel:
        return L.conv_layer(kind, x, w16 if half else w, b), None
    if not half:
        return L.conv_layer_vel(kind, x, plain(dxs, g_in, x), w, dw, b)
    if gauged and kind == 'conv3' and dxs is not None:
        dwt = w16 * be()[:, None, None, None, None]
    else:
        dwt = _f16(dw - w * g_in[None, :, None, None, None])
    return L.conv_layer_vel(kind, x, dxs, w16, dwt, b)


def plain(dxs, g, x):
    """stored tangent -> plain tangent"""
    return None if dxs is None else dxs - _gx(g, x)


def stage1(params, s, block, x, dxs, mid, pad=0, vel=True, half=False, g=None, gauged=True):
    """hidden = act(conv_0(x)) of a residual block, or the whole resampling block; x float64, dxs the STORED input tangent
    (None: conv_l00 / displacement only); g: the (input, hidden, output) gauges in place of the table's, with gauged =
    False for an engine that stores plain tangents and runs three products per layer (NBE_GAUGE=0)."""
    g_in, g_hid, g_out = g or gauges(params, s, block, mid)
    if not vel:
        dxs = None
    if block in RESAMPLE_BLOCKS:
        pp, dpp = _layer(params, block, 'conv_0', s, 'down' if block.startswith('down') else 'up', x, dxs, g_in, vel, half, gauged)
        return Stage(pp, dpp, True, g_out, vel)
    if pad:
        x, dxs = _wrap(x, 2), _wrap(dxs, 2)
    pp, dpp = _layer(params, block, 'conv_0', s, 'conv3', x, dxs, g_in, vel, half, gauged)
    if pad:                                              # the hidden tensor's interior
        pp, dpp = pp[:, :, 1:-1, 1:-1], (None if dpp is None else dpp[:, :, 1:-1, 1:-1])
    return Stage(pp, dpp, True, g_hid, vel)


def stage2(params, s, block, x, dxs, h, dhs, mid, pad=0, vel=True, half=False, g=None, gauged=True, fused=True):
    """result = [act](conv_1(h) + skip(crop(x))) on a GIVEN hidden tensor h with stored tangent dhs.  half and not fused:
    the float16 engine runs the skip as a launch of its own, whose result conv_1 reads back as a float16 residual."""
    g_in, g_hid, g_out = g or gauges(params, s, block, mid)
    if not vel:
        dxs = dhs = None
    if pad:
        h, dhs = _wrap(h, 1), _wrap(dhs, 1)
        crop = lambda a: None if a is None else a[:, 2:-2]
    else:
        crop = lambda a: None if a is None else a[:, 2:-2, 2:-2, 2:-2]
    pp, dpp = _layer(params, block, 'conv_1', s, 'conv3', h, dhs, g_hid, vel, half, gauged)
    ps, dps = _layer(params, block, 'skip', s, 'skip', crop(x), crop(dxs), g_in, vel, half, gauged)
    if half and not fused:
        ps, dps = _f16(ps), (None if dps is None else _f16(dps))
    pp = pp + ps
    if vel:
        dpp = dpp + dps
    return Stage(pp, dpp, BLOCK_SEQ[block][-1] == 'A', g_out, vel)


def block(params, s, name, x, dxs, mid, pad=0, vel=True):
    """both stages chained on the oracle's own hidden tensor: (y, stored dy)"""
    h, dhs = stage1(params, s, name, x, dxs, mid, pad, vel).result()
    if name in RESAMPLE_BLOCKS:
        return h, dhs
    return stage2(params, s, name, x, dxs, h, dhs, mid, pad, vel).result()


# ---- the sizes the network hands its blocks -----------------------------------------------------------------------------

def input_size(block, k):
    """extent per axis of the block's input for a network input of 8 k >= 104 voxels per axis"""
    return {'conv_l00': 8 * k, 'conv_l01': 8 * k - 4, 'down_l0': 8 * k - 8,
            'conv_l1': 4 * k - 4, 'down_l1': 4 * k - 8,
            'conv_l2': 2 * k - 4, 'down_l2': 2 * k - 8,
            'conv_c': k - 4, 'up_r2': k - 8,
            'conv_r2': 2 * (k - 8), 'up_r1': 2 * (k - 10),
            'conv_r1': 4 * (k - 10), 'up_r0': 4 * (k - 11),
            'conv_r00': 8 * (k - 11), 'conv_r01': 8 * (k - 11) - 4}[block]


def output_size(block, n):
    return n // 2 if block.startswith('down') else 2 * n if block.startswith('up') else n - 4
