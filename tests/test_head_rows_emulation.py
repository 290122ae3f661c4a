"""CPU restatement, in float64, of the index arithmetic of the head kernel (csrc/nbe_kernels_head.h, conv_h3nz_kernel) and
of the packed weights it reads: 16-channel chunks, the packed layout [chunk][dz][tap][unit][16 couts][8 ch] of which rows
0-3 of every unit are kept ([chunk][dz][tap][unit][4]), the A operand row m = 4 dz + co, the 10 x 34 patch with its halo and
the tap pairs (0,1) (2,3) [4] (5,6) (7,8) as address shifts, lane group q of the 16x16x32 MFMA supplying channels
8 (q & 1) .. of tap q >> 1 of a pair, the accumulator of lane (c, q) holding rows 4 q .. 4 q + 3 of column c, the skip's
8 x 32 patch without halo in rows 0-3, and the running sum that moves one lane group up per input plane so that group 2
holds output plane p - 2 = (dz 0 + dz 1) + dz 2.  It must equal a direct 3x3x3 VALID convolution plus the 1x1x1 skip.

In float64 the lo parts of the f16x3 split are zero, so only the hi-part addresses carry numbers; the part pairing of the
odd tap ([wh|wl].[xl|xh] and [0|wh].[xl|xh]) is restated with them."""

import numpy as np
import pytest

ROWS, COLS = 8, 32
RS = COLS + 2
PL = (ROWS + 2) * RS
PP = (PL + 7) // 8 * 8
R = 4
TAPU = 4 * R
WG = 9 * TAPU
WC = 3 * WG
WS = 2 * TAPU
SP = ROWS * COLS
SH = {0: 0, 2: 2, 4: RS + 1, 5: RS + 2, 7: 2 * RS + 1}


def pack16(w):
    """launch_pack's narrow layout: [chunk][seg = 3 kz + ky][tap kx][u = 2 h + part][co 16][j 8], channel = 16 chunk + 8 h + j"""
    cout, cin, k = w.shape[0], w.shape[1], w.shape[2]
    nchunk = -(-cin // 16)
    nseg, taps = (9, 3) if k == 3 else (1, 1)
    out = np.zeros((nchunk, nseg, taps, 4, 16, 8))
    for ch in range(nchunk):
        for h in range(2):
            for j in range(8):
                ci = 16 * ch + 8 * h + j
                if ci < cin:
                    for seg in range(nseg):
                        for t in range(taps):
                            out[ch, seg, t, 2 * h, :cout, j] = w[:, ci, seg // 3, seg % 3, t] if k == 3 else w[:, ci, 0, 0, 0]
    return out.reshape(-1, 8)                                    # 16-byte units


def resident(packed, n):
    """rows 0-3 of every 16-row unit: LDS unit d <- packed unit (d >> 2) * 16 + (d & 3)"""
    d = np.arange(n)
    return packed[(d >> 2) * 16 + (d & 3)]


def planes16(x, chunk):
    """the four planes (u = 2 h + part) of a 16-channel chunk of x [C, D, H, W] as [4, D, H, W, 8]; lo parts are zero"""
    C = x.shape[0]
    out = np.zeros((4,) + x.shape[1:] + (8,))
    for h in range(2):
        for j in range(8):
            ci = 16 * chunk + 8 * h + j
            if ci < C:
                out[2 * h, ..., j] = x[ci]
    return out


def mfma(acc, A, B):
    """acc[c, q, e] (column c, row 4 q + e) += sum over lane groups q' and j of A[row][q'][j] * B[c][q'][j]"""
    D = np.einsum('mqj,nqj->mn', A, B)                           # [row m][column n]
    acc += D.T.reshape(16, 4, 4)


def head_emulated(w, ws, dws, beta, x, dx, xs, dxs, z0, zn, y0, x0):
    """one workgroup: output planes z0 .. z0 + zn - 1 of the 8 x 32 patch at (y0, x0); x, dx: [C, D, H, W] zero-padded so that
    the whole 10 x 34 patches exist; returns y, dy [3, zn, 8, 32]"""
    cin, cs = w.shape[1], ws.shape[1]
    nchunk, nskip = -(-cin // 16), -(-cs // 16)
    Lw = resident(pack16(w), nchunk * WC)
    Ls = np.concatenate([np.concatenate([resident(pack16(ws)[64 * sc:64 * sc + 64], TAPU),
                                         resident(pack16(dws)[64 * sc:64 * sc + 64], TAPU)]) for sc in range(nskip)])
    c = np.arange(16)
    arow = np.minimum(c >> 2, 2) * WG + (c & 3)
    y = np.zeros((3, zn, ROWS, COLS))
    dy = np.zeros_like(y)
    for rowp in range(ROWS):                                     # a wave
        ry, rd = np.zeros((2, 16, 4, 4)), np.zeros((2, 16, 4, 4))
        for p in range(zn + 2):
            ym, dm = np.zeros((2, 16, 4, 4)), np.zeros((2, 16, 4, 4))
            for k in range(nchunk):                              # stage (p, k): the staged patch, plane pitch PP
                X = np.zeros((2, 4 * PP, 8))
                for t, src in enumerate((x, dx)):
                    P4 = planes16(src, k)[:, z0 + p, y0:y0 + ROWS + 2, x0:x0 + COLS + 2]
                    for u in range(4):
                        X[t, u * PP:u * PP + PL] = P4[u].reshape(PL, 8)
                wb = k * WC

                def operands(tap0, pairstep):
                    A = np.zeros((16, 4, 8))
                    B = np.zeros((2, 2, 16, 4, 8))               # [tensor][nt]
                    for q in range(4):
                        kh, ks = q & 1, q >> 1
                        A[:, q] = Lw[wb + tap0 * TAPU + (ks * 4 + 2 * kh) * R + arow]
                        bB = (2 * kh) * PP + rowp * RS + c + SH[tap0] + pairstep * ks
                        for nt in range(2):
                            B[:, nt, :, q] = X[:, bB + 16 * nt]
                    return A, B
                for tap0, step in ((0, 1), (2, 32), (5, 32), (7, 1)):   # tap pairs: the second tap is 1 or 32 units on
                    A, B = operands(tap0, step)
                    for nt in range(2):
                        mfma(ym[nt], A, B[0, nt])
                        mfma(dm[nt], A, B[1, nt])
                A = np.zeros((16, 4, 8))                         # tap 4: [0|wh].[xl|xh]
                B = np.zeros((2, 2, 16, 4, 8))
                for q in range(4):
                    kh, ks = q & 1, q >> 1
                    if ks:
                        A[:, q] = Lw[wb + 4 * TAPU + (2 * kh) * R + arow]
                    bS1 = (2 * kh + 1 - ks) * PP + rowp * RS + c + SH[4]
                    for nt in range(2):
                        B[:, nt, :, q] = X[:, bS1 + 16 * nt]
                for nt in range(2):
                    mfma(ym[nt], A, B[0, nt])
                    mfma(dm[nt], A, B[1, nt])
            if p < zn:
                for sc in range(nskip):                          # the skip's 8 x 32 patch, plane pitch SP, rows 0-3 only
                    X = np.zeros((2, 4 * SP, 8))
                    for t, src in enumerate((xs, dxs)):
                        P4 = planes16(src, sc)[:, z0 + p, y0 + 1:y0 + 1 + ROWS, x0 + 1:x0 + 1 + COLS]
                        for u in range(4):
                            X[t, u * SP:(u + 1) * SP] = P4[u].reshape(SP, 8)
                    wb = sc * WS
                    A0, A0d = np.zeros((16, 4, 8)), np.zeros((16, 4, 8))
                    B = np.zeros((2, 2, 16, 4, 8))
                    for q in range(4):
                        kh, ks = q & 1, q >> 1
                        if ks:
                            A0[:R, q] = Ls[wb + (2 * kh) * R + (c[:R] & 3)]
                            A0d[:R, q] = Ls[wb + TAPU + (2 * kh) * R + (c[:R] & 3)]
                        bS1 = (2 * kh + 1 - ks) * SP + rowp * COLS + c
                        for nt in range(2):
                            B[:, nt, :, q] = X[:, bS1 + 16 * nt]
                    for nt in range(2):
                        mfma(ym[nt], A0, B[0, nt])
                        mfma(dm[nt], A0, B[1, nt])
                        mfma(dm[nt], A0d, B[0, nt])
            # retire plane p: R[q] <- R[q - 1] + T[q]; lane group 2 holds output plane p - 2
            for r_, t_ in ((ry, ym), (rd, dm)):
                sh = np.zeros_like(r_)
                sh[:, :, 1:] = r_[:, :, :-1]
                r_[...] = sh + t_
            if p >= 2:
                for nt in range(2):
                    for e in range(3):
                        yp = ry[nt, :, 2, e]
                        y[e, p - 2, rowp, 16 * nt:16 * nt + 16] = yp
                        dy[e, p - 2, rowp, 16 * nt:16 * nt + 16] = rd[nt, :, 2, e] + beta[e] * yp
    return y, dy


def direct(w, ws, dws, beta, x, dx, xs, dxs):
    """3x3x3 VALID convolution + the 1x1x1 skip on the centre (skip tensors have the geometry of x)"""
    D, H, W = x.shape[1:]
    y = np.zeros((w.shape[0], D - 2, H - 2, W - 2))
    dy = np.zeros_like(y)
    for kz in range(3):
        for ky in range(3):
            for kx in range(3):
                sl = (slice(None), slice(kz, kz + D - 2), slice(ky, ky + H - 2), slice(kx, kx + W - 2))
                y += np.einsum('oi,izyx->ozyx', w[:, :, kz, ky, kx], x[sl])
                dy += np.einsum('oi,izyx->ozyx', w[:, :, kz, ky, kx], dx[sl])
    c = (slice(None), slice(0, D - 2), slice(1, H - 1), slice(1, W - 1))
    y += np.einsum('oi,izyx->ozyx', ws[:, :, 0, 0, 0], xs[c])
    dy += np.einsum('oi,izyx->ozyx', ws[:, :, 0, 0, 0], dxs[c]) + np.einsum('oi,izyx->ozyx', dws[:, :, 0, 0, 0], xs[c])
    return y, dy + beta[:, None, None, None] * y


@pytest.mark.parametrize("cin", [8, 24, 64])
@pytest.mark.parametrize("zn", [1, 2, 5])
def test_rows_and_running_sum_equal_the_direct_convolution(cin, zn):
    """ragged patches: 11 x 37 outputs are two tile rows and two tile columns, the second of each 3 and 5 wide; the run
    starts at plane 1 of a tensor with zn + 1 output planes"""
    rng = np.random.default_rng(100 * cin + zn)
    Hv, Wv, z0 = 11, 37, 1
    Dv = z0 + zn
    cs = cin                                                     # conv_r01: the block input has the hidden tensor's channels
    w = rng.standard_normal((3, cin, 3, 3, 3)) / np.sqrt(27 * cin)          # fields of order one: the bound below is absolute
    ws, dws = rng.standard_normal((2, 3, cs, 1, 1, 1)) / np.sqrt(cs)
    beta = rng.standard_normal(3)
    x, dx = rng.standard_normal((2, cin, Dv + 2, Hv + 2, Wv + 2))
    xs, dxs = rng.standard_normal((2, cs, Dv + 2, Hv + 2, Wv + 2))   # pointers offset so that the centre tap is the skip's voxel
    y_o, dy_o = direct(w, ws, dws, beta, x, dx, xs, dxs)
    tny, tnx = -(-Hv // ROWS), -(-Wv // COLS)
    pad = lambda t: np.pad(t, ((0, 0), (0, 0), (0, tny * ROWS - Hv), (0, tnx * COLS - Wv)))   # what a ragged tile reads beyond the tensor
    xp, dxp, xsp, dxsp = pad(x), pad(dx), pad(xs), pad(dxs)
    y, dy = np.zeros_like(y_o), np.zeros_like(dy_o)
    for ty in range(tny):
        for tx in range(tnx):
            yt, dyt = head_emulated(w, ws, dws, beta, xp, dxp, xsp, dxsp, z0, zn, ty * ROWS, tx * COLS)
            hh, ww = min(ROWS, Hv - ty * ROWS), min(COLS, Wv - tx * COLS)
            y[:, z0:, ty * ROWS:ty * ROWS + hh, tx * COLS:tx * COLS + ww] = yt[:, :, :hh, :ww]
            dy[:, z0:, ty * ROWS:ty * ROWS + hh, tx * COLS:tx * COLS + ww] = dyt[:, :, :hh, :ww]
    assert np.abs(y_o[:, z0:]).max() > 1 and np.abs(dy_o[:, z0:]).max() > 1
    assert np.abs(y[:, z0:] - y_o[:, z0:]).max() <= 1e-12
    assert np.abs(dy[:, z0:] - dy_o[:, z0:]).max() <= 1e-12
