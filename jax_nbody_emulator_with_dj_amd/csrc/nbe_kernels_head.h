// Included by nbe_kernels_h3.hip (uses its patch constants, dma16s, split4, xcd_tile).
//
// conv_h3nz_kernel: the head convolution conv_r01/conv_1 (64 -> 3, style_nbody_emulator_vel_core.py:178-186) with the block's
// fused 1x1x1 skip: f16x3, velocity, gauged input tangent, at most FOUR output channels.
//
// The kernel it replaces gave a workgroup four output planes of an 8 x 32 patch: per 16-channel chunk it staged six input
// planes (1.5 per output plane), staged the skip's patch with a halo nobody read, and spent a 16-row MFMA tile on 3 couts,
// once per dz -- 360 MFMAs per 16 voxels, 1.72 KB of L2 -> LDS traffic per voxel.  Two changes:
//
// ONE PASS ALONG z.  A workgroup owns one 8 x 32 patch and a RUN of zn consecutive output planes (the launcher picks the
// run length, at most HNZ_ZRUN).  It walks the zn + 2 input planes of the run once; a stage is (input plane, chunk), its
// 10 x 34 patch (x and dx~, 44 KB) is staged exactly once.  The skip of output plane p is staged as one stage per chunk
// of the block input, 8 x 32 centre only (32 KB), after the main stages of input plane p.
//
// dz IN THE MFMA ROWS.  Row m = 4 dz + co of the A operand holds W[co, :, dz, ky, kx]: one set of products on input plane p
// yields, for every voxel of the patch, that plane's contribution to the output planes p (rows 0-3), p - 1 (rows 4-7) and
// p - 2 (rows 8-11) -- a third of the MFMAs of one product set per dz, and no second staging of anything.  Lane group
// q = lane >> 4 of an accumulator holds rows 4 q .. 4 q + 3, i.e. exactly the dz = q rows.  When the stages of plane p are
// done its (main + 2^-11 correction) sums T_p are folded into a running register R that moves one lane group up per plane,
//     R[q] <- R[q - 1] + T_p[q]   (R[-1] = 0),
// so that group q = 2 then holds (T_{p-2}[dz 0] + T_{p-1}[dz 1]) + T_p[dz 2] = output plane p - 2, complete; its 16 lanes
// run the epilogue (bias, beta . (W.x), LeakyReLU, gauge, split4) and store 16 bytes per voxel and part.  The skip's
// products go into rows 0-3 of plane p's accumulators (rows >= 4 of its A operands are zeroed), tap-4 part pairing as before.
//
// Weights: the layer's packing is unchanged ([chunk][dz][tap][unit][16 couts][8 ch], cout_t = 16).  Only rows 0-3 of each
// 16-row unit are real, and only they are copied to LDS, once per workgroup: 432 units per chunk, 27 KB for 64 channels,
// resident for the whole run, plus 32 units per skip chunk.  Lane c of an A operand reads row c & 3 of group dz = c >> 2.
//
// Position independence: every output voxel sums the same products in the same order -- per input plane chunk 0 .. n - 1
// (nine taps each in the fixed pair order), then the skip chunks, then (dz 0 + dz 1) + dz 2 -- wherever its run, tile or
// launch begins.
//
// One barrier per stage; stage s + 1 is fetched by global -> LDS DMA at the start of stage s into the other patch buffer.
// MFMAs are compiler intrinsics, so the VALU -> MFMA hazards are the compiler's.
// Resources (hipcc --offload-arch=gfx950 -O3 -Rpass-analysis=kernel-resource-usage): 172 VGPRs, 0 AGPRs, 102 SGPRs,
// scratch 0, no spills; LDS 117,760 B, all dynamic (one workgroup of 8 waves per CU).
constexpr int HNZ_ZRUN = 32;                                    // longest run of output planes of one workgroup
// (HNZ_MAXCH, at most 64 input channels and 64 of the block input, and HNZ_R, the weight rows kept per 16-row unit: nbe_conv_select.h)
constexpr int HNZ_TAPU = 4 * HNZ_R;                             // units per tap: 2 channel halves x hi/lo x 4 rows
constexpr int HNZ_WG = 9 * HNZ_TAPU;                            // one (chunk, dz) group: 144 units
constexpr int HNZ_WC = 3 * HNZ_WG;                              // a chunk: 432 units
constexpr int HNZ_WS = 2 * HNZ_TAPU;                            // a skip chunk: [W_s | dW_s~]: 32 units
constexpr int HNZ_SBASE = HNZ_MAXCH * HNZ_WC;                   // 1728
constexpr int HNZ_XBASE = HNZ_SBASE + HNZ_MAXCH * HNZ_WS;       // 1856
constexpr int HNZ_LDS_UNITS = HNZ_XBASE + 2 * HQ_XB;            // 7360 units = 117,760 B
constexpr int HNZ_SP = HP_ROWS * HP_COLS;                       // plane pitch of the skip's 8 x 32 patch
static_assert(8 * HNZ_SP <= HQ_XB, "the skip's patch fits a patch buffer");

__global__ __launch_bounds__(512, 1) void conv_h3nz_kernel(ConvKArgs a) {
    constexpr int R = HNZ_R, TAPU = HNZ_TAPU, WG = HNZ_WG, WC = HNZ_WC, XBASE = HNZ_XBASE, NT = 2, NW = 8;
    f32x4* lds = lds_h3;
    const half8* L8 = (const half8*)lds_h3;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int c = lane & 15, q = lane >> 4, kh = q & 1, ks = q >> 1;

    // tiles: runs fastest (neighbours along z share two input planes through the XCD's L2)
    const int nrun = (a.Dv + a.zrun - 1) / a.zrun;
    const int tile = xcd_tile(blockIdx.x, a.ntiles);
    const int zr = tile % nrun, tyx = tile / nrun;
    const int ty = tyx / a.tnx, tx = tyx - ty * a.tnx;
    const int y0 = ty * HP_ROWS, x0 = tx * HP_COLS, z0 = zr * a.zrun;
    const int zn = min(a.zrun, a.Dv - z0);                       // output planes of this run
    const int nchunk = a.nchunk, nskip = a.nskip;
    const long plane = (long)a.H * a.W * 16;
    const long to = (((long)z0 * a.H + y0) * a.W + x0) * 16;

    // per-lane offsets of the patch DMA.  Main: 24 wave-instructions per tensor (4 planes x 6), three per wave.
    // Skip: 16 per tensor (4 planes x 4 pairs of rows), two per wave, both on row pair wave & 3.
    unsigned xoff[3];
    bool xval[3];
#pragma unroll
    for (int t = 0; t < 3; ++t) {
        const int k = (wave + NW * t) % 6;
        const int u = k * 64 + lane;
        xval[t] = u < HP_PL;
        const int uu = xval[t] ? u : HP_PL - 1;
        const int row = uu / HP_RS, col = uu - row * HP_RS;
        xoff[t] = (unsigned)(row * a.W + col) * 16u;
    }
    const unsigned soff = (unsigned)((2 * (wave & 3) + (lane >> 5) + 1) * a.W + (lane & 31) + 1) * 16u;
    // stage (input plane p, k): k < nchunk a chunk of the layer input (a.gs[k] = its planes at z = 0), else chunk k - nchunk of the skip
    auto fetch = [&](int p, int k, int buf) {
        const ConvGroupSrc e = a.gs[k];
        const char* xs = e.x + to + (long)p * plane;
        const char* dxs = e.dx + to + (long)p * plane;
        f32x4* xb = lds + XBASE + buf * HQ_XB;
        if (k < nchunk) {
#pragma unroll
            for (int t = 0; t < 3; ++t) {
                const int n = wave + NW * t, pl = n / 6, kk = n - 6 * pl;
                if (xval[t]) {
                    dma16s(xs + (long)pl * e.psb, xoff[t], xb + pl * HQ_PP + kk * 64);
                    dma16s(dxs + (long)pl * e.psb, xoff[t], xb + HQ_XT + pl * HQ_PP + kk * 64);
                }
            }
        } else {
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                const int n = wave + NW * t, pl = n >> 2, kk = n & 3;
                dma16s(xs + (long)pl * e.psb, soff, xb + pl * HNZ_SP + kk * 64);
                dma16s(dxs + (long)pl * e.psb, soff, xb + 4 * HNZ_SP + pl * HNZ_SP + kk * 64);
            }
        }
    };

    // ---- resident weights: rows 0-3 of every 16-row unit of the packed layer (unit d of LDS <- unit (d >> 2) * 16 + (d & 3))
    {
        const int nmain = nchunk * WC;
        for (int n = wave; n * 64 < nmain; n += NW) {
            const int d = n * 64 + lane;
            if (d < nmain) dma16((const float*)((const char*)a.w + ((long)(d >> 2) * 16 + (d & 3)) * 16), lds + n * 64);
        }
        const int nsk = nskip * HNZ_WS;                          // [chunk][W_s | dW_s~][unit][row]
        for (int n = wave; n * 64 < nsk; n += NW) {
            const int d = n * 64 + lane, sc = d >> 5, set = (d >> 4) & 1, r = d & 15;
            if (d < nsk)
                dma16((const float*)((const char*)a.ws + (set ? a.dws_delta : 0) + ((long)sc * 64 + (r >> 2) * 16 + (r & 3)) * 16),
                      lds + HNZ_SBASE + n * 64);
        }
    }

    f32x4 ym[NT], yc[NT], dm[NT], dc[NT];                        // input plane p: rows 4 dz + co
    f32x4 ry[NT], rd[NT];                                        // lane group q: output plane p - q, the dz <= q terms summed
#pragma unroll
    for (int t = 0; t < NT; ++t)
#pragma unroll
        for (int e = 0; e < 4; ++e) { ym[t][e] = 0.f; yc[t][e] = 0.f; dm[t][e] = 0.f; dc[t][e] = 0.f; ry[t][e] = 0.f; rd[t][e] = 0.f; }
    auto mm = [&](f32x4& acc, const half8& A, const half8& B) { acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(A, B, acc, 0, 0, 0); };

    const int rowp = wave;                                       // this wave's row of the 8 x 32 patch
    const int arow = min(c >> 2, 2) * WG + (c & 3);              // A row c = (dz c >> 2, cout c & 3); rows 12-15 are not used
    const int aP = (ks * 4 + 2 * kh) * R + arow;
    const int bB = (2 * kh) * HQ_PP + rowp * HP_RS + c;
    const int bP1 = bB + ks, bP32 = bB + 32 * ks;
    constexpr int SH4 = HP_RS + 1, SH5 = HP_RS + 2, SH7 = 2 * HP_RS + 1;
    const half8 zero = {0, 0, 0, 0, 0, 0, 0, 0};

    // the nine taps of chunk wb on the staged plane, all three dz at once: four tap pairs and the odd tap
    auto group = [&](int wb, int xb) {
        auto pair = [&](int wa, int xp) {
            const half8 wh = L8[wa + aP], wl = L8[wa + R + aP];
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const half8 xh = L8[xp + 16 * nt], xl = L8[xp + HQ_PP + 16 * nt];
                const half8 dxh = L8[xp + HQ_XT + 16 * nt], dxl = L8[xp + HQ_XT + HQ_PP + 16 * nt];
                mm(yc[nt], wh, xl); mm(ym[nt], wh, xh); mm(dm[nt], wh, dxh);
                mm(dc[nt], wh, dxl); mm(yc[nt], wl, xh); mm(dc[nt], wl, dxh);
            }
            __builtin_amdgcn_sched_barrier(0);                   // one pair's operands at a time (or the scheduler hoists every LDS read of a stage)
        };
        pair(wb, xb + bP1);                                      // taps (0,1)
        pair(wb + 2 * TAPU, xb + 2 + bP32);                      // taps (2,3)
        {                                                        // tap 4: the K halves select the PART: [wh|wl].[xl|xh], [0|wh].[xl|xh]
            const half8 a1w = L8[wb + 4 * TAPU + (2 * kh + ks) * R + arow];
            half8 a0 = L8[wb + 4 * TAPU + (2 * kh) * R + arow];
            a0 = ks ? a0 : zero;
            const int bS1 = xb + (2 * kh + 1 - ks) * HQ_PP + rowp * HP_RS + c + SH4;
#pragma unroll
            for (int nt = 0; nt < NT; ++nt) {
                const half8 b1x = L8[bS1 + 16 * nt], b1d = L8[bS1 + HQ_XT + 16 * nt];
                mm(yc[nt], a1w, b1x); mm(ym[nt], a0, b1x); mm(dc[nt], a1w, b1d); mm(dm[nt], a0, b1d);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        pair(wb + 5 * TAPU, xb + SH5 + bP32);                    // taps (5,6)
        pair(wb + 7 * TAPU, xb + SH7 + bP1);                     // taps (7,8)
    };
    // the fused skip's chunk on the 8 x 32 patch of the block input at this plane, into rows 0-3 (dz 0: this plane's own
    // output plane): y += W_s.x, dy += W_s.dx~ + dW_s~.x
    auto skipgroup = [&](int wb, int xb) {
        const bool r03 = c < R;
        half8 a1w = L8[wb + (2 * kh + ks) * R + (c & 3)], a1d = L8[wb + TAPU + (2 * kh + ks) * R + (c & 3)];
        half8 a0 = L8[wb + (2 * kh) * R + (c & 3)], a0d = L8[wb + TAPU + (2 * kh) * R + (c & 3)];
        a1w = r03 ? a1w : zero; a1d = r03 ? a1d : zero;
        a0 = (r03 && ks) ? a0 : zero; a0d = (r03 && ks) ? a0d : zero;
        const int bS1 = xb + (2 * kh + 1 - ks) * HNZ_SP + rowp * HP_COLS + c;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const half8 b1x = L8[bS1 + 16 * nt], b1d = L8[bS1 + 4 * HNZ_SP + 16 * nt];
            mm(yc[nt], a1w, b1x); mm(ym[nt], a0, b1x);
            mm(dc[nt], a1w, b1d); mm(dm[nt], a0, b1d);
            mm(dc[nt], a1d, b1x); mm(dm[nt], a0d, b1x);
        }
    };

    // ---- epilogue vectors: channels 0-7 of the one 8-channel group (4-7: padding, written as the old kernel wrote it)
    const bool act = a.flags & F_ACT, gauge = a.gout != nullptr;
    float bv[8], be[8], gv[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) { bv[j] = a.bias[j]; be[j] = a.beta[j]; gv[j] = gauge ? a.gout[j] : 0.f; }
    const int up16 = ((lane - 16) & 63) * 4;                     // ds_bpermute address: the lane one group below
    // input plane pp is complete: fold it into the running sums; lane group 2 then holds output plane z0 + pp - 2
    auto retire = [&](int pp) {
#pragma unroll
        for (int nt = 0; nt < NT; ++nt)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float ty = ym[nt][e] + yc[nt][e] * H3_INV, td = dm[nt][e] + dc[nt][e] * H3_INV;
                const float oy = ry[nt][e], od = rd[nt][e];
                const float sy = __int_as_float(__builtin_amdgcn_ds_bpermute(up16, __float_as_int(oy)));
                const float sd = __int_as_float(__builtin_amdgcn_ds_bpermute(up16, __float_as_int(od)));
                ry[nt][e] = (q ? sy : 0.f) + ty;
                rd[nt][e] = (q ? sd : 0.f) + td;
            }
        if (pp < 2 || q != 2) return;
        const int z = z0 + pp - 2;
#pragma unroll
        for (int nt = 0; nt < NT; ++nt) {
            const int yy = y0 + rowp, xx = x0 + 16 * nt + c;
            if (!(yy < a.Hv && xx < a.Wv)) continue;
            const long o = ((long)z * a.Ho + yy) * a.Wo + xx;
            half4 vh[2], vl[2], dh[2], dl[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                f32x4 v, dv;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const int j = 4 * h + e;
                    const float yp = h ? 0.f : ry[nt][e];
                    v[e] = yp + bv[j];
                    dv[e] = (h ? 0.f : rd[nt][e]) + be[j] * yp;
                    if (act) {
                        dv[e] = v[e] > 0.f ? dv[e] : 0.01f * dv[e];
                        v[e] = v[e] >= 0.f ? v[e] : 0.01f * v[e];
                    }
                    if (gauge) dv[e] += gv[j] * v[e];
                }
                split4(v, vh[h], vl[h]);
                split4(dv, dh[h], dl[h]);
            }
            const long ob = ((long)a.out_g0 * a.out_pstride + o) * 16;
            const long ol = ob + a.out_pstride * 16;
            struct alignas(16) H8 { half4 c03, c47; };         // one 16-byte store per voxel and part
            *(H8*)((char*)a.y + ob) = H8{vh[0], vh[1]};
            *(H8*)((char*)a.y + ol) = H8{vl[0], vl[1]};
            *(H8*)((char*)a.dy + ob) = H8{dh[0], dh[1]};
            *(H8*)((char*)a.dy + ol) = H8{dl[0], dl[1]};
        }
    };

    fetch(0, 0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    int s = 0;
    for (int p = 0; p < zn + 2; ++p) {
        const int nk = nchunk + (p < zn ? nskip : 0);            // the last two input planes carry no output plane's skip
        for (int k = 0; k < nk; ++k, ++s) {
            const bool last = k + 1 == nk;
            if (!last || p + 1 < zn + 2) fetch(last ? p + 1 : p, last ? 0 : k + 1, (s + 1) & 1);
            if (k == 0 && p > 0) {                               // the previous plane retires under this stage's DMA
                retire(p - 1);
#pragma unroll
                for (int t = 0; t < NT; ++t)
#pragma unroll
                    for (int e = 0; e < 4; ++e) { ym[t][e] = 0.f; yc[t][e] = 0.f; dm[t][e] = 0.f; dc[t][e] = 0.f; }
            }
            const int xb = XBASE + (s & 1) * HQ_XB;
            if (k < nchunk) group(k * WC, xb);
            else skipgroup(HNZ_SBASE + (k - nchunk) * HNZ_WS, xb);
            asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
            __syncthreads();
        }
    }
    retire(zn + 1);
}

// (launches that have no such form -- h3nz_ok, nbe_conv_select.h -- take conv_h3g_kernel<NARROW>)
static int launch_h3nz(ConvKArgs ka, int ctiles, int cout, hipStream_t s) {
    constexpr size_t smem = (size_t)HNZ_LDS_UNITS * 16;
    static_assert(smem <= 160 * 1024, "LDS budget of one CU");
    if (!h3nz_ok(ka, ctiles, cout)) return 2;
    ensure_lds_limit((const void*)conv_h3nz_kernel, smem);
    // runs of equal length, as long as HNZ_ZRUN allows: a run of Z planes stages Z + 2
    const int nrun = (ka.Dv + HNZ_ZRUN - 1) / HNZ_ZRUN;
    ka.zrun = (ka.Dv + nrun - 1) / nrun;
    ka.ntiles = (int)patch_tiles(ka, HP_ROWS, HP_COLS, (ka.Dv + ka.zrun - 1) / ka.zrun);
    for (int chunk = 0; chunk < ka.nchunk; ++chunk) {
        const ChunkSrc c = input_chunk(ka, chunk);
        ka.gs[chunk] = {c.x, c.dx, (const char*)ka.w, c.psb};
    }
    for (int sc = 0; sc < ka.nskip; ++sc) {
        const ChunkSrc c = skip_chunk(ka, sc);
        ka.gs[ka.nchunk + sc] = {c.x, c.dx, (const char*)ka.ws, c.psb};
    }
    ka.dws_delta = ka.nskip ? (const char*)ka.dws - (const char*)ka.ws : 0;
    hipLaunchKernelGGL(conv_h3nz_kernel, dim3(ka.ntiles), dim3(512), smem, s, ka);
    return 0;
}
