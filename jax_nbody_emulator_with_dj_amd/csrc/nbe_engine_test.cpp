// Test hooks: single layers (nbe_test_layer*) and single blocks of the loaded network (nbe_test_block) against the
// float64 oracle, and the modulation kernel on its own.
#include "nbe_engine_internal.h"

extern "C" {

int nbe_test_modulate(nbe_ctx* c, const float* weight, const float* sw, const float* sb, int cout, int cin, int k,
                      float s0, float s1, float eps, int first_layer, float* w_n, float* dw_tot) {
    if (!c) return fail("null context");
    HIPCHK(hipSetDevice(c->device));
    const size_t nw = (size_t)cout * cin * k * k * k;
    float *dw_ = nullptr, *dsw = nullptr, *dsb = nullptr, *dwn = nullptr, *ddw = nullptr;
    HIPCHK(hipMalloc((void**)&dw_, nw * 4)); HIPCHK(hipMalloc((void**)&dsw, cin * 8)); HIPCHK(hipMalloc((void**)&dsb, cin * 4));
    HIPCHK(hipMalloc((void**)&dwn, nw * 4)); HIPCHK(hipMalloc((void**)&ddw, nw * 4));
    HIPCHK(hipMemcpy(dw_, weight, nw * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsw, sw, cin * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(dsb, sb, cin * 4, hipMemcpyHostToDevice));
    launch_modulate(dw_, dsw, dsb, cout, cin, k * k * k, s0, s1, eps, first_layer, dwn, dw_tot ? ddw : nullptr, c->stream);
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipMemcpy(w_n, dwn, nw * 4, hipMemcpyDeviceToHost));
    if (dw_tot) HIPCHK(hipMemcpy(dw_tot, ddw, nw * 4, hipMemcpyDeviceToHost));
    (void)hipFree(dw_); (void)hipFree(dsw); (void)hipFree(dsb); (void)hipFree(dwn); (void)hipFree(ddw);
    return 0;
}

}  // extern "C"

// beta != NULL: the gauged form of a 3x3x3 layer (conv_h3g_kernel / conv_h3w_kernel / their float32 and float16 siblings):
// dx is the tangent in this layer's gauge, dy = W.dx + beta[o] * (W.x); dw is not used
static int test_layer(nbe_ctx* c, int kind, int crop, int flags, const float* x, const float* dx, int cin, int D, int H, int W,
                      const float* w, const float* dw, const float* bias, int cout, const float* res, const float* dres,
                      float* y, float* dy, const float* beta) {
    if (!c || !x || !w || !bias || !y) return fail("null argument");
    if (kind < 0 || kind > 3) return fail("kind must be 0..3");
    if (beta && !(kind == 0 && dx && dy)) return fail("the gauged form belongs to 3x3x3 layers with an input tangent");
    HIPCHK(hipSetDevice(c->device));
    const bool vel = (dw != nullptr || beta != nullptr) && dy != nullptr, has_dx = vel && dx != nullptr;
    const bool saved_vel = c->vel, saved_ga = c->gauge_active, saved_wino = c->wino_ok;
    c->vel = vel;
    c->sst.valid = false;
    const int k = kind == 0 ? 3 : kind == 1 ? 1 : 2;
    int OD, OH, OW;
    if (kind == 0) { OD = D - 2; OH = H - 2; OW = W - 2; }
    else if (kind == 1) { OD = D - 2 * crop; OH = H - 2 * crop; OW = W - 2 * crop; }
    else if (kind == 2) { OD = D / 2; OH = H / 2; OW = W / 2; }
    else { OD = 2 * D; OH = 2 * H; OW = 2 * W; }
    const size_t nin = (size_t)cin * D * H * W, nout = (size_t)cout * OD * OH * OW, nw = (size_t)cout * cin * k * k * k;
    int rc = 0;
    float *dxin = nullptr, *ddx = nullptr, *dwt = nullptr, *ddw = nullptr, *dout = nullptr;
    Layer L;
    char* ws = nullptr;
    do {
        L.cout = cout; L.cin = cin; L.k = k; L.kind = kind;
        L.first = !has_dx && cin <= 3;                           // the hook has no block names: a first layer is one that reads <= 3 channels without a tangent
        PackedW& pw = L.pw;
        pw = layer_geometry(c->prec, kind, cout, cin);
#define TCHK(e) if ((e) != hipSuccess) { rc = fail("hip error in nbe_test_layer: %s", hipGetErrorString(hipGetLastError())); break; }
        TCHK(hipMalloc((void**)&pw.w, pw.floats * pw.nsets * 4));
        if (vel) TCHK(hipMalloc((void**)&pw.dw, pw.floats * pw.nsets * 4));
        // (no narrow packing pwn, which a loaded network gives its cout <= 4 layers: the hook holds the wide tile to the oracle whatever cout is)
        if (packs_stem(c->prec, L) && alloc_stem(pw)) { rc = 1; break; }
        const int nb = pw.ctiles * 32 * pw.ni;
        TCHK(hipMalloc((void**)&pw.bias, nb * 4)); TCHK(hipMemset(pw.bias, 0, nb * 4));
        TCHK(hipMemcpy(pw.bias, bias, cout * 4, hipMemcpyHostToDevice));
        TCHK(hipMalloc((void**)&dwt, nw * 4)); TCHK(hipMemcpy(dwt, w, nw * 4, hipMemcpyHostToDevice));
        launch_pack(dwt, cout, cin, kind, pw, pw.w, c->stream);
        if (vel && !beta) { TCHK(hipMalloc((void**)&ddw, nw * 4)); TCHK(hipMemcpy(ddw, dw, nw * 4, hipMemcpyHostToDevice));
                            launch_pack(ddw, cout, cin, kind, pw, pw.dw, c->stream); }
        if (beta) {
            const size_t nbt = (size_t)pw.ctiles * 32 * pw.ni + 64;
            TCHK(hipMalloc((void**)&L.beta, nbt * 4)); TCHK(hipMemset(L.beta, 0, nbt * 4));
            TCHK(hipMemcpy(L.beta, beta, cout * 4, hipMemcpyHostToDevice));
            L.g6 = true; c->gauge_active = true;
            c->wino_ok = false;                                  // a gauged layer without a Winograd-z form must not inherit the loaded network's flag
        }
        // The hook packs the Winograd-z form only where its one launch can take it (run_conv): the gauged form, and
        // displacement only -- conv_h3w_kernel<false, NOVEL>; a loaded network packs it for every eligible layer.
        if ((beta || !vel) && packs_wino(c->prec, vel, L)) {
            if (alloc_wino(pw) || wino_flag_round_trip(c, [&] {
                    launch_pack_h3w(dwt, cout, cin, pw.cin_pad, pw.ctiles, pw.ww, c->wino_flag, c->stream, c->prec); })) { rc = 1; break; }
        }
        TCHK(hipMalloc((void**)&dxin, nin * 4)); TCHK(hipMemcpy(dxin, x, nin * 4, hipMemcpyHostToDevice));
        if (has_dx) { TCHK(hipMalloc((void**)&ddx, nin * 4)); TCHK(hipMemcpy(ddx, dx, nin * 4, hipMemcpyHostToDevice)); }
        TCHK(hipMalloc((void**)&dout, nout * 4));
        // private workspace: input, output, residual planes
        auto mk = [&](int C, int d, int h, int wd, int64_t* bytes) {
            Planes p; p.G = planes_for(C, c->prec); p.D = d; p.H = h; p.W = wd; p.pstride = (p.vox() + 63) & ~int64_t(63);
            *bytes = (int64_t)p.G * p.pstride * 16; return p; };
        int64_t bi, bo;
        Planes pin = mk(cin, D, H, W, &bi), pout = mk(cout, OD, OH, OW, &bo), pres = pout;
        const int64_t tot = 2 * bi + 4 * bo + ((int64_t)2 * H * W + 2 * W + 1024) * 16;
        // NBE_TEST_ADDR_BIT31 = 0 / 1 places the tensors where bit 31 of their addresses is clear / set.  The global -> LDS
        // DMA of the 16x16x32 kernels splits its wave-uniform base into two 32-bit halves (readfirstlane) and joins them
        // again (dma16s); a join that sign-extends the low half is wrong exactly when that bit is set -- the memory access
        // fault at 0xffffbf6e4000 of round 1 -- and right for every other address.
        char* wb = nullptr;
        if (const char* e = getenv("NBE_TEST_ADDR_BIT31")) {
            const uint64_t two = 1ull << 31, want = atoi(e) ? 1 : 0;
            if ((uint64_t)tot >= two) { rc = fail("NBE_TEST_ADDR_BIT31 needs a test tensor below 2 GiB"); break; }
            TCHK(hipMalloc((void**)&ws, tot + 2 * two));
            uint64_t b = ((uint64_t)ws + two - 1) & ~(two - 1);
            if (((b >> 31) & 1) != want) b += two;
            wb = (char*)b;
        } else {
            TCHK(hipMalloc((void**)&ws, tot));
            wb = ws;
        }
        TCHK(hipMemsetAsync(wb, 0, tot, c->stream));
        pin.x = (float*)wb; pin.dx = (float*)(wb + bi);
        pout.x = (float*)(wb + 2 * bi); pout.dx = (float*)(wb + 2 * bi + bo);
        pres.x = (float*)(wb + 2 * bi + 2 * bo); pres.dx = (float*)(wb + 2 * bi + 3 * bo);
        launch_to_planes(dxin, cin, pin, false, 1.0f, c->prec, c->stream);
        if (has_dx) launch_to_planes(ddx, cin, pin, true, 1.0f, c->prec, c->stream);
        if (flags & F_RES) {
            if (!res) { rc = fail("residual flag set but res is NULL"); break; }
            TCHK(hipMemcpyAsync(dout, res, nout * 4, hipMemcpyHostToDevice, c->stream));
            launch_to_planes(dout, cout, pres, false, 1.0f, c->prec, c->stream);
            if (vel && dres) { TCHK(hipStreamSynchronize(c->stream)); TCHK(hipMemcpyAsync(dout, dres, nout * 4, hipMemcpyHostToDevice, c->stream));
                               launch_to_planes(dout, cout, pres, true, 1.0f, c->prec, c->stream); }
            TCHK(hipStreamSynchronize(c->stream));
        }
        ConvLaunch cl; cl.in = pin; cl.out = pout; cl.res = pres; cl.flags = flags;
        if (kind == 0) { cl.Dv = OD; cl.Hv = OH; cl.Wv = OW; rc = run_conv(c, L, cl, has_dx); }
        else if (kind == 1) { cl.in_off = ((int64_t)crop * H + crop) * W + crop; cl.Dv = OD; cl.Hv = OH; cl.Wv = OW; rc = run_conv(c, L, cl, has_dx); }
        else if (kind == 2) { cl.Dv = OD; cl.Hv = OH; cl.Wv = OW; rc = run_conv(c, L, cl, has_dx); }
        else {
            const bool up8 = up8_launch(c, L, has_dx);          // as upblock()
            for (int p = 0; p < (up8 ? 1 : 8) && !rc; ++p) {
                ConvLaunch u = cl; u.Dv = D; u.Hv = H; u.Wv = W; u.osz = 2; u.oz = (p >> 2) & 1; u.oy = (p >> 1) & 1; u.ox = p & 1;
                u.set = up8 ? -1 : p;
                rc = run_conv(c, L, u, has_dx);
            }
        }
        if (rc) break;
        launch_from_planes(pout, false, cout, dout, c->prec, c->stream);
        TCHK(hipStreamSynchronize(c->stream));
        TCHK(hipMemcpy(y, dout, nout * 4, hipMemcpyDeviceToHost));
        if (vel) {
            launch_from_planes(pout, true, cout, dout, c->prec, c->stream);
            TCHK(hipStreamSynchronize(c->stream));
            TCHK(hipMemcpy(dy, dout, nout * 4, hipMemcpyDeviceToHost));
        }
        TCHK(hipGetLastError());
#undef TCHK
    } while (0);
    c->vel = saved_vel; c->gauge_active = saved_ga; c->wino_ok = saved_wino;
    (void)hipFree(dxin); (void)hipFree(ddx); (void)hipFree(dwt); (void)hipFree(ddw); (void)hipFree(dout); (void)hipFree(ws);
    release_layer(L);
    return rc;
}

// ---- nbe_test_block: one block of the loaded network through resblock / resblock_part / upblock / downblock -----------
namespace {
struct BlockIO {                                                 // host <-> engine tensors of nbe_test_block
    nbe_ctx* c; std::vector<void*> dev; float scale = 1.f;
    ~BlockIO() { for (void* p : dev) (void)hipFree(p); }
    float* stage(size_t n) { void* p = nullptr; if (hipMalloc(&p, n * 4) != hipSuccess) { (void)hipGetLastError(); return nullptr; } dev.push_back(p); return (float*)p; }
    // dense (C, D, Hi, Wi) host arrays a (channels [0, Ca)) and b (channels [Ca, C), nullable) -> the interior of t, times scale
    int put(const Tensor& t, int C, int Ca, int Hi, int Wi, const float* a, const float* b, bool tangent) {
        const int D = t.p.D, H = t.p.H, W = t.p.W, pad = t.pad;
        std::vector<float> hbuf((size_t)C * D * H * W, 0.f);
        for (int ch = 0; ch < C; ++ch) {
            const float* src = ch < Ca ? a + (size_t)ch * D * Hi * Wi : (b ? b + (size_t)(ch - Ca) * D * Hi * Wi : nullptr);
            if (!src) continue;
            for (int z = 0; z < D; ++z) for (int yy = 0; yy < Hi; ++yy)
                memcpy(&hbuf[(((size_t)ch * D + z) * H + yy + pad) * W + pad], src + ((size_t)z * Hi + yy) * Wi, (size_t)Wi * 4);
        }
        float* d = stage(hbuf.size());
        if (!d) return fail("nbe_test_block: out of device memory");
        HIPCHK(hipMemcpy(d, hbuf.data(), hbuf.size() * 4, hipMemcpyHostToDevice));
        launch_to_planes(d, C, t.p, tangent, scale, c->prec, c->stream);
        return 0;
    }
    // the (C, D, Hi, Wi) voxels of t from (pad, pad) on -> dense host array, divided by scale
    int get(const Tensor& t, int C, int Hi, int Wi, float* out, bool tangent) {
        const int D = t.p.D, H = t.p.H, W = t.p.W, pad = t.pad;
        const size_t n = (size_t)C * D * H * W;
        float* d = stage(n);
        if (!d) return fail("nbe_test_block: out of device memory");
        launch_from_planes(t.p, tangent, C, d, c->prec, c->stream);
        HIPCHK(hipStreamSynchronize(c->stream));
        std::vector<float> hbuf(n);
        HIPCHK(hipMemcpy(hbuf.data(), d, n * 4, hipMemcpyDeviceToHost));
        const float inv = 1.0f / scale;
        for (int ch = 0; ch < C; ++ch) for (int z = 0; z < D; ++z) for (int yy = 0; yy < Hi; ++yy) {
            const float* s = &hbuf[(((size_t)ch * D + z) * H + yy + pad) * W + pad];
            float* o = out + (((size_t)ch * D + z) * Hi + yy) * Wi;
            for (int xx = 0; xx < Wi; ++xx) o[xx] = s[xx] * inv;
        }
        return 0;
    }
};
}  // namespace

static int test_block(nbe_ctx* c, const char* block, int pad, int two_source, const float* x, const float* dx, int D, int H, int W,
                      const float* x2, const float* dx2, float* y, float* dy, float* h, float* dh, float* gauges, int* paths) {
    if (!c || !block || !x || !y || !gauges || !paths) return fail("null argument");
    if (require_ready(c)) return 1;
    if (pad != 0 && pad != 1) return fail("nbe_test_block: pad must be 0 or 1");
    HIPCHK(hipSetDevice(c->device));
    const int m = c->mid;
    const std::string name = block;
    const bool up = !name.compare(0, 3, "up_"), down = !name.compare(0, 5, "down_"), res = !up && !down;
    const bool dec = name == "conv_r2" || name == "conv_r1" || name == "conv_r00";
    const Layer *L0 = find_layer(c, block, "conv_0"), *L1 = find_layer(c, block, "conv_1");
    if (!L0 || (res && (!L1 || !find_layer(c, block, "skip")))) return fail("nbe_test_block: unknown block %s", block);
    const bool has_dx = name != "conv_l00", vel = c->vel;
    if (vel && ((has_dx && !dx) || !dy || (x2 && !dx2) || (h && !dh))) return fail("nbe_test_block: a velocity context needs the tangents");
    if (x2 && !dec && !up) return fail("nbe_test_block: block %s takes one input", block);
    if (two_source && !(dec && x2)) return fail("nbe_test_block: the two-source form belongs to the decoder blocks, with x2");
    const int lim = res ? 5 : 1;
    if (D < lim || H < (pad && res ? 3 : lim) || W < (pad && res ? 3 : lim)) return fail("nbe_test_block: input (%d, %d, %d) too small for %s", D, H, W, block);
    if (down && ((D | H | W) & 1)) return fail("nbe_test_block: down-sampling needs even extents");
    const int cin = L0->cin, cmid = L0->cout, cout = res ? L1->cout : L0->cout;
    const bool final_act = name != "conv_r01";
    const int sy = pad ? 0 : 2;
    if (two_source && !(block_fused(c, L1, D - 4) && two_source_width(c))) return fail("nbe_test_block: block %s does not run the two-source form here", block);

    const float keep_preset = c->preset_absmax;
    int* const keep_paths = c->paths;
    c->sst.valid = false;                                        // the arena is reused: a pending brick's tensors are gone
    // the call's range shift, as a box applies it: max |x| over what goes in (Dz / 6 = 1)
    size_t n1 = (size_t)(x2 && dec ? m : cin) * D * H * W, n2 = x2 ? (size_t)m * D * H * W * (up ? 8 : 1) : 0;
    unsigned bits = host_absmax_bits(x, (int64_t)n1);
    if (x2) bits = std::max(bits, host_absmax_bits(x2, (int64_t)n2));
    memcpy(&c->preset_absmax, &bits, 4);
    int rc = prepare_range(c, nullptr, 0, 6.0f);
    c->preset_absmax = keep_preset;
    if (rc) return rc;

    BlockIO io; io.c = c; io.scale = c->act_scale;
    int word = 0;
    Tensor ty, th;                                               // result and hidden tensor of the real pass
    int yC = cout, yH = 0, yW = 0;
    auto body = [&]() -> int {
        c->arena.reset();
        if (res) {
            const bool cat = dec && x2 && !two_source;           // concat on the way in
            Tensor tx = tallocp(c, two_source ? m : cin, D, H, W, pad), tx2;
            if (two_source) tx2 = tallocp(c, m, D, H, W, pad);
            if (tx.off < 0 || (two_source && tx2.off < 0)) return fail("workspace exhausted in nbe_test_block");
            if (!c->dry) {
                if (io.put(tx, two_source ? m : cin, cat ? m : cin, H, W, x, cat ? x2 : nullptr, false)) return 1;
                if (vel && has_dx && io.put(tx, two_source ? m : cin, cat ? m : cin, H, W, dx, cat ? dx2 : nullptr, true)) return 1;
                if (two_source && (io.put(tx2, m, m, H, W, x2, nullptr, false) || (vel && io.put(tx2, m, m, H, W, dx2, nullptr, true)))) return 1;
            }
            fill_halo(c, tx);
            if (two_source) fill_halo(c, tx2);
            if (!two_source) {
                if (resblock(c, block, tx, has_dx, final_act, cout, cmid, &ty, &th)) return 1;
            } else {
                // the first-slab call of stream_tail: persistent hidden and result tensors, the up-sampled half as x2
                th = alloc_hidden(c, cmid, D - 2, tx, block_fused(c, L1, D - 4));
                ty = tallocp(c, cout, D - 4, H - 2 * sy, W - 2 * sy, pad);
                if (th.off < 0 || ty.off < 0) return fail("workspace exhausted in nbe_test_block");
                if (resblock_part(c, block, tx, th, ty, 0, D - 4, 0, D - 2, true, final_act, nullptr, &tx2)) return 1;
            }
            yH = H - 2 * sy; yW = W - 2 * sy;
        } else if (down) {
            Tensor tx = tallocp(c, m, D, H, W, pad);
            if (tx.off < 0) return fail("workspace exhausted in nbe_test_block");
            if (!c->dry && (io.put(tx, m, m, H, W, x, nullptr, false) || (vel && io.put(tx, m, m, H, W, dx, nullptr, true)))) return 1;
            fill_halo(c, tx);
            if (!pad) { if (downblock(c, block, tx, &ty)) return 1; }
            else {                                               // periodic-yx: the interior only (stream_level1)
                ty = talloc(c, m, D / 2, H / 2, W / 2);
                if (ty.off < 0) return fail("workspace exhausted in nbe_test_block");
                if (down_conv(c, *L0, tx, ty, false)) return 1;
            }
            yH = H / 2; yW = W / 2;
        } else {
            Tensor tx = tallocp(c, m, D, H, W, pad);
            ty = tallocp(c, x2 ? 2 * m : m, 2 * D, 2 * H, 2 * W, pad);
            if (tx.off < 0 || ty.off < 0) return fail("workspace exhausted in nbe_test_block");
            if (!c->dry) {
                if (io.put(tx, m, m, H, W, x, nullptr, false) || (vel && io.put(tx, m, m, H, W, dx, nullptr, true))) return 1;
                if (x2 && (io.put(ty, 2 * m, m, 2 * H, 2 * W, x2, nullptr, false) || (vel && io.put(ty, 2 * m, m, 2 * H, 2 * W, dx2, nullptr, true)))) return 1;
            }
            fill_halo(c, tx);
            if (upblock(c, block, tx, ty, 0, x2 ? -1 : 0)) return 1;
            fill_halo(c, ty);
            yC = x2 ? 2 * m : m; yH = 2 * H; yW = 2 * W;
        }
        return 0;
    };
    c->dry = true;
    rc = body();
    c->dry = false;
    if (rc) return rc;
    const int64_t need = c->arena.high;
    if (need > c->ws_bytes) {
        if (c->ws) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
        HIPCHK(hipMalloc((void**)&c->ws, need));
        HIPCHK(hipMemsetAsync(c->ws, 0, need, c->stream));
        c->ws_bytes = need;
    }
    c->paths = &word;
    rc = body();
    c->paths = keep_paths;
    if (!rc) rc = io.get(ty, yC, yH, yW, y, false);
    if (!rc && vel) rc = io.get(ty, yC, yH, yW, dy, true);
    if (!rc && res && h) {
        // a fused block's hidden tensor borrows the input's pitch: its valid voxels start at (0, 0) (pad = 0) / (1, 1)
        rc = io.get(th, cmid, H - sy, W - sy, h, false);
        if (!rc && vel) rc = io.get(th, cmid, H - sy, W - sy, dh, true);
    }
    c->range_pending = false;                                    // no head ran: nothing to check
    if (rc) return rc;
    HIPCHK(hipStreamSynchronize(c->stream));
    HIPCHK(hipGetLastError());
    // the gauges as the device holds them
    memset(gauges, 0, (size_t)6 * m * 4);
    if (c->gauge_active && vel) {
        const float* gin = res ? (has_dx ? L0->alpha : nullptr) : L0->a_in;
        const float* ghid = res ? L1->alpha : nullptr;
        const float* gout = res ? L1->gout : L0->gout;
        if (gin) HIPCHK(hipMemcpy(gauges, gin, (size_t)cin * 4, hipMemcpyDeviceToHost));
        if (ghid) HIPCHK(hipMemcpy(gauges + 2 * m, ghid, (size_t)cmid * 4, hipMemcpyDeviceToHost));
        if (gout) HIPCHK(hipMemcpy(gauges + 4 * m, gout, (size_t)cout * 4, hipMemcpyDeviceToHost));
    }
    *paths = word;
    return 0;
}

extern "C" {

int nbe_test_block(nbe_ctx* c, const char* block, int pad, int two_source, const float* x, const float* dx, int D, int H, int W,
                   const float* x2, const float* dx2, float* y, float* dy, float* h, float* dh, float* gauges, int* paths) {
    return test_block(c, block, pad, two_source, x, dx, D, H, W, x2, dx2, y, dy, h, dh, gauges, paths);
}

int nbe_test_layer(nbe_ctx* c, int kind, int crop, int flags, const float* x, const float* dx, int cin, int D, int H, int W,
                   const float* w, const float* dw, const float* bias, int cout, const float* res, const float* dres,
                   float* y, float* dy) {
    return test_layer(c, kind, crop, flags, x, dx, cin, D, H, W, w, dw, bias, cout, res, dres, y, dy, nullptr);
}

int nbe_test_layer_gauged(nbe_ctx* c, int flags, const float* x, const float* dx, int cin, int D, int H, int W,
                          const float* w, const float* beta, const float* bias, int cout, float* y, float* dy) {
    if (!beta) return fail("null argument");
    return test_layer(c, 0, 0, flags, x, dx, cin, D, H, W, w, nullptr, bias, cout, nullptr, nullptr, y, dy, beta);
}

int nbe_test_layer_gauged_res(nbe_ctx* c, int flags, const float* x, const float* dx, int cin, int D, int H, int W,
                              const float* w, const float* beta, const float* bias, int cout, const float* res, const float* dres,
                              float* y, float* dy) {
    if (!beta) return fail("null argument");
    return test_layer(c, 0, 0, flags, x, dx, cin, D, H, W, w, nullptr, bias, cout, res, dres, y, dy, beta);
}

}  // extern "C"
