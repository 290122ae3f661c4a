// Weights: what a layer needs on the device (packing geometry, which packings a layer gets, the Winograd-z range flag,
// release), loading a parameter tree, gauge wiring of the tangents, and the Winograd-z weights of a modulation.
#include "nbe_engine_internal.h"

// ------------------------------------------------------------------------------------------------
// What a layer needs on the device.  load_weights, pack_wino and the layer test hook (nbe_engine_test.cpp) go through
// these, so the hook's layer is packed by the rules a loaded network's layers are.
// ------------------------------------------------------------------------------------------------

// geometry of the packing of a (cout, cin) layer of `kind` (0 conv3, 1 skip, 2 down, 3 up); no buffers
PackedW layer_geometry(int prec, int kind, int cout, int cin) {
    PackedW pw;
    pw.mode = kind == 0 ? MODE_FLAT3 : (kind == 2 ? MODE_DOWN : MODE_FLAT1);
    pw.prec = prec;
    pw.ni = (prec_is_half(prec) || cout > 32) ? 2 : 1;
    pw.cin = cin; pw.cout = cout;
    pw.cin_pad = roundup(cin, prec_ck(prec, pw.mode));
    pw.ctiles = (cout + 32 * pw.ni - 1) / (32 * pw.ni);
    pw.nsets = kind == 3 ? 8 : 1;
    pw.floats = (int64_t)pw.ctiles * 32 * pw.ni * mode_nseg(pw.mode) * mode_taps(pw.mode) * pw.cin_pad / (prec == PREC_F16 ? 2 : 1);
    return pw;
}

// Which packings a layer gets beside pw.w / pw.dw.  They read L.kind, L.first, L.cout, L.cin and L.pw's geometry;
// packs_wino and packs_wino_skip also whether the narrow packing exists (L.pwn.w), which therefore comes first.

// the narrow packing (16-cout tiles, conv_h3g_kernel<true>)
// (cout <= 4: the head convolution 64 -> 3.  Narrow test models, cout 8 or 16, stay on the wide tile so that they
// exercise what production-width layers run, skip fusion included.)
bool packs_narrow(int prec, bool vel, const Layer& L) {
    return prec == PREC_F16X3 && vel && (L.kind == 0 || L.kind == 1) && L.cout <= 4 && !L.first;
}
// the Winograd-z packing of a 3x3x3 layer (conv_h3w_kernel): 4 transformed kernels per 3 dz slices, wide tile only, Cin <= 128
bool packs_wino(int prec, bool vel, const Layer& L) {
    return L.kind == 0 && !L.first && ((prec == PREC_F16X3 && !L.pwn.w && h3w_stages_fit(L.pw.cin_pad)) || wino_f16_layer(prec, vel, L.pw.cin_pad));
}
// [W_s | dW_s~] of a skip that may run fused into its block's conv_1 (the float16 model: style path only, with dwn_f beside it)
bool packs_wino_skip(int prec, bool vel, bool style, const Layer& L) {
    return L.kind == 1 && ((prec == PREC_F16X3 && !L.pwn.w && h3w_stages_fit(L.pw.cin_pad)) ||
                           (style && !L.first && wino_f16_layer(prec, vel, L.pw.cin_pad)));
}
// the first layer in its own packing (stem_h3_kernel): K = 27 taps x 3 channels = 81 <= 96
bool packs_stem(int prec, const Layer& L) {
    return prec_is_half(prec) && L.kind == 0 && L.first && L.cin <= 3 && L.cout <= 64;
}
int alloc_wino(PackedW& pw) { HIPCHK(hipMalloc((void**)&pw.ww, pw.floats * 4 / 3 * 4)); return 0; }
int alloc_stem(PackedW& pw) { HIPCHK(hipMalloc((void**)&pw.stem, 4 * 3 * 4 * 64 * 16)); return 0; }

// The range flag of the Winograd-z packs: `packs` enqueues launch_pack_h3w / launch_pack_h3w_skip with c->wino_flag; wino_ok
// is cleared when a weight they transformed leaves the f16 range at the kernel's 2^14 scale.  (synchronises the stream)
int wino_flag_round_trip(nbe_ctx* c, const std::function<void()>& packs) {
    if (!c->wino_flag) HIPCHK(hipMalloc((void**)&c->wino_flag, 4));
    HIPCHK(hipMemsetAsync(c->wino_flag, 0, 4, c->stream));
    packs();
    int bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, c->wino_flag, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    c->wino_ok = bad == 0;
    return 0;
}

// every device buffer a Layer owns
void release_layer(Layer& L) {
    (void)hipFree(L.weight); (void)hipFree(L.sw); (void)hipFree(L.sb); (void)hipFree(L.wn); (void)hipFree(L.dwn);
    (void)hipFree(L.pw.w); (void)hipFree(L.pw.dw); (void)hipFree(L.pw.bias); (void)hipFree(L.bias0); (void)hipFree(L.pw.stem); (void)hipFree(L.pw.ww); (void)hipFree(L.pwn.w); (void)hipFree(L.pwn.dw); (void)hipFree(L.bias_f);
    (void)hipFree(L.alpha); (void)hipFree(L.beta); (void)hipFree(L.dwn_f);
}

// ------------------------------------------------------------------------------------------------
// loading
// ------------------------------------------------------------------------------------------------
void free_layers(nbe_ctx* c) {
    drop_graphs(c); ++c->epoch;
    c->bp_slab = 0;                                             // the workspace layout follows the layers (width, fused skips): plan the brick again
    for (auto& kv : c->layers) release_layer(kv.second);
    c->layers.clear();
    c->bias_scale = 1.f; c->bias_max = 0.f; c->bias_dirty = true;
    c->have_weights = false; c->modulated = false; c->gauge = false; c->gauge_active = false; c->fuse = false; c->novel_fuse = false; c->wino_ok = false;
}

static int kind_of(const nbe_layer_desc& d, int* kind) {
    const std::string blk = d.block, lay = d.layer;
    if (lay == "skip") { if (d.k != 1) return fail("%s/%s: skip layers have k=1", d.block, d.layer); *kind = 1; return 0; }
    if (blk.rfind("down_", 0) == 0) { if (d.k != 2) return fail("%s: down layers have k=2", d.block); *kind = 2; return 0; }
    if (blk.rfind("up_", 0) == 0) { if (d.k != 2) return fail("%s: up layers have k=2", d.block); *kind = 3; return 0; }
    if (d.k != 3) return fail("%s/%s: conv layers have k=3", d.block, d.layer);
    *kind = 0;
    return 0;
}

static int expected_shape(nbe_ctx* c, const std::string& blk, const std::string& lay, int* cout, int* cin) {
    const int m = c->mid;
    int bi, bo;
    if (blk == "conv_l00") { bi = c->in_chan; bo = m; }
    else if (blk == "conv_r2" || blk == "conv_r1" || blk == "conv_r00") { bi = 2 * m; bo = m; }
    else if (blk == "conv_r01") { bi = m; bo = c->out_chan; }
    else { bi = m; bo = m; }
    const int midc = bi > bo ? bi : bo;                     // style_blocks_vel.py:126
    if (lay == "skip") { *cin = bi; *cout = bo; }
    else if (blk.rfind("down_", 0) == 0 || blk.rfind("up_", 0) == 0) { *cin = bi; *cout = bo; }
    else if (lay == "conv_0") { *cin = bi; *cout = midc; }
    else if (lay == "conv_1") { *cin = midc; *cout = bo; }
    else return fail("unknown layer %s/%s", blk.c_str(), lay.c_str());
    return 0;
}

static const char* kBlocks[15] = {"conv_l00", "conv_l01", "down_l0", "conv_l1", "down_l1", "conv_l2", "down_l2", "conv_c",
                                  "up_r2", "conv_r2", "up_r1", "conv_r1", "up_r0", "conv_r00", "conv_r01"};

// Winograd-z weights of the gauged wide 3x3x3 layers (conv_h3w_kernel), from the modulated weights L.wn that are current
int pack_wino(nbe_ctx* c) {
    c->wino_ok = false;
    if (!((c->prec == PREC_F16X3 && (c->vel ? c->gauge_active : true)) || (c->prec == PREC_F16 && c->vel && c->gauge_active))) return 0;
    if (wino_flag_round_trip(c, [c] {
            for (auto& kv : c->layers) {
                Layer& L = kv.second;
                if (L.pw.ww && L.kind == 0 && (L.g6 || !c->vel)) launch_pack_h3w(L.wn, L.cout, L.cin, L.pw.cin_pad, L.pw.ctiles, L.pw.ww, c->wino_flag, c->stream, c->prec);
                if (L.pw.ww && L.kind == 1 && (c->vel ? (L.b_sub && c->fuse) : c->novel_fuse)) {   // a fused skip: [W_s | dW_s~] for conv_h3w_kernel<SKIP>
                    launch_pack_h3w_skip(L.wn, L.cout, L.cin, L.pw, L.pw.ww, c->wino_flag, c->stream);
                    if (c->vel) launch_pack_h3w_skip(c->prec == PREC_F16 ? L.dwn_f : L.dwn, L.cout, L.cin, L.pw, L.pw.ww + L.pw.floats, c->wino_flag, c->stream);
                }
            }
        })) return 1;
    if (!c->vel) c->fuse = c->novel_fuse && c->wino_ok;         // displacement only: the fused skips live in the Winograd-z kernel
    if (c->prec == PREC_F16) c->fuse = c->fuse && c->wino_ok;   // the float16 model: likewise
    return 0;
}

// Displacement-only f16x3 networks: every block whose conv_1 has a Winograd-z form runs its 1x1x1 skip inside that launch
// (conv_h3w_kernel<SKIP, NOVEL>), as the velocity networks do through wire_gauge
static int wire_novel(nbe_ctx* c) {
    c->novel_fuse = false;
    if (c->vel || c->prec != PREC_F16X3) return 0;
    for (const char* b : kBlocks) {
        if (!strncmp(b, "down_", 5) || !strncmp(b, "up_", 3)) continue;
        auto i1 = c->layers.find(std::string(b) + "/conv_1"), is = c->layers.find(std::string(b) + "/skip");
        if (i1 == c->layers.end() || is == c->layers.end()) return fail("internal: block %s", b);
        Layer &L1 = i1->second, &Ls = is->second;
        if (!L1.pw.ww || !Ls.pw.ww || !h3w_skip_fits(Ls.pw.cin_pad) || L1.pw.ctiles != Ls.pw.ctiles) return 0;   // all blocks or none
    }
    for (const char* b : kBlocks) {
        if (!strncmp(b, "down_", 5) || !strncmp(b, "up_", 3)) continue;
        Layer &L1 = c->layers[std::string(b) + "/conv_1"], &Ls = c->layers[std::string(b) + "/skip"];
        L1.fskip = &Ls;
        const int nb = L1.pw.ctiles * 32 * L1.pw.ni;
        HIPCHK(hipMalloc((void**)&L1.bias_f, nb * 4));
    }
    c->novel_fuse = true;
    return 0;
}

// Tangent gauges of the style path (conv_h3g_kernel): every tensor with a tangent stores dx + a (.) x, a = the alpha
// of the one 3x3x3 layer that reads it, so that layer runs two products instead of three; the tensor's other readers
// (skips, down-sampling) fold a into their tangent weights.  Tensors read only by general kernels keep a = 0.
static int wire_gauge(nbe_ctx* c) {
    const int m = c->mid;
    for (auto& kv : c->layers) {
        Layer& L = kv.second;
        const size_t na = (size_t)roundup(L.cin, 16) + 64, nb = (size_t)L.pw.ctiles * 32 * L.pw.ni + 64;
        HIPCHK(hipMalloc((void**)&L.alpha, na * 4)); HIPCHK(hipMemset(L.alpha, 0, na * 4));
        HIPCHK(hipMalloc((void**)&L.beta, nb * 4)); HIPCHK(hipMemset(L.beta, 0, nb * 4));
    }
    if (!c->gauge_flag) HIPCHK(hipMalloc((void**)&c->gauge_flag, 4));
    auto lay = [&](const char* b, const char* l) -> Layer* {
        auto it = c->layers.find(std::string(b) + "/" + l);
        return it == c->layers.end() ? nullptr : &it->second;
    };
    // output of `producer` is read by the 3x3x3 layer `consumer`/conv_0 as its input channels [off, off + cout)
    struct Rule { const char* pb; const char* pl; const char* consumer; int off; };
    const Rule rules[] = {
        {"conv_l00", "conv_1", "conv_l01", 0}, {"conv_l01", "conv_1", "conv_r00", 0}, {"down_l0", "conv_0", "conv_l1", 0},
        {"conv_l1", "conv_1", "conv_r1", 0},   {"down_l1", "conv_0", "conv_l2", 0},   {"conv_l2", "conv_1", "conv_r2", 0},
        {"down_l2", "conv_0", "conv_c", 0},    {"up_r2", "conv_0", "conv_r2", m},     {"up_r1", "conv_0", "conv_r1", m},
        {"up_r0", "conv_0", "conv_r00", m},    {"conv_r00", "conv_1", "conv_r01", 0},
    };
    for (const Rule& r : rules) {
        Layer *P = lay(r.pb, r.pl), *C = lay(r.consumer, "conv_0");
        if (!P || !C || r.off + P->cout > C->cin) return fail("internal: gauge wiring %s/%s -> %s", r.pb, r.pl, r.consumer);
        P->gout = C->alpha + r.off;
    }
    for (const char* b : kBlocks) {
        if (!strncmp(b, "down_", 5) || !strncmp(b, "up_", 3)) continue;
        Layer *L0 = lay(b, "conv_0"), *L1 = lay(b, "conv_1"), *Ls = lay(b, "skip");
        L0->gout = L1->alpha;                                    // the hidden tensor is read by conv_1 only
        L1->g6 = true;
        if (strcmp(b, "conv_l00")) { L0->g6 = true; Ls->a_in = L0->alpha; }   // conv_l00 reads the input field: no tangent
        // the skip can run inside conv_1 (conv_h3g_kernel<false>): f16x3, the block input has a tangent, the wide tile,
        // and the groups of both fit the kernel's table
        if (c->prec == PREC_F16X3 && (!L1->pwn.w || Ls->pwn.dw) &&
            3 * (L1->pw.cin_pad / 16) + Ls->pw.cin_pad / 16 <= NBE_MAX_GROUPS) {
            L1->fskip = Ls; Ls->b_sub = L1->beta;
            const int nb = L1->pw.ctiles * 32 * L1->pw.ni;
            HIPCHK(hipMalloc((void**)&L1->bias_f, nb * 4));
        }
        // float16 model (style path): the skip runs inside conv_h3w_kernel<SKIP, ., F16> wherever conv_1's launch has that form
        if (c->prec == PREC_F16 && L1->pw.ww && Ls->pw.ww && Ls->dwn_f && L1->pw.ctiles == Ls->pw.ctiles &&
            h3w_skip_fits(Ls->pw.cin_pad, H3W_F16_CHUNKS)) {
            L1->fskip = Ls; Ls->b_sub = L1->beta;
            const int nb = L1->pw.ctiles * 32 * L1->pw.ni;
            HIPCHK(hipMalloc((void**)&L1->bias_f, nb * 4));
        }
    }
    // every gauged 3x3x3 layer must fit the group table of conv_h3g_kernel
    for (auto& kv : c->layers)
        if (kv.second.g6 && 3 * (kv.second.pw.cin_pad / 16) > NBE_MAX_GROUPS) { c->gauge = false; return 0; }
    lay("down_l0", "conv_0")->a_in = lay("conv_r00", "conv_0")->alpha;    // they read conv_l01 / conv_l1 / conv_l2's output
    lay("down_l1", "conv_0")->a_in = lay("conv_r1", "conv_0")->alpha;
    lay("down_l2", "conv_0")->a_in = lay("conv_r2", "conv_0")->alpha;
    c->gauge = true;
    return 0;
}

// Premodulated (W, dW) pairs: modulate_emulator_parameters_vel (nbody_emulator.py:221-266) produces dW = W (.) (alpha[ci] +
// beta[co]) -- recognise that from the numbers (weighted alternating least squares for the additive model, then an
// element-wise check) and run the gauged kernels; any 3x3x3 layer whose pair does not factorise to float32 rounding
// (hand-made or perturbed dweight) leaves the whole network on the general three-product kernels.
static int wire_gauge_premod(nbe_ctx* c, const nbe_layer_desc* descs, int n) {
    std::map<std::string, std::vector<double>> al, be;
    std::map<std::string, const nbe_layer_desc*> by_name;
    for (int i = 0; i < n; ++i) by_name[std::string(descs[i].block) + "/" + descs[i].layer] = &descs[i];
    for (const char* b : kBlocks) {
        if (!strncmp(b, "down_", 5) || !strncmp(b, "up_", 3)) continue;
        for (const char* l : {"conv_0", "conv_1"}) {
            if (!strcmp(b, "conv_l00") && !strcmp(l, "conv_0")) continue;    // reads the input field: never gauged
            const std::string key = std::string(b) + "/" + l;
            const nbe_layer_desc& d = *by_name[key];
            const int co = d.cout, ci = d.cin, k3 = d.k * d.k * d.k;
            std::vector<double> a(ci, 0.0), bt(co, 0.0);
            double dmax = 0.0;
            for (size_t e = 0; e < (size_t)co * ci * k3; ++e) dmax = std::max(dmax, (double)std::fabs(d.dweight[e]));
            for (int iter = 0; iter < 200; ++iter) {
                double change = 0.0;
                for (int i = 0; i < ci; ++i) {                           // alpha[i] = sum w (dW - W beta) / sum w^2 over (o, k)
                    double num = 0.0, den = 0.0;
                    for (int o = 0; o < co; ++o)
                        for (int k = 0; k < k3; ++k) {
                            const double w = d.weight[((size_t)o * ci + i) * k3 + k], dw = d.dweight[((size_t)o * ci + i) * k3 + k];
                            num += w * (dw - w * bt[o]); den += w * w;
                        }
                    const double v = den > 0 ? num / den : 0.0;
                    change = std::max(change, std::fabs(v - a[i])); a[i] = v;
                }
                for (int o = 0; o < co; ++o) {
                    double num = 0.0, den = 0.0;
                    for (int i = 0; i < ci; ++i)
                        for (int k = 0; k < k3; ++k) {
                            const double w = d.weight[((size_t)o * ci + i) * k3 + k], dw = d.dweight[((size_t)o * ci + i) * k3 + k];
                            num += w * (dw - w * a[i]); den += w * w;
                        }
                    const double v = den > 0 ? num / den : 0.0;
                    change = std::max(change, std::fabs(v - bt[o])); bt[o] = v;
                }
                if (change < 1e-13) break;
            }
            double res = 0.0;
            for (int o = 0; o < co; ++o)
                for (int i = 0; i < ci; ++i)
                    for (int k = 0; k < k3; ++k) {
                        const size_t e = ((size_t)o * ci + i) * k3 + k;
                        res = std::max(res, std::fabs((double)d.dweight[e] - (double)d.weight[e] * (a[i] + bt[o])));
                    }
            if (!(res <= 2e-6 * dmax + 1e-30)) return 0;                 // does not factorise: keep the general kernels
            // alpha + c, beta - c is the same pair: centre alpha, and keep it small (the f16 formats store dx + alpha * x)
            const double amin = *std::min_element(a.begin(), a.end()), amax = *std::max_element(a.begin(), a.end());
            const double mid = 0.5 * (amin + amax);
            for (double& v : a) v -= mid;
            for (double& v : bt) v += mid;
            if (amax - mid > 64.0) return 0;
            al[key] = a; be[key] = bt;
        }
    }
    if (wire_gauge(c)) return 1;
    if (!c->gauge) return 0;                                    // a layer too wide for the gauged kernel's group table
    for (auto& kv : c->layers) {
        Layer& L = kv.second;
        auto ia = al.find(kv.first);
        if (ia != al.end()) {
            std::vector<float> fa(ia->second.begin(), ia->second.end()), fb(be[kv.first].begin(), be[kv.first].end());
            HIPCHK(hipMemcpy(L.alpha, fa.data(), fa.size() * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.beta, fb.data(), fb.size() * 4, hipMemcpyHostToDevice));
        }
    }
    // general layers that read a gauged tensor: dW - W (.) a_in, a_in = alpha of the tensor's 3x3x3 reader (wire_gauge)
    auto fold = [&](const char* b, const char* l, const char* reader, int off) -> int {
        const std::string key = std::string(b) + "/" + l;
        const nbe_layer_desc& d = *by_name[key];
        Layer& L = c->layers[key];
        static const std::vector<double> none(4096, 0.0);          // reader == nullptr: the input carries no gauge (conv_l00)
        const std::vector<double>& a = reader ? al[std::string(reader) + "/conv_0"] : none;
        // a skip that runs inside its block's conv_1 (Layer::b_sub): the kernel's epilogue adds beta_1[o] * (W_s.x) as well
        const std::vector<double>* bsub = L.b_sub ? &be[std::string(b) + "/conv_1"] : nullptr;
        const int k3 = d.k * d.k * d.k;
        std::vector<float> eff((size_t)d.cout * d.cin * k3);
        for (int o = 0; o < d.cout; ++o)
            for (int i = 0; i < d.cin; ++i)
                for (int k = 0; k < k3; ++k) {
                    const size_t e = ((size_t)o * d.cin + i) * k3 + k;
                    eff[e] = (float)((double)d.dweight[e] - (double)d.weight[e] * a[off + i]
                                     - (bsub ? (double)d.weight[e] * (*bsub)[o] : 0.0));
                }
        HIPCHK(hipMemcpy(L.dwn, eff.data(), eff.size() * 4, hipMemcpyHostToDevice));
        launch_pack(L.dwn, d.cout, d.cin, L.kind, L.pw, L.pw.dw, c->stream);
        if (L.pwn.dw) launch_pack(L.dwn, d.cout, d.cin, L.kind, L.pwn, L.pwn.dw, c->stream);
        return 0;
    };
    for (const char* b : kBlocks) {
        if (!strncmp(b, "down_", 5) || !strncmp(b, "up_", 3)) continue;
        if (!strcmp(b, "conv_l00")) { if (c->layers[std::string(b) + "/skip"].b_sub && fold(b, "skip", nullptr, 0)) return 1; continue; }
        if (fold(b, "skip", b, 0)) return 1;
    }
    if (fold("down_l0", "conv_0", "conv_r00", 0) || fold("down_l1", "conv_0", "conv_r1", 0) ||
        fold("down_l2", "conv_0", "conv_r2", 0)) return 1;
    HIPCHK(hipStreamSynchronize(c->stream));
    c->gauge_active = c->gauge;
    c->fuse = c->gauge && c->prec == PREC_F16X3;
    return pack_wino(c);
}

static int load_weights(nbe_ctx* c, const nbe_layer_desc* descs, int n, bool style) {
    c->sst.valid = false;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    free_layers(c);
    for (int i = 0; i < n; ++i) {
        const nbe_layer_desc& d = descs[i];
        if (!d.block || !d.layer || !d.weight || !d.bias) return fail("layer %d: block, layer, weight and bias are required", i);
        Layer L;
        L.block = d.block; L.layer = d.layer; L.cout = d.cout; L.cin = d.cin; L.k = d.k;
        if (kind_of(d, &L.kind)) return 1;
        int ec, ei;
        if (expected_shape(c, L.block, L.layer, &ec, &ei)) return 1;
        if (ec != d.cout || ei != d.cin)
            return fail("%s/%s: weight shape (%d,%d,k) does not match the architecture (%d,%d,k)", d.block, d.layer, d.cout, d.cin, ec, ei);
        L.first = (L.block == "conv_l00") && (L.layer == "conv_0" || L.layer == "skip");     // nbody_emulator.py:243-246
        const size_t nw = (size_t)d.cout * d.cin * d.k * d.k * d.k;
        PackedW& pw = L.pw;
        pw = layer_geometry(c->prec, L.kind, d.cout, d.cin);
        HIPCHK(hipMalloc((void**)&pw.w, pw.floats * pw.nsets * 4));
        if (c->vel) HIPCHK(hipMalloc((void**)&pw.dw, pw.floats * pw.nsets * 4));
        const int nb = pw.ctiles * 32 * pw.ni;
        HIPCHK(hipMalloc((void**)&pw.bias, nb * 4));
        HIPCHK(hipMemset(pw.bias, 0, nb * 4));
        HIPCHK(hipMemcpy(pw.bias, d.bias, d.cout * 4, hipMemcpyHostToDevice));
        if (packs_narrow(c->prec, c->vel, L)) {
            PackedW& pn = L.pwn;                               // same layer, 16-cout tiles (conv_h3g_kernel<true>)
            pn = pw; pn.w = nullptr; pn.dw = nullptr;
            pn.cout_t = 16; pn.ctiles = 1;
            pn.floats = (int64_t)16 * mode_nseg(pn.mode) * mode_taps(pn.mode) * pn.cin_pad;
            HIPCHK(hipMalloc((void**)&pn.w, pn.floats * 4));
            if (L.kind == 1) HIPCHK(hipMalloc((void**)&pn.dw, pn.floats * 4));   // a skip that runs inside the narrow conv_1
        }
        if (packs_wino(c->prec, c->vel, L) && alloc_wino(pw)) return 1;
        if (packs_wino_skip(c->prec, c->vel, style, L)) {           // W_s and dW_s~
            HIPCHK(hipMalloc((void**)&pw.ww, pw.floats * 2 * 4));
            if (c->prec == PREC_F16) HIPCHK(hipMalloc((void**)&L.dwn_f, nw * 4));   // float16 model: Layer::dwn_f
        }
        if (packs_stem(c->prec, L) && alloc_stem(pw)) return 1;
        HIPCHK(hipMalloc((void**)&L.bias0, nb * 4));
        HIPCHK(hipMemcpy(L.bias0, pw.bias, nb * 4, hipMemcpyDeviceToDevice));
        for (int i = 0; i < d.cout; ++i)
            if (std::isfinite(d.bias[i])) c->bias_max = std::max(c->bias_max, std::fabs(d.bias[i]));
        HIPCHK(hipMalloc((void**)&L.wn, nw * 4));
        if (c->vel) HIPCHK(hipMalloc((void**)&L.dwn, nw * 4));
        if (style) {
            if (!d.style_weight || !d.style_bias) return fail("%s/%s: style_weight and style_bias are required", d.block, d.layer);
            HIPCHK(hipMalloc((void**)&L.weight, nw * 4));
            HIPCHK(hipMalloc((void**)&L.sw, d.cin * 2 * 4));
            HIPCHK(hipMalloc((void**)&L.sb, d.cin * 4));
            HIPCHK(hipMemcpy(L.weight, d.weight, nw * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.sw, d.style_weight, d.cin * 2 * 4, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(L.sb, d.style_bias, d.cin * 4, hipMemcpyHostToDevice));
        } else {
            if (c->vel && !d.dweight) return fail("%s/%s: dweight is required for premodulated velocity weights", d.block, d.layer);
            HIPCHK(hipMemcpy(L.wn, d.weight, nw * 4, hipMemcpyHostToDevice));
            if (c->vel) HIPCHK(hipMemcpy(L.dwn, d.dweight, nw * 4, hipMemcpyHostToDevice));
            launch_pack(L.wn, d.cout, d.cin, L.kind, pw, pw.w, c->stream);
            if (c->vel) launch_pack(L.dwn, d.cout, d.cin, L.kind, pw, pw.dw, c->stream);
            if (L.pwn.w) launch_pack(L.wn, d.cout, d.cin, L.kind, L.pwn, L.pwn.w, c->stream);
            if (L.pwn.dw) launch_pack(L.dwn, d.cout, d.cin, L.kind, L.pwn, L.pwn.dw, c->stream);
        }
        c->layers[L.block + "/" + L.layer] = L;
    }
    // completeness: 9 ResNet blocks x {skip, conv_0, conv_1} + 6 resample blocks x {conv_0} = 33 layers
    for (const char* b : kBlocks) {
        const bool rs = !strncmp(b, "down_", 5) || !strncmp(b, "up_", 3);
        const char* need[3] = {"conv_0", rs ? nullptr : "skip", rs ? nullptr : "conv_1"};
        for (const char* l : need)
            if (l && !find_layer(c, b, l)) return fail("parameter tree is missing %s/%s", b, l);
    }
    HIPCHK(hipStreamSynchronize(c->stream));
    c->have_weights = true; c->style = style; c->modulated = !style;
    c->mod_Om = NAN; c->mod_Dz = NAN;
    const char* ge = getenv("NBE_GAUGE");
    if (c->vel && !(ge && atoi(ge) == 0)) return style ? wire_gauge(c) : wire_gauge_premod(c, descs, n);
    if (!c->vel) {
        if (wire_novel(c)) return 1;
        if (!style) return pack_wino(c);                         // premodulated weights are final: pack their Winograd-z form now
    }
    return 0;
}

extern "C" {

int nbe_load_style_weights(nbe_ctx* c, const nbe_layer_desc* layers, int n) {
    if (!c || !layers) return fail("null argument");
    return load_weights(c, layers, n, true);
}

int nbe_load_premod_weights(nbe_ctx* c, const nbe_layer_desc* layers, int n) {
    if (!c || !layers) return fail("null argument");
    return load_weights(c, layers, n, false);
}

}  // extern "C"
