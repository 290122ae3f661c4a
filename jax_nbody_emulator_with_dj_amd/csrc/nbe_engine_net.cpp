// The network: tensors in the workspace arena, one convolution launch (run_conv), the blocks, and the U-Net schedule
// (style_nbody_emulator_vel_core.py:105-195) on whole tensors (network) and in z-slabs (network_stream).
#include "nbe_engine_internal.h"

// every consumer reads whole 16-channel chunks; PREC_F16 stores 8 channels per plane, the others 4 (or hi+lo of 8)
int planes_for(int C, int prec) { return roundup(C, 16) / (prec == PREC_F16 ? 8 : 4); }

static Planes ws_planes(nbe_ctx* c, int G, int D, int H, int W, int64_t* off_out) {
    Planes p;
    p.G = G; p.D = D; p.H = H; p.W = W;
    p.pstride = (p.vox() + 63) & ~int64_t(63);
    const int64_t one = (int64_t)G * p.pstride * 16;
    // slack: the conv kernels stream whole row segments and may read up to 2*H*W + 2*W + ~600 voxels past the
    // end of a plane for flat positions whose outputs are discarded (the last plane must not run off the arena)
    const int64_t slack = ((int64_t)2 * H * W + 2 * W + 1024) * 16;
    const int64_t off = c->arena.alloc(one * (c->vel ? 2 : 1) + slack);
    *off_out = off;
    if (!c->dry) {
        p.x = (float*)(c->ws + off);
        p.dx = c->vel ? (float*)(c->ws + off + one) : nullptr;
    }
    return p;
}

// (zero_rest = false: a tensor none of whose consumers reads a channel plane beyond C -- conv_r01's result, which the head reads)
Tensor talloc(nbe_ctx* c, int C, int D, int H, int W, bool zero_rest) {
    Tensor t;
    t.p = ws_planes(c, planes_for(C, c->prec), D, H, W, &t.off);
    // Channel planes beyond C (C not a multiple of 16: narrow test models) are read by the consumer against zero
    // weights but never written by the producer: they must hold finite values whatever an earlier call -- another
    // shape, a NaN in its input, an overflow -- left at this place of the arena.  No such planes at production width.
    const int gw = c->prec == PREC_F16 ? (C + 7) / 8 : c->prec == PREC_F16X3 ? 2 * ((C + 7) / 8) : (C + 3) / 4;
    if (zero_rest && !c->dry && t.off >= 0 && gw < t.p.G) {
        const size_t off = (size_t)gw * t.p.pstride * 4, bytes = (size_t)(t.p.G - gw) * t.p.pstride * 16;
        launch_zero(t.p.x + off, (int64_t)bytes, c->stream);
        if (t.p.dx) launch_zero(t.p.dx + off, (int64_t)bytes, c->stream);
    }
    return t;
}
// interior Hi x Wi plus a y/x halo of `pad`
Tensor tallocp(nbe_ctx* c, int C, int D, int Hi, int Wi, int pad, bool zero_rest) {
    Tensor t = talloc(c, C, D, Hi + 2 * pad, Wi + 2 * pad, zero_rest);
    t.pad = pad;
    return t;
}
// the interior as output planes: same strides, origin moved by (pad, pad)
static Planes inner(const Tensor& t) {
    Planes p = t.p;
    const int64_t sh = (int64_t)t.pad * (t.p.W + 1) * 4;
    if (p.x) p.x += sh;
    if (p.dx) p.dx += sh;
    return p;
}
void fill_halo(nbe_ctx* c, const Tensor& t) {
    if (t.pad > 0 && !c->dry) launch_fill_yx(t.p, t.pad, c->vel, c->stream);
}
void tfree(nbe_ctx* c, Tensor& t) { if (t.off >= 0) c->arena.release(t.off); t.off = -1; }
// planes [z0, z0 + nz) of every channel plane of t as a tensor of its own (not owning: pstride, H, W unchanged)
Tensor zview(const Tensor& t, int z0, int nz) {
    Tensor v = t;
    v.off = -1;
    const int64_t sh = (int64_t)z0 * t.p.H * t.p.W * 4;          // floats: one voxel of a plane is 16 bytes
    if (v.p.x) v.p.x += sh;
    if (v.p.dx) v.p.dx += sh;
    v.p.D = nz;
    v.org[0] += z0;
    return v;
}
// frame bookkeeping of the branch probe: a tensor produced from x by `nconv` 3x3x3 layers (VALID: same origin; periodic
// in y and x: the interior's origin moves one voxel out per layer)
static void org_conv(const Tensor& x, int nconv, int out[3]) {
    const int p = x.pad ? nconv : 0;
    out[0] = x.org[0]; out[1] = x.org[1] - p; out[2] = x.org[2] - p;
}
void set_org(Tensor& t, int z, int y, int x) { t.org[0] = z; t.org[1] = y; t.org[2] = x; }

// the float16 model's Winograd-z form (conv_h3w_kernel<., ., F16>): whole 32-channel stages
bool wino_f16_layer(int prec, bool vel, int cin_pad) {
    return prec == PREC_F16 && vel && cin_pad % (H3_CHUNK * H3W_F16_CHUNKS) == 0 && h3w_stages_fit(cin_pad, H3W_F16_CHUNKS);
}
bool wino_env_off() { return getenv("NBE_WINO") && atoi(getenv("NBE_WINO")) == 0; }   // A/B switch, read per launch
// f16-based arithmetic, Cin <= 64 and an input tangent wherever there is velocity: all eight parities of an up-sampling
// in one launch (up_h3_kernel: the input is read once)
bool up8_launch(const nbe_ctx* c, const Layer& L, bool has_dx) { return prec_is_half(c->prec) && (!c->vel || has_dx) && up8_fits(L.pw.cin_pad); }

// launch one convolution layer (or record it in a dry run)
int run_conv(nbe_ctx* c, const Layer& L, const ConvLaunch& cl_in, bool has_dx) {
    if (c->dry) return 0;
    ConvLaunch cl = cl_in;
    const bool g6 = c->gauge_active && L.g6 && has_dx;
    const bool nov = !c->vel && c->prec == PREC_F16X3 && L.kind == 0 && L.pw.ww && c->wino_ok;   // displacement only: conv_h3w_kernel<., NOVEL>
    if (c->gauge_active) { cl.gout = L.gout; cl.beta = g6 ? L.beta : nullptr; }
    if (cl.skw) {                                                // the block's skip runs inside this launch
        if (!((g6 || nov) && c->fuse && L.fskip)) return fail("internal error: fused skip requested for %s/%s", L.block.c_str(), L.layer.c_str());
        cl.bias = L.bias_f;
    }
    const PackedW& pw = (g6 && L.kind == 0 && L.pwn.w) ? L.pwn : L.pw;
    // Winograd along z (conv_h3w_kernel) is allowed: policy only -- whether this launch has that form is conv_select's
    // decision.  NBE_WINO=0 is the A/B switch (read per launch: tests flip it).
    cl.wino = c->wino_ok && !c->direct_z && !wino_env_off();
    hipEvent_t ea = nullptr, eb = nullptr;
    if (c->prof) {
        ea = get_event(c); eb = get_event(c);
        (void)hipEventRecord(ea, c->stream);
    }
    ConvKernel k;
    if (launch_conv(pw, cl, c->vel, has_dx, c->stream, &k))
        return fail("internal error: no kernel for layer %s/%s (mode %d, gauged %d, input tangent %d, crop offset %ld, output stride %d, selected %s)",
                    L.block.c_str(), L.layer.c_str(), L.pw.mode, (int)g6, (int)has_dx, (long)cl.in_off, cl.osz, conv_kernel_name(k));
    if (c->paths)
        *c->paths |= (cl.skw ? NBE_PATH_SKIP_FUSED : 0) | (cl.skw && (cl.flags & F_SKIP_NODX) ? NBE_PATH_SKIP_NODX : 0) |
                     (cl.csplit_ch ? NBE_PATH_TWO_SOURCE : 0) | (cl.skw && cl.sk_split_ch ? NBE_PATH_TWO_SOURCE_SKIP : 0) |
                     (conv_is_wino(k) ? (L.layer == "conv_1" ? NBE_PATH_WINO_1 : NBE_PATH_WINO_0) : 0) |
                     (conv_is_narrow(k) ? NBE_PATH_NARROW : 0) | (k == CONV_UP8 ? NBE_PATH_UP8 : 0);
    if (c->prof) {
        (void)hipEventRecord(eb, c->stream);
        std::string pn = conv_label(k, pw, c->vel, has_dx);     // the label of the kernel that ran
        static const bool per_layer = getenv("NBE_PROF_LAYERS") && atoi(getenv("NBE_PROF_LAYERS")) == 1;   // tools: one entry per layer
        if (per_layer) pn += " " + L.block + "/" + L.layer;
        const int pe = prof_entry(c, pn);
        c->pending.push_back({pe, ea, eb});
        // algorithmic FLOPs: 2*MAC over valid outputs; x3 with tangent (x2 when the input has no tangent, and for
        // the gauged form W.x, W.dx~)
        const double nout = (double)cl.Dv * cl.Hv * cl.Wv * (cl.set < 0 ? 8.0 : 1.0);
        const int taps = L.kind == 0 ? 27 : L.kind == 2 ? 8 : 1;
        const double gemms = c->vel ? ((has_dx && !g6) ? 3.0 : 2.0) : 1.0;
        c->prof_entries[pe].flops += 2.0 * nout * L.cout * L.cin * taps * gemms;
        if (cl.skw) c->prof_entries[pe].flops += 2.0 * nout * L.cout * L.fskip->cin * (!c->vel ? 1.0 : (cl.flags & F_SKIP_NODX) ? 2.0 : 3.0);   // W_s.x, [W_s.dx,] dW_s.x
        c->prof_entries[pe].launches += 1;
        if (c->pending.size() > 4096) prof_collect(c);
    }
    return 0;
}

const Layer* find_layer(nbe_ctx* c, const char* block, const char* layer) {
    auto it = c->layers.find(std::string(block) + "/" + layer);
    return it == c->layers.end() ? nullptr : &it->second;
}

// ------------------------------------------------------------------------------------------------
// schedule
// ------------------------------------------------------------------------------------------------

// A tile that is the whole periodic box: planes of periodic z context on either side of a level input's own planes.  Level 1:
// what conv_l1 reads beyond the box's own N / 2 planes for the N / 2 + 8 planes of the level-1 skip connection (4 + 2).
// Level 2 (also its y/x halo, in every periodic-yx tile): what levels 2 and 3 consume.  The same counts as a brick's faces.
static constexpr int L1_CTX = BRICK_H1, L2_CTX = BRICK_H2;

// StyleResNetBlock3DVel (style_blocks_vel.py:96-166): skip 1x1x1 cropped by 2, conv-act-conv, add, [act].
// Periodic-yx mode (x.pad = 1): y and x do not shrink -- every 3x3x3 convolution reads its input's wrap-around halo
// and writes the interior of a tensor of the same padded size, whose halo is filled afterwards; z shrinks as always.
// (has_dx false: conv_l00, whose skip reads the input field -- fused with F_SKIP_NODX)
// (displacement only: conv_h3w_kernel<SKIP, NOVEL> is the one kernel that runs a fused skip without a tangent)
// (the float16 model: as displacement only -- the Winograd-z kernel is the one kernel with a fused skip)
static bool wino_only_fuse(const nbe_ctx* c) { return !c->vel || c->prec == PREC_F16; }
// Does the block of conv_1 layer L1 run its skip fused, on `nres` result planes?  (displacement only and float16: the fused
// skip exists in conv_h3w_kernel alone, which pairs planes -- an odd number of result planes, and conv_c (direct_z), take
// the unfused path; slabs always have an even number)
bool block_fused(const nbe_ctx* c, const Layer* L1, int nres) {
    return c->fuse && L1->fskip != nullptr && (!wino_only_fuse(c) || (!c->direct_z && !wino_env_off() && h3w_pairs_planes(nres)));
}

// Can a fused decoder block read concat([skip, up]) from two tensors?  The kernels switch sources between whole K chunks: 16
// channels in conv_h3g_kernel / conv_h3w_kernel, 32 in the float16 model's Winograd-z form (the one kernel that fuses there).
bool two_source_width(const nbe_ctx* c) { return c->mid % two_source_chunk(c->prec) == 0; }

// hidden tensor of a block whose input x has `pad`: interior (Hi - sy) x (Wi - sy).  A fused block gives it the row
// and plane pitch of x (conv_h3g_kernel fetches the skip's patches of x with the offsets of its own input's).
Tensor alloc_hidden(nbe_ctx* c, int cmid, int nz, const Tensor& x, bool fused) {
    const int pad = x.pad, sy = pad ? 0 : 2;
    if (fused && !pad) return talloc(c, cmid, nz, x.p.H, x.p.W);
    return tallocp(c, cmid, nz, x.p.H - 2 * pad - sy, x.p.W - 2 * pad - sy, pad);
}

// The residual block's three launches on plane ranges of persistent tensors (the z-slab schedule; resblock() runs it over
// whole tensors).  Plane indices are in block-input coordinates (result plane j is centred on input plane j + 2): hidden
// planes [jh, jh + nh) and result planes [js, js + ns) are computed; what precedes them was carried over from the slab
// before.  h and s have the geometry resblock() gives them (s also serves as the skip / residual, in place).
// zr = {lo, hi, period} (branch probe): planes [lo, hi) of the block's result exist in a box periodic along z (nullptr: no wrap).
// x2: the block input is concat([x, x2]) along the channels (mid channels each, same geometry) without a concat tensor:
// the gauged f16x3 kernel reads its K chunks from two tensors (fused blocks only)
// halo_s = false: nothing reads the y/x halo of the result (conv_r01: the head reads the interior), so it is not filled
int resblock_part(nbe_ctx* c, const char* name, const Tensor& x, const Tensor& h, const Tensor& s,
                         int js, int ns, int jh, int nh, bool has_dx, bool final_act, const int* zr, const Tensor* x2, bool halo_s) {
    const Layer *Ls = find_layer(c, name, "skip"), *L0 = find_layer(c, name, "conv_0"), *L1 = find_layer(c, name, "conv_1");
    if (!Ls || !L0 || !L1) return fail("missing layers of block %s", name);
    const int H = x.p.H, W = x.p.W, pad = x.pad;
    const bool fused = block_fused(c, L1, ns);
    if (fused && (h.p.H != H || h.p.W != W)) return fail("internal: hidden tensor of fused block %s lacks the input's pitch", name);
    if (x2 && (!fused || x2->p.H != H || x2->p.W != W || x2->pad != pad)) return fail("internal: two-source input of block %s", name);
    const Tensor sv = zview(s, js, ns), hv = zview(h, jh, nh);
    const Tensor xs = zview(x, js, ns + 4);                      // what the skip of result planes [js, js + ns) reads
    const int64_t sk_off = (2L * H + (pad ? pad : 2)) * W + (pad ? pad : 2);   // skip: centre crop of x by the two convolutions
    // Unfused: the second convolution adds the skip as a residual and writes its result over it (every lane reads its
    // residual elements before it stores the same elements): one full-resolution tensor pair less at the workspace peak.
    // Fused (gauged f16x3): conv_1 computes the skip itself from x -- no skip launch, no residual round trip.
    if (!fused) {
        ConvLaunch cl; cl.in = xs.p; cl.in_off = sk_off;
        cl.Dv = ns; cl.Hv = s.p.H - 2 * pad; cl.Wv = s.p.W - 2 * pad; cl.out = inner(sv); cl.flags = 0;
        if (run_conv(c, *Ls, cl, has_dx)) return 1;
    }
    int og[3];
    {
        ConvLaunch cl; cl.in = zview(x, jh, nh + 2).p; cl.Dv = nh; cl.Hv = H - 2; cl.Wv = W - 2; cl.out = inner(hv); cl.flags = F_ACT;
        if (x2) { cl.in2 = zview(*x2, jh, nh + 2).p; cl.csplit_ch = c->mid; }
        if (run_conv(c, *L0, cl, has_dx)) return 1;
        org_conv(x, 1, og); og[0] += jh;                         // hidden plane j is centred on plane j + 1 of x
        const int zh[3] = {zr ? zr[0] : 0, zr ? zr[1] + 2 : 0, zr ? zr[2] : 0};
        probe_act(c, *L0, cl.out, 0, og, cl.Dv, cl.Hv, cl.Wv, pad != 0, zr ? zh : nullptr);
    }
    fill_halo(c, hv);
    {
        ConvLaunch cl; cl.in = zview(h, js, ns + 2).p; cl.Dv = ns; cl.Hv = s.p.H - 2 * pad; cl.Wv = s.p.W - 2 * pad; cl.out = inner(sv);
        if (fused) { cl.sk = xs.p; cl.sk_off = sk_off; cl.skw = L1->pwn.w ? &Ls->pwn : &Ls->pw; cl.flags = (final_act ? F_ACT : 0) | (has_dx ? 0 : F_SKIP_NODX);
                     if (x2) { cl.sk2 = zview(*x2, js, ns + 4).p; cl.sk_split_ch = c->mid; } }
        else { cl.res = inner(sv); cl.flags = F_RES | (final_act ? F_ACT : 0); }
        if (run_conv(c, *L1, cl, true)) return 1;
        org_conv(x, 2, og); og[0] += js;
        if (final_act) probe_act(c, *L1, cl.out, 0, og, cl.Dv, cl.Hv, cl.Wv, pad != 0, zr);
    }
    if (halo_s) fill_halo(c, sv);
    return 0;
}

// the block on whole tensors: its result is allocated (cout channels), the hidden tensor (cmid channels) lives meanwhile
// (hidden_out: a view of the released hidden tensor, whose planes stay as they are until the next allocation -- nbe_test_block)
// (zr, x2: as resblock_part)
int resblock(nbe_ctx* c, const char* name, const Tensor& x, bool has_dx, bool final_act, int cout, int cmid, Tensor* out,
                    Tensor* hidden_out, const int* zr, const Tensor* x2) {
    const Layer* L1 = find_layer(c, name, "conv_1");
    if (!L1) return fail("missing layers of block %s", name);
    const int D = x.p.D, pad = x.pad;
    const int sy = pad ? 0 : 2;                                  // what one 3x3x3 convolution takes off y and x
    Tensor s = tallocp(c, cout, D - 4, x.p.H - 2 * pad - 2 * sy, x.p.W - 2 * pad - 2 * sy, pad);
    Tensor h = alloc_hidden(c, cmid, D - 2, x, block_fused(c, L1, D - 4));
    if (s.off < 0 || h.off < 0) return fail("workspace exhausted in block %s", name);
    if (resblock_part(c, name, x, h, s, 0, D - 4, 0, D - 2, has_dx, final_act, zr, x2)) return 1;
    tfree(c, h);
    if (hidden_out) *hidden_out = h;
    int og[3];
    org_conv(x, 2, og);
    set_org(s, og[0], og[1], og[2]);
    *out = s;
    return 0;
}

// planes [src, src + n) of t -> planes [dst, dst + n) of the same tensor (the ranges must not overlap)
static void carry_planes(nbe_ctx* c, const Tensor& t, int src, int dst, int n) {
    if (c->dry || n <= 0) return;
    launch_crop(zview(t, src, n).p, 0, zview(t, dst, n).p, 0, c->vel, c->stream, 0);
}

// down-sampling layer L (stride 2) of x's interior into o's interior (o.pad > 0: the kernel writes where the next level reads,
// the caller fills the halo), which takes x's frame halved; probe: record its branches (zr: as probe_act)
int down_conv(nbe_ctx* c, const Layer& L, const Tensor& x, Tensor& o, bool probe, const int* zr) {
    ConvLaunch cl; cl.in = inner(x); cl.Dv = o.p.D; cl.Hv = o.p.H - 2 * o.pad; cl.Wv = o.p.W - 2 * o.pad; cl.out = inner(o); cl.flags = F_ACT;
    if (run_conv(c, L, cl, true)) return 1;
    set_org(o, x.org[0] / 2, x.org[1] / 2, x.org[2] / 2);
    // (periodic-yx: the interior only; its periodic images are copies)
    if (probe) probe_act(c, L, cl.out, 0, o.org, cl.Dv, cl.Hv, cl.Wv, x.pad != 0, zr);
    return 0;
}

// Periodic z context of a level input whose own planes [cz, D - cz) are complete, y/x halo included: the cz planes on either
// side are copies of the planes one period (= the own planes) away: plain plane copies.  A shallow box has fewer own planes
// than context planes (depth 8: 4 and 2 own planes against 6 and 10), so the context is built outward from the own planes
// in chunks of at most one period -- each chunk's source is own or already copied, and never overlaps its destination.
static void wrap_z(nbe_ctx* c, const Tensor& t, int cz) {
    const int own = t.p.D - 2 * cz;
    for (int done = 0; done < cz; done += own) {
        const int n = std::min(own, cz - done);
        carry_planes(c, t, cz - done - n + own, cz - done - n, n);   // below the planes [cz - done, ..)
        carry_planes(c, t, cz + done, cz + own + done, n);            // above the planes [.., cz + own + done)
    }
}

int downblock(nbe_ctx* c, const char* name, const Tensor& x, Tensor* out) {
    const Layer* L = find_layer(c, name, "conv_0");
    if (!L) return fail("missing layer %s/conv_0", name);
    Tensor o = talloc(c, c->mid, x.p.D / 2, x.p.H / 2, x.p.W / 2);
    if (o.off < 0) return fail("workspace exhausted in %s", name);
    if (down_conv(c, *L, x, o, true)) return 1;
    *out = o;
    return 0;
}

// channel planes of the first mid channels: the skip half of a concat tensor (not planes_for, which rounds up to 16
// channels -- narrow models store the up-sampled half right behind mid channels)
static int mid_planes(const nbe_ctx* c) { return c->mid / (c->prec == PREC_F16 ? 8 : 4); }

// up-sample into planes [mid/4, 2*mid/4) of the concat tensor (core :166-169: concat([skip, up]))
// (xcrop: centre crop of x in y and x before up-sampling; the result goes to the interior of cat)
// (g0 < 0: into the second half of a 2 * mid channel concat tensor; g0 = 0: into a mid channel tensor of its own)
int upblock(nbe_ctx* c, const char* name, const Tensor& x, const Tensor& cat, int xcrop, int g0) {
    const Layer* L = find_layer(c, name, "conv_0");
    if (!L) return fail("missing layer %s/conv_0", name);
    xcrop += x.pad;                                              // a periodic halo of x is not up-sampled either
    const int Hx = x.p.H - 2 * xcrop, Wx = x.p.W - 2 * xcrop;
    if (cat.p.D != 2 * x.p.D || cat.p.H - 2 * cat.pad != 2 * Hx || cat.p.W - 2 * cat.pad != 2 * Wx)
        return fail("internal: concat geometry mismatch in %s", name);
    const bool up8 = up8_launch(c, *L, true);
    const int out_g0 = g0 >= 0 ? g0 : mid_planes(c);
    for (int p = 0; p < (up8 ? 1 : 8); ++p) {
        ConvLaunch cl; cl.in = x.p; cl.in_off = ((int64_t)xcrop * x.p.W + xcrop);
        cl.Dv = x.p.D; cl.Hv = Hx; cl.Wv = Wx; cl.out = inner(cat);
        cl.out_g0 = out_g0; cl.osz = 2; cl.oz = (p >> 2) & 1; cl.oy = (p >> 1) & 1; cl.ox = p & 1;
        cl.flags = F_ACT; cl.set = up8 ? -1 : p;
        if (run_conv(c, *L, cl, true)) return 1;
    }
    // output voxel 2 i + parity comes from the input voxel i of the cropped interior (the crop beyond x's own halo)
    const int xc = xcrop - x.pad;
    const int og[3] = {2 * x.org[0], 2 * (x.org[1] + xc), 2 * (x.org[2] + xc)};
    probe_act(c, *L, inner(cat), out_g0, og, 2 * x.p.D, 2 * Hx, 2 * Wx, cat.pad != 0);
    return 0;
}

// the first mid channels of src, centre-cropped by `crop` in y and x and by `cz` in z (-1: by `crop`), into dst
void crop_into(nbe_ctx* c, const Tensor& src, int crop, const Tensor& dst, int cz) {
    if (c->dry) return;
    Planes s = src.p; s.G = mid_planes(c);
    launch_crop(s, crop, dst.p, 0, c->vel, c->stream, cz);
}

int check_dims(int D, int H, int W) {
    const int v[3] = {D, H, W};
    for (int i = 0; i < 3; ++i)
        if (v[i] < 104 || v[i] % 8 != 0)
            return fail("input spatial size %d unsupported: each of (D,H,W) must be >= 104 and a multiple of 8 "
                        "(all-VALID U-Net with three 2x levels, receptive-field crop 48)", v[i]);
    return 0;
}

void run_head(nbe_ctx* c, const Tensor& y, const Tensor& xin, const HeadOut& h, int zoff) {
    if (c->dry) return;
    // core :187-193 with the call's range shift s = 2^k divided out (exact): disp = (y + x0) * 6 / s,
    // vel = dy * (vf * 6 / s) + x0 * (vf * 6 / (Dz * s))
    const float inv_s = 1.0f / c->act_scale;
    HeadScale hs;
    hs.k_disp = 6.0f * inv_s; hs.k_dy = h.vel_fac * 6.0f * inv_s; hs.k_x0 = h.vel_fac * 6.0f / h.Dz * inv_s;
    hs.bad = c->flags ? (int*)(c->flags + 1) : nullptr;
    launch_head(y.p, xin.p, 48, c->out_chan, hs, c->vel, h.disp, h.velo, h.out_dtype, h.OD, h.OH, h.OW,
                h.a0 + zoff, h.a1, h.a2, c->prec, c->stream, y.pad);
}

// The same network with the two full-resolution levels run in slabs of S output planes (S even): the encoder blocks
// conv_l00 / conv_l01 (+ the crop of the skip connection and down_l0) and the decoder blocks up_r0 / conv_r00 /
// conv_r01 (+ head) only ever hold slab-sized tensors, so a tile can be as deep as the box (no halo recompute along
// z inside it) at a fraction of the workspace.  Neighbouring slabs recompute the 2-plane overlaps of the 3x3x3
// layers: (S + 6) / S on the first hidden tensor, less further down.  Everything is the whole-tensor schedule on
// z-views of the same tensors; results are identical.
//
// Periodic-yx mode (tin.pad = 1: the tile spans the whole periodic box in y and x).  The two full-resolution levels
// do not pad-and-shrink in y and x: their tensors are N + 2 wide, every 3x3x3 convolution reads the wrap-around halo
// of its input and the halo of its output is filled afterwards -- the same arithmetic per voxel as the reference's
// 48-voxel periodic padding, without computing the halo voxels (about 10 % of the FLOPs of a 512^3 box).  Level 1 runs
// the same way on the interior that down_l0 writes straight into its input tensor; levels 2 and 3 keep the padded scheme
// on the 10 voxels of periodic context that stream_level1 gives the level-2 input; up_r0 takes the centre of the level-1
// result.
static int stream_encode(nbe_ctx* c, const Tensor& tin, const HeadOut& ho, int S, Tensor* skip0_out, Tensor* td_out) {
    const int m = c->mid, pad = tin.pad;
    const int D = tin.p.D, H = tin.p.H, W = tin.p.W;
    const int Hi = H - 2 * pad, Wi = W - 2 * pad;
    const int Y = D - 8;                                          // planes of the level-0 encoder output
    // Periodic in z too (the tile is the whole box): the 40 outermost planes of the level-0 encoder output on either
    // side only feed the lower levels, whose input can be extended periodically in z just as in y and x.  The encoder
    // then produces the Y - 80 planes of the skip connection only, and down_l0 the box's own (D - 96) / 2 planes.
    const bool zx = pad && c->zx;                                 // brick mode: as pz, the z context of level 1 comes from the neighbours
    const bool pz = pad && (c->pz || zx);
    // brick mode: the brick's own D - 96 planes of the skip connection only (planes 4 .. of the tensor) -- the four on either
    // side that the decoder reads as well are the neighbours' own planes and arrive by exchange (network_stream)
    const int zlo = pz ? (zx ? 44 : 40) : 0, zhi = pz ? (zx ? Y - 44 : Y - 40) : Y;
    // the level-0 skip connection: centre crop by 40 (z only in periodic-yx mode)
    Tensor skip0 = pad ? tallocp(c, m, Y - 80, Hi, Wi, pad) : talloc(c, m, Y - 80, H - 88, W - 88);
    // down_l0 output.  Periodic-yx: down_l0 writes the interior of the level-1 input itself (1-voxel y/x halo; periodic in z,
    // L1_CTX planes of context on either side of the box's own N / 2), which stream_level1 completes.  Brick mode keeps a
    // tensor of the interior alone (td): its faces travel to the neighbours as they are.
    const int cz1 = (pz && !zx) ? L1_CTX : 0, dpad = (pad && !zx) ? 1 : 0;
    const int D1 = pz ? (D - 96) / 2 : Y / 2;
    Tensor td = pad ? tallocp(c, m, D1 + 2 * cz1, Hi / 2, Wi / 2, dpad) : talloc(c, m, Y / 2, (H - 8) / 2, (W - 8) / 2);
    if (skip0.off < 0 || td.off < 0) return fail("workspace exhausted (level 0)");
    const Layer* Ld = find_layer(c, "down_l0", "conv_0");
    if (!Ld) return fail("missing layer down_l0/conv_0");
    // Persistent slab tensors of the level-0 encoder: hidden and result of conv_l00 (h0, a), hidden of conv_l01 (h1)
    // and, unless the slabs land in the skip tensor directly, its result (y0).  Consecutive slabs overlap by 6 / 4 / 2
    // planes of h0 / a / h1: those are carried over from the slab before (a copy of a few planes) instead of being
    // recomputed, so every layer computes every plane exactly once.
    const int sy = pad ? 0 : 2;
    const Layer* L00 = find_layer(c, "conv_l00", "conv_1");
    if (!L00) return fail("missing layer conv_l00/conv_1");
    Tensor h0 = alloc_hidden(c, m, S + 6, tin, block_fused(c, L00, S + 4)), a = tallocp(c, m, S + 4, Hi - 2 * sy, Wi - 2 * sy, pad);
    const Layer *L01 = find_layer(c, "conv_l01", "conv_1"), *Lr00 = find_layer(c, "conv_r00", "conv_1"), *Lr01 = find_layer(c, "conv_r01", "conv_1");
    if (!L01 || !Lr00 || !Lr01) return fail("missing conv_1 layers of the level-0 blocks");
    Tensor h1 = alloc_hidden(c, m, S + 2, a, block_fused(c, L01, S));
    Tensor y0r = pz ? Tensor() : tallocp(c, m, S, Hi - 4 * sy, Wi - 4 * sy, pad);
    if (h0.off < 0 || a.off < 0 || h1.off < 0 || (!pz && y0r.off < 0)) return fail("workspace exhausted (level-0 encoder slabs)");
    // (branch probe: periodic in z, the planes [zlo, zhi + 4) of conv_l00's result and [zlo, zhi) of conv_l01's exist)
    const int zr00[3] = {zlo, zhi + 4, pz ? D - 96 : 0}, zr01[3] = {zlo, zhi, pz ? D - 96 : 0};
    // Pipelined host path: the first slab is short (PIPE_EDGE planes), so that the kernels start as soon as a small first
    // upload has landed; the decoder's last slab is short for the same reason at the other end (its copy to the host is
    // the only one nothing hides).  Slabs start on even planes either way, so the fields do not change.
    for (int z = zlo, n = 0; z < zhi; z += n) {
        n = std::min(((c->pipe.active || c->pipe.slabwise) && z == zlo) ? std::min(S, PIPE_EDGE) : S, zhi - z);
        const int n_next = std::min(S, zhi - (z + n));
        const bool first = z == zlo;
        // periodic in z: the slab is exactly planes [z - 40, z - 40 + n) of the skip connection -- write it there
        Tensor y0 = pz ? zview(skip0, z - 40, n) : zview(y0r, 0, n);
        if ((c->pipe.active || c->pipe.slabwise) && !c->dry && pipe_input(c, tin, z, z + n + 8, n_next, ho.Dz / 6.0f * c->act_scale)) return 1;
        // frames (branch probe): plane j of the persistent slab tensors is plane z + j of the layer's whole tensor
        { int og[3]; org_conv(zview(tin, z, n + 8), 2, og); set_org(a, og[0], og[1], og[2]);
          org_conv(a, 2, og); set_org(y0, og[0], og[1], og[2]); }
        if (first) {
            if (resblock_part(c, "conv_l00", zview(tin, z, n + 8), h0, a, 0, n + 4, 0, n + 6, false, true, zr00)) return 1;
            if (resblock_part(c, "conv_l01", a, h1, y0, 0, n, 0, n + 2, true, true, zr01)) return 1;
        } else {
            if (resblock_part(c, "conv_l00", zview(tin, z, n + 8), h0, a, 4, n, 6, n, false, true, zr00)) return 1;
            if (resblock_part(c, "conv_l01", a, h1, y0, 0, n, 2, n, true, true, zr01)) return 1;
        }
        if (z + n < zhi) {                                       // what the next slab will not recompute
            carry_planes(c, h0, n, 0, 6);
            carry_planes(c, a, n, 0, 4);
            carry_planes(c, h1, n, 0, 2);
        }
        const int i0 = std::max(0, 40 - z), i1 = std::min(n, Y - 40 - z);      // planes of this slab inside the crop
        if (!pz && i1 > i0) crop_into(c, y0, pad ? 0 : 40, zview(skip0, z + i0 - 40, i1 - i0), i0);
        {
            // planes [d0, d1) of this slab go through down_l0 (periodic in z: only the box's own planes, 44 .. Y - 44)
            const int d0 = pz ? std::max(z, 44) : z, d1 = pz ? std::min(z + n, Y - 44) : z + n;
            if (d1 > d0) {
                const Tensor tv = zview(td, cz1 + (d0 - (pz ? 44 : 0)) / 2, (d1 - d0) / 2);
                Tensor yv = zview(y0, d0 - z, d1 - d0);
                ConvLaunch cl; cl.in = inner(yv); cl.Dv = tv.p.D; cl.Hv = tv.p.H - 2 * dpad; cl.Wv = tv.p.W - 2 * dpad; cl.out = inner(tv); cl.flags = F_ACT;
                if (run_conv(c, *Ld, cl, true)) return 1;
                const int og[3] = {yv.org[0] / 2, yv.org[1] / 2, yv.org[2] / 2};
                const int zd[3] = {22, 22 + (D - 96) / 2, pz ? (D - 96) / 2 : 0};   // periodic in z: the box's own N / 2 planes
                probe_act(c, *Ld, cl.out, 0, og, cl.Dv, cl.Hv, cl.Wv, pad != 0, zd);     // periodic-yx: down_l0 ran on the interior only
            }
        }
    }
    tfree(c, h0); tfree(c, a); tfree(c, h1);
    if (!pz) tfree(c, y0r);
    // frames: the skip connection is conv_l01's result cropped by 40 (its frame starts 40 voxels in; periodic-yx keeps all
    // of y and x, whose interior sits 44 voxels into the padded frame); down_l0's output starts at plane 44 / 2 when the
    // encoder only produced the box's own planes (pz), cz1 planes of context before them
    set_org(skip0, 0, pad ? 4 : 0, pad ? 4 : 0);
    set_org(td, pz ? 22 - cz1 : 0, pad ? 22 : 0, pad ? 22 : 0);
    *skip0_out = skip0; *td_out = td;
    return 0;
}

// Level 1 of the encoder (whole tensors, and the z-slab schedule outside brick mode): the down_l0 output td -> conv_l1's
// result, from which come the level-1 skip connection and the level-2 input t.
// Periodic-yx: level 1 runs periodic in y and x as well.  td is its input already -- down_l0 wrote the interior of the box's
// own planes (stream_encode); here their 1-voxel wrap-around halo is filled and, periodic in z, the L1_CTX planes of context on
// either side are copied from the own planes one period away.  conv_l1 then computes N / 2 + 8 planes: exactly the skip
// connection.  Level 2 and below keep the padded scheme, and get their context the same way: down_l1 runs on the box's own
// planes and writes the interior of the level-2 input, whose L2_CTX voxels of y/x halo are filled and whose L2_CTX planes of z
// context are copied.  (A tile that is not the whole box in z has no periodic images along z: conv_l1 and down_l1 run on
// all planes, and the skip connection is the result cropped by 16 planes.)
// The skip connection: a fused conv_r1 at a two-source width reads it where it is -- conv_l1's result stays alive (*y1_out)
// and no concat tensor is formed (lower_levels); otherwise it is copied into the first half of the concat tensor *cat1_out.
static int stream_level1(nbe_ctx* c, int pad, bool pz, Tensor td, Tensor* cat1_out, Tensor* y1_out, Tensor* t_out) {
    const int m = c->mid;
    Tensor t = td, y1, cat1;
    *y1_out = Tensor();
    if (!pad) {
        if (resblock(c, "conv_l1", t, true, true, m, m, &y1)) return 1;
        tfree(c, t);
        cat1 = talloc(c, 2 * m, y1.p.D - 32, y1.p.H - 32, y1.p.W - 32);
        if (cat1.off < 0) return fail("workspace exhausted (cat1)");
        crop_into(c, y1, 16, cat1);
        if (downblock(c, "down_l1", y1, &t)) return 1;
        tfree(c, y1);
        *cat1_out = cat1; *t_out = t;
        return 0;
    }
    const int cz1 = pz ? L1_CTX : 0, cz2 = pz ? L2_CTX : 0;
    fill_halo(c, zview(t, cz1, t.p.D - 2 * cz1));
    wrap_z(c, t, cz1);
    // (branch probe: periodic in z, planes [16, 16 + N / 2 + 8) of conv_l1's result exist, and the box's own N / 4 of down_l1's)
    const int zr1[3] = {t.org[0], t.org[0] + t.p.D - 4, t.p.D - 2 * cz1};
    if (resblock(c, "conv_l1", t, true, true, m, m, &y1, nullptr, pz ? zr1 : nullptr)) return 1;
    tfree(c, t);

    const int zc = pz ? 0 : 16;                                   // planes of y1 on either side of the skip connection
    const Layer *Lr1 = find_layer(c, "conv_r1", "conv_1"), *Ld1 = find_layer(c, "down_l1", "conv_0");
    if (!Lr1 || !Ld1) return fail("missing layer conv_r1/conv_1 or down_l1/conv_0");
    const bool two = block_fused(c, Lr1, y1.p.D - 2 * zc - 4) && two_source_width(c);
    if (!two) {
        cat1 = tallocp(c, 2 * m, y1.p.D - 2 * zc, y1.p.H - 2, y1.p.W - 2, 1);
        if (cat1.off < 0) return fail("workspace exhausted (cat1)");
        crop_into(c, y1, 0, cat1, zc);
        set_org(cat1, y1.org[0] + zc - 16, y1.org[1] - 16, y1.org[2] - 16);   // the skip connection's frame starts 16 voxels into y1's on every axis
    }
    Tensor y1d = pz ? zview(y1, 4, y1.p.D - 8) : y1;              // what down_l1 runs on
    t = talloc(c, m, y1d.p.D / 2 + 2 * cz2, (y1.p.H - 2) / 2 + 2 * L2_CTX, (y1.p.W - 2) / 2 + 2 * L2_CTX);
    if (t.off < 0) return fail("workspace exhausted (level 2 input)");
    Tensor tp = zview(t, cz2, y1d.p.D / 2);                       // its own planes as a tensor with a y/x halo
    tp.pad = L2_CTX;
    const int zd[3] = {y1d.org[0] / 2, y1d.org[0] / 2 + tp.p.D, tp.p.D};
    if (down_conv(c, *Ld1, y1d, tp, true, pz ? zd : nullptr)) return 1;
    fill_halo(c, tp);
    wrap_z(c, t, cz2);
    set_org(t, tp.org[0] - cz2, tp.org[1] - L2_CTX, tp.org[2] - L2_CTX);
    if (two) *y1_out = y1; else tfree(c, y1);
    *cat1_out = cat1; *t_out = t;
    return 0;
}

// Levels 2 and 3 and the level-1 decoder: the level-2 input t and the level-1 skip connection -> the level-1 decoder output
// (conv_r1) in *r_out.  The skip connection is the first half of the concat tensor cat1, or (y1.off >= 0, stream_level1) the
// centre planes of conv_l1's result y1: conv_r1 then reads concat([skip, up]) from two tensors, as the level-0 decoder does.
static int lower_levels(nbe_ctx* c, Tensor t, Tensor cat1, Tensor y1, Tensor* r_out) {
    const int m = c->mid;
    Tensor y2, cat2, r;
    if (resblock(c, "conv_l2", t, true, true, m, m, &y2)) return 1;
    tfree(c, t);
    cat2 = talloc(c, 2 * m, y2.p.D - 8, y2.p.H - 8, y2.p.W - 8);
    if (cat2.off < 0) return fail("workspace exhausted (cat2)");
    crop_into(c, y2, 4, cat2);
    if (downblock(c, "down_l2", y2, &t)) return 1;
    tfree(c, y2);

    // Level 3 runs on the direct kernels: its plane count (D / 8 - 2, - 4 for a tile of D planes) is even or odd with the cut
    // of the box, and the Winograd-z kernel pairs planes -- a voxel's bits would depend on the tile or brick it falls in.
    // (Levels 0 - 2 launch even plane counts from even planes for every tile and brick.)  0.1 % of the 512^3 box's kernel time.
    c->direct_z = true;
    const int rc = resblock(c, "conv_c", t, true, true, m, m, &r);
    c->direct_z = false;
    if (rc) return 1;
    tfree(c, t);

    if (upblock(c, "up_r2", r, cat2)) return 1;
    tfree(c, r);
    if (resblock(c, "conv_r2", cat2, true, true, m, 2 * m, &r)) return 1;
    tfree(c, cat2);

    const bool two = y1.off >= 0;
    Tensor sk;
    if (two) {                                                   // the up-sampled half in a mid-channel tensor of its own
        cat1 = tallocp(c, m, 2 * r.p.D, y1.p.H - 2, y1.p.W - 2, 1);
        if (cat1.off < 0) return fail("workspace exhausted (up_r1)");
        sk = zview(y1, (y1.p.D - 2 * r.p.D) / 2, 2 * r.p.D);
        set_org(sk, sk.org[0] - 16, y1.org[1] - 16, y1.org[2] - 16);   // the skip connection's frame starts 16 voxels into y1's on every axis
        set_org(cat1, sk.org[0], sk.org[1], sk.org[2]);
    }
    // periodic-yx (cat1.pad = 1): the level-2 result carries 2 voxels of y/x context that the periodic level 1 does not need
    if (upblock(c, "up_r1", r, cat1, cat1.pad ? 2 : 0, two ? 0 : -1)) return 1;
    fill_halo(c, cat1);
    tfree(c, r);
    if (resblock(c, "conv_r1", two ? sk : cat1, true, true, m, 2 * m, r_out, nullptr, nullptr, two ? &cat1 : nullptr)) return 1;
    tfree(c, cat1);
    if (two) tfree(c, y1);
    return 0;
}

// the network body on whole tensors of a resident input tensor; returns conv_r01's output tensor (out_chan channels).  Only
// the level-0 encoder and decoder differ from the z-slab schedule (network_stream).
int network(nbe_ctx* c, const Tensor& tin, Tensor* yout) {
    const int m = c->mid;
    Tensor a, y0, t, cat0, cat1, y1, r;
    if (resblock(c, "conv_l00", tin, false, true, m, m, &a)) return 1;
    if (resblock(c, "conv_l01", a, true, true, m, m, &y0)) return 1;
    tfree(c, a);
    cat0 = talloc(c, 2 * m, y0.p.D - 80, y0.p.H - 80, y0.p.W - 80);
    if (cat0.off < 0) return fail("workspace exhausted (cat0)");
    crop_into(c, y0, 40, cat0);
    if (downblock(c, "down_l0", y0, &t)) return 1;
    tfree(c, y0);

    if (stream_level1(c, 0, false, t, &cat1, &y1, &t)) return 1;
    if (lower_levels(c, t, cat1, y1, &r)) return 1;

    if (upblock(c, "up_r0", r, cat0)) return 1;
    tfree(c, r);
    if (resblock(c, "conv_r00", cat0, true, true, m, 2 * m, &r)) return 1;
    tfree(c, cat0);

    if (resblock(c, "conv_r01", r, true, false, c->out_chan, m, yout)) return 1;
    tfree(c, r);
    return 0;
}

// Everything from the level-2 input on: levels 2-3, the level-1 decoder, then the level-0 decoder slab by slab with the head.
// (cat1, y1: the level-1 skip connection in either of its forms, lower_levels)
static int stream_tail(nbe_ctx* c, const Tensor& tin, const HeadOut& ho, int S, Tensor skip0, Tensor cat1, Tensor y1, Tensor t) {
    const int m = c->mid, pad = tin.pad;
    const int sy = pad ? 0 : 2;
    const Layer *Lr00 = find_layer(c, "conv_r00", "conv_1"), *Lr01 = find_layer(c, "conv_r01", "conv_1");
    if (!Lr00 || !Lr01) return fail("missing conv_1 layers of the level-0 blocks");
    Tensor r;                                                    // the level-1 decoder output
    if (lower_levels(c, t, cat1, y1, &r)) return 1;
    if (2 * r.p.D != skip0.p.D || 2 * (r.p.H - 2 * r.pad) != skip0.p.H - 2 * pad || 2 * (r.p.W - 2 * r.pad) != skip0.p.W - 2 * pad)
        return fail("internal: level-0 concat geometry mismatch");

    if (pad && c->zx && !c->dry && c->bio.skip_recv_lo) {
        // brick mode: the neighbours' planes of the skip connection, below and above the brick's own -- the last of the four
        // exchanges to be needed; it travelled while levels 1-3 ran, and only now does the stream wait for it
        if (c->bio.skip_ready) HIPCHK(hipStreamWaitEvent(c->stream, c->bio.skip_ready, 0));
        brick_recv(c, skip0, c->bio.skip_recv_lo, c->bio.skip_recv_hi, BRICK_H0, skip0, 0);
    }
    const int Yo = skip0.p.D - 8;                                 // output planes (= D - 96)
    // Persistent slab tensors of the level-0 decoder, with the same carry-over of the overlaps (8 / 6 / 4 / 2 planes of
    // the concat tensor, the hidden and the result of conv_r00, the hidden of conv_r01).
    const int Hs = skip0.p.H - 2 * pad, Ws = skip0.p.W - 2 * pad;
    // Fused blocks on the gauged f16x3 kernel read concat([skip, up]) from two tensors (core :168-169 without the concat):
    // the slab's planes of the skip connection where they are, the up-sampled half in a mid-channel tensor of its own.
    const bool two = block_fused(c, Lr00, S + 4) && two_source_width(c);
    Tensor cat = tallocp(c, two ? m : 2 * m, S + 8, Hs, Ws, pad), hq = alloc_hidden(c, 2 * m, S + 6, cat, block_fused(c, Lr00, S + 4));
    Tensor q = tallocp(c, m, S + 4, Hs - 2 * sy, Ws - 2 * sy, pad), hy = alloc_hidden(c, m, S + 2, q, block_fused(c, Lr01, S));
    // conv_r01's result: the head reads out_chan channels of its interior and nothing else does -- its padding channel planes are
    // not zeroed and its y/x halo is not filled
    Tensor y = tallocp(c, c->out_chan, S, Hs - 4 * sy, Ws - 4 * sy, pad, false);
    if (cat.off < 0 || hq.off < 0 || q.off < 0 || hy.off < 0 || y.off < 0) return fail("workspace exhausted (level-0 decoder slabs)");
    for (int z = 0, n = 0; z < Yo; z += n) {
        n = std::min(S, Yo - z);
        if (c->pipe.active && c->pipe.out_async && Yo - z > PIPE_EDGE && Yo - z - n < PIPE_EDGE)
            n = Yo - z - PIPE_EDGE;                              // leave a short last slab (pipelined host path, see stream_encode)
        const bool first = z == 0;
        const int c0 = first ? 0 : 8, cn = first ? n + 8 : n;     // new planes of the concat tensor: [c0, c0 + cn)
        set_org(cat, skip0.org[0] + z, skip0.org[1], skip0.org[2]);  // slab-local plane j of the concat is plane z + j of the skip connection
        { int og[3]; org_conv(cat, 2, og); set_org(q, og[0], og[1], og[2]); }
        if (!two && !c->dry) launch_crop(zview(skip0, z + c0, cn).p, 0, zview(cat, c0, cn).p, 0, c->vel, c->stream, 0);
        if (upblock(c, "up_r0", zview(r, (z + c0) / 2, cn / 2), zview(cat, c0, cn), 0, two ? 0 : -1)) return 1;
        fill_halo(c, zview(cat, c0, cn));
        // two sources: slab-local plane j of the concat is plane z + j of the skip connection
        const Tensor sk = two ? zview(skip0, z, std::min(S + 8, skip0.p.D - z)) : cat;
        const Tensor* up2 = two ? &cat : nullptr;
        if (first) {
            if (resblock_part(c, "conv_r00", sk, hq, q, 0, n + 4, 0, n + 6, true, true, nullptr, up2)) return 1;
            if (resblock_part(c, "conv_r01", q, hy, y, 0, n, 0, n + 2, true, false, nullptr, nullptr, false)) return 1;
        } else {
            if (resblock_part(c, "conv_r00", sk, hq, q, 4, n, 6, n, true, true, nullptr, up2)) return 1;
            if (resblock_part(c, "conv_r01", q, hy, y, 0, n, 2, n, true, false, nullptr, nullptr, false)) return 1;
        }
        if (z + n < Yo) {
            carry_planes(c, cat, n, 0, 8);
            carry_planes(c, hq, n, 0, 6);
            carry_planes(c, q, n, 0, 4);
            carry_planes(c, hy, n, 0, 2);
        }
        run_head(c, zview(y, 0, n), zview(tin, z, n + 96), ho, z);
        if (c->pipe.active && c->pipe.out_async && !c->dry && pipe_output(c, z, n)) return 1;
        if (c->prog && !c->dry && z + n < Yo)                    // the tile's last slab is reported by the sub-box loop
            c->prog->post(c->pipe.active && c->pipe.out_async ? c->down_stream : c->stream,
                          c->prog_k * 1000 + (int)(1000L * (z + n) / Yo), c->prog_n * 1000);
    }
    tfree(c, cat); tfree(c, hq); tfree(c, q); tfree(c, hy); tfree(c, y);
    tfree(c, r); tfree(c, skip0);
    return 0;
}

static void stash_arena(nbe_ctx* c) { c->sst.blks = c->arena.blks; c->sst.high = c->arena.high; }

// phase 0: the whole schedule.  Brick mode (c->zx): 1 = encoder + faces of the down_l0 output, 2 = the interior of conv_l1,
// 3 = with the received faces up to the faces of the down_l1 output, 4 = with those, everything else.  The arena keeps the
// tensors in between (c->sst); any other use of the context drops them (sst.valid).
int network_stream(nbe_ctx* c, const Tensor& tin, const HeadOut& ho, int S) {
    auto& st = c->sst;
    const int pad = tin.pad;
    const bool zx = pad && c->zx;
    if (c->phase >= 2) {
        if (!st.valid || st.stage != c->phase - 1) return fail("brick calls out of order (encode, interior, exchange, finish) or the context was used in between");
        c->arena.blks = st.blks; c->arena.high = st.high;
    }
    if (c->phase <= 1) {
        if (stream_encode(c, tin, ho, S, &st.skip0, &st.td)) return 1;
        st.tin = tin; st.S = S;
        if (c->phase == 1) {
            // the boundary planes of the down_l0 output for the neighbours
            brick_send(c, st.td, 0, BRICK_H1, c->bio.send_lo, c->bio.send_hi);
            // ... and the first / last four of the brick's own planes of the skip connection (planes 4 .. D - 4 of the tensor)
            brick_send(c, st.skip0, BRICK_H0, BRICK_H0, c->bio.skip_send_lo, c->bio.skip_send_hi);
            st.valid = true; st.stage = 1; stash_arena(c);
            return 0;
        }
    }
    if (!zx) {
        Tensor cat1, y1, t;
        if (stream_level1(c, pad, pad && c->pz, st.td, &cat1, &y1, &t)) return 1;
        return stream_tail(c, tin, ho, S, st.skip0, cat1, y1, t);
    }
    if (c->phase == 0 || c->phase == 2) {
        if (brick_interior(c, st)) return 1;
        if (c->phase == 2) { st.stage = 2; stash_arena(c); return 0; }
    }
    if (c->phase == 0 || c->phase == 3) {
        if (brick_edges(c, st)) return 1;
        if (c->phase == 3) { st.stage = 3; stash_arena(c); return 0; }
    }
    Tensor t;
    if (brick_level2(c, st, &t)) return 1;
    st.valid = false;
    return stream_tail(c, st.tin, ho, st.S, st.skip0, st.cat1, Tensor(), t);
}

// periodic-yx tiles: z as usual; y and x are the box itself (+ 2 halo voxels), a multiple of 8 and at least 48, so that the
// 10 voxels of y/x halo of the level-2 input fit its extent of at least 12.  z has no such bound:
// a tile that is the whole box in z may be 8 planes deep, and the periodic z context of the level-1 and level-2 inputs
// (6 and 10 planes) then spans several periods (wrap_z)
int check_dims_pyx(int D, int H, int W) {
    if (D < 104 || D % 8 != 0) return fail("input depth %d unsupported: must be >= 104 and a multiple of 8", D);
    const int v[2] = {H - 2, W - 2};
    for (int i = 0; i < 2; ++i)
        if (v[i] < 48 || v[i] % 8 != 0) return fail("periodic extent %d unsupported: must be >= 48 and a multiple of 8", v[i]);
    return 0;
}
