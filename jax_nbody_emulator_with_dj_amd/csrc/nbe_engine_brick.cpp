// Brick mode of the sharded box: one rank's z-slab of a periodic box (include/nbe.h, "Brick mode").
#include "nbe_engine_internal.h"

// ---- the steps of a brick inside network_stream (BRICK_H0 / BRICK_H1 / BRICK_H2: nbe_engine_internal.h) -----------------
static Planes brick_planes(nbe_ctx* c, const Tensor& like, const void* buf, int nplanes) {
    Planes p = like.p;
    p.D = nplanes;
    p.pstride = (p.vox() + 63) & ~int64_t(63);
    p.x = (float*)buf;
    p.dx = c->vel ? (float*)buf + (int64_t)p.G * p.pstride * 4 : nullptr;
    return p;
}
// faces for the neighbours: planes [in, in + n) of t -> lo, the mirror planes [D - in - n, D - in) -> hi
void brick_send(nbe_ctx* c, const Tensor& t, int in, int n, void* lo, void* hi) {
    if (c->dry) return;
    for (int s = 0; s < 2; ++s)
        launch_crop(zview(t, s ? t.p.D - in - n : in, n).p, 0, brick_planes(c, t, s ? hi : lo, n), 0, c->vel, c->stream, 0);
}
// the neighbours' faces (n planes shaped like `like`) -> the first (lo) and the last (hi) n planes of dst: wrap > 0 extends
// them periodically by that many voxels in y and x (a level input), 0 copies them as they are (the skip connection)
void brick_recv(nbe_ctx* c, const Tensor& like, const void* lo, const void* hi, int n, const Tensor& dst, int wrap) {
    if (c->dry) return;
    for (int s = 0; s < 2; ++s) {
        const Planes face = brick_planes(c, like, s ? hi : lo, n), to = zview(dst, s ? dst.p.D - n : 0, n).p;
        if (wrap) launch_wrap_pad(face, to, wrap, c->vel, c->stream, 0);
        else launch_crop(face, 0, to, 0, c->vel, c->stream, 0);
    }
}
static int64_t brick_halo_bytes(nbe_ctx* c, int nplanes, int Hd, int Wd) {
    Planes p; p.G = planes_for(c->mid, c->prec); p.D = nplanes; p.H = Hd; p.W = Wd;
    p.pstride = (p.vox() + 63) & ~int64_t(63);
    return (int64_t)p.G * p.pstride * 16 * (c->vel ? 2 : 1);
}

// conv_l1 on plane ranges of the whole level-1 tensors (resblock_part): part 0 = what depends on the brick's own planes only,
// part 1 = the planes next to the low face, part 2 = next to the high face
static int brick_conv_l1(nbe_ctx* c, const Tensor& t, const Tensor& h, const Tensor& y1, int part) {
    const int B = t.p.D - 2 * BRICK_H1;
    if (part == 0) return resblock_part(c, "conv_l1", t, h, y1, BRICK_H1, B - 4, BRICK_H1, B - 2, true, true, nullptr);
    if (part == 1) return resblock_part(c, "conv_l1", t, h, y1, 0, BRICK_H1, 0, BRICK_H1, true, true, nullptr);
    return resblock_part(c, "conv_l1", t, h, y1, B + 2, BRICK_H1, B + 4, BRICK_H1, true, true, nullptr);
}

// After the encoder: the level-1 tensors, the brick's own planes of the level-1 input, and the part of conv_l1 that needs
// nothing from the neighbours -- it runs while the faces travel.
int brick_interior(nbe_ctx* c, nbe_ctx::StreamState& st) {
    const int m = c->mid;
    const Tensor& td = st.td;
    const Layer* L1 = find_layer(c, "conv_l1", "conv_1");
    if (!L1) return fail("missing layer conv_l1/conv_1");
    st.t = tallocp(c, m, td.p.D + 2 * BRICK_H1, td.p.H, td.p.W, 1);
    if (st.t.off < 0) return fail("workspace exhausted (level 1 input)");
    st.h = alloc_hidden(c, m, st.t.p.D - 2, st.t, block_fused(c, L1, st.t.p.D - 4));
    st.y1 = tallocp(c, m, st.t.p.D - 4, td.p.H, td.p.W, 1);
    if (st.h.off < 0 || st.y1.off < 0) return fail("workspace exhausted (level 1)");
    if (!c->dry) launch_wrap_pad(td.p, zview(st.t, BRICK_H1, td.p.D).p, 1, c->vel, c->stream, 0);
    return brick_conv_l1(c, st.t, st.h, st.y1, 0);
}

// With the neighbours' faces: the rest of conv_l1, the level-1 skip connection, down_l1 on the brick's own planes, and its
// boundary planes for the second exchange.
int brick_edges(nbe_ctx* c, nbe_ctx::StreamState& st) {
    const int m = c->mid;
    Tensor& td = st.td;
    const int B = td.p.D;
    brick_recv(c, td, c->bio.recv_lo, c->bio.recv_hi, BRICK_H1, st.t, 1);
    if (brick_conv_l1(c, st.t, st.h, st.y1, 1) || brick_conv_l1(c, st.t, st.h, st.y1, 2)) return 1;
    tfree(c, st.h); tfree(c, st.t); tfree(c, td);
    Tensor& y1 = st.y1;                                           // planes [-4, B + 4) of the brick's level-1 encoder output
    st.cat1 = tallocp(c, 2 * m, y1.p.D, y1.p.H - 2, y1.p.W - 2, 1);
    if (st.cat1.off < 0) return fail("workspace exhausted (cat1)");
    crop_into(c, y1, 0, st.cat1, 0);
    st.t2 = talloc(c, m, B / 2, (y1.p.H - 2) / 2, (y1.p.W - 2) / 2);
    const Layer* Ld1 = find_layer(c, "down_l1", "conv_0");
    if (st.t2.off < 0 || !Ld1) return fail("workspace exhausted or missing layer (down_l1)");
    if (down_conv(c, *Ld1, zview(y1, 4, B), st.t2, false)) return 1;
    tfree(c, y1);
    if (c->bio.send_lo) brick_send(c, st.t2, 0, BRICK_H2, c->bio.send_lo, c->bio.send_hi);
    return 0;
}

// The level-2 input: the brick's own down_l1 planes between the neighbours' (second exchange), extended periodically by 10
// voxels in y and x.
int brick_level2(nbe_ctx* c, nbe_ctx::StreamState& st, Tensor* t_out) {
    Tensor& t2 = st.t2;
    Tensor t = talloc(c, c->mid, t2.p.D + 2 * BRICK_H2, t2.p.H + 20, t2.p.W + 20);
    if (t.off < 0) return fail("workspace exhausted (level 2 input)");
    if (!c->dry) launch_wrap_pad(t2.p, zview(t, BRICK_H2, t2.p.D).p, 10, c->vel, c->stream, 0);
    brick_recv(c, t2, c->bio.recv_lo, c->bio.recv_hi, BRICK_H2, t, 10);
    tfree(c, t2);
    *t_out = t;
    return 0;
}

extern "C" {

// ---- the brick calls of the C ABI: the context below the full-resolution level is exchanged between them ------------
static constexpr int BRICK_RAW = 4;      // planes of RAW input a brick needs from either z neighbour (the level-0 encoder's reach for the brick's own planes)
static int brick_setup(nbe_ctx* c, const int64_t bsize[3], int* D, int* H, int* W, int64_t* need_out = nullptr) {
    c->sst.valid = false;
    if (require_ready(c)) return 1;
    if (!bsize) return fail("null argument");
    const int64_t b0 = bsize[0], S1 = bsize[1], S2 = bsize[2];
    if (b0 % 8 != 0 || b0 < 48) return fail("brick depth %lld unsupported: a multiple of 8, at least 48", (long long)b0);
    *D = (int)b0 + 96; *H = (int)S1 + 2; *W = (int)S2 + 2;
    if (check_dims_pyx(*D, *H, *W)) return 1;
    HIPCHK(hipSetDevice(c->device));
    c->pyx = true; c->pz = false; c->zx = true;
    // a brick of this size has been planned before and its workspace is still held (nbe_brick_plan allocates it): the same plan,
    // whatever the other tenants of the card have allocated since
    if (c->bp_slab > 0 && c->bp_size[0] == b0 && c->bp_size[1] == S1 && c->bp_size[2] == S2 && c->ws_bytes >= c->bp_need) {
        c->slab = c->bp_slab;
        if (need_out) *need_out = c->bp_need;
        return 0;
    }
    const int64_t budget = plan_budget(c, 0);
    int64_t need = 0;
    const int sl = choose_slab(c, *D, *H, *W, budget < 0 ? INT64_MAX / 4 : budget, &need, true, false);
    if (sl <= 0) { c->zx = false; return fail("brick of %lld x %lld x %lld does not fit the device memory that is free", (long long)b0, (long long)S1, (long long)S2); }
    c->slab = sl;
    c->bp_size[0] = b0; c->bp_size[1] = S1; c->bp_size[2] = S2; c->bp_slab = sl; c->bp_need = need;
    if (need_out) *need_out = need;
    return 0;
}

int64_t nbe_brick_halo_bytes(nbe_ctx* c, const int64_t bsize[3], int which) {
    if (!c || !bsize || which < 0 || which > 3) return -1;
    if (which == 3) return brick_halo_bytes(c, BRICK_H0, (int)bsize[1] + 2, (int)bsize[2] + 2);   // whole planes, wrap-around columns included
    if (which == 0) return (int64_t)c->in_chan * BRICK_RAW * bsize[1] * bsize[2] * 4;       // raw input planes, float32
    if (which == 1) return brick_halo_bytes(c, BRICK_H1, (int)bsize[1] / 2, (int)bsize[2] / 2) + 16;   // + the sender's range shift
    return brick_halo_bytes(c, BRICK_H2, (int)bsize[1] / 4, (int)bsize[2] / 4);
}

// > 0: the brick fits the device memory that is free now, with that many planes per z-slab; 0: it does not (no error)
int nbe_brick_plan(nbe_ctx* c, const int64_t bsize[3]) {
    if (!c || !bsize) return 0;
    int D, H, W;
    const int keep_slab = c->slab; const bool kp = c->pyx, kz = c->pz;   // the caller's plan survives a brick plan
    int rc = brick_setup(c, bsize, &D, &H, &W);
    // take the workspace now: what is free when the first brick is encoded may be less (other ranks of a shared card, the
    // caller's exchange buffers), and the ranks must not part ways after they have agreed on brick mode
    if (!rc) { rc = ensure_workspace(c, D, H, W); if (rc) { c->bp_slab = 0; (void)hipGetLastError(); } }
    const int sl = rc ? 0 : c->slab;
    c->zx = false; c->slab = keep_slab; c->pyx = kp; c->pz = kz;
    (void)nbe_last_error();
    return sl;
}

struct BrickOff { nbe_ctx* c; ~BrickOff() { c->phase = 0; c->zx = false; c->bio.skip_ready = nullptr; c->bio.skip_recv_lo = nullptr; } };

int nbe_brick_encode(nbe_ctx* c, const void* box, const int64_t bsize[3], float Dz, float vel_fac, void* send_lo, void* send_hi,
                     void* skip_send_lo, void* skip_send_hi) {
    if (!c || !box || !send_lo || !send_hi || !skip_send_lo || !skip_send_hi) return fail("null argument");
    if (!is_device_ptr(box) || !is_device_ptr(send_lo) || !is_device_ptr(send_hi) || !is_device_ptr(skip_send_lo) || !is_device_ptr(skip_send_hi))
        return fail("nbe_brick_encode takes device pointers");
    int D, H, W;
    if (brick_setup(c, bsize, &D, &H, &W)) return 1;
    BrickOff off{c};
    if (ensure_workspace(c, D, H, W)) return 1;
    const int Dh = (int)bsize[0] + 2 * BRICK_RAW;
    if (prepare_range(c, (const float*)box, (int64_t)c->in_chan * Dh * bsize[1] * bsize[2], Dz)) return 1;
    c->arena.reset();
    Tensor tin = talloc(c, c->in_chan, D, H, W);
    tin.pad = 1; set_org(tin, 0, 48, 48);
    // the haloed brick is (C, b0 + 8, S1, S2): planes [44, b0 + 52) of the tile's frame -- all the level-0 encoder reads for the
    // brick's own planes of the skip connection (the head reads the brick's own input planes); y and x periodic (origin -1)
    launch_gather((const float*)box, c->in_chan, Dh, (int)bsize[1], (int)bsize[2], 0, -1, -1, zview(tin, 48 - BRICK_RAW, Dh).p,
                  Dz / 6.0f * c->act_scale, c->prec, c->stream);
    c->phase = 1; c->bio.send_lo = send_lo; c->bio.send_hi = send_hi; c->bio.skip_send_lo = skip_send_lo; c->bio.skip_send_hi = skip_send_hi;
    c->sst.D = D; c->sst.H = H; c->sst.W = W;
    c->sst.Dz = Dz; c->sst.vel_fac = vel_fac; c->sst.act_scale = c->act_scale; c->sst.ws = c->ws;
    const HeadOut ho{nullptr, nullptr, NBE_F32, (int)bsize[0], (int)bsize[1], (int)bsize[2], 0, 0, 0, Dz, vel_fac};
    if (network_stream(c, tin, ho, c->slab)) return 1;
    // the last word of either face carries this rank's range shift: the receiver refuses faces computed with another one
    const int64_t body = brick_halo_bytes(c, BRICK_H1, (int)bsize[1] / 2, (int)bsize[2] / 2);
    unsigned bits; memcpy(&bits, &c->act_scale, 4);
    launch_tag_word((unsigned*)((char*)send_lo + body), bits, nullptr, nullptr, 0, c->stream);
    launch_tag_word((unsigned*)((char*)send_hi + body), bits, nullptr, nullptr, 0, c->stream);
    HIPCHK(hipGetLastError());
    return 0;
}

static int brick_resume(nbe_ctx* c, int phase) {
    if (!c->sst.valid) return fail("brick call without a preceding nbe_brick_encode (or another call has used this context's workspace in between)");
    if (c->sst.ws != c->ws) return fail("the workspace was reallocated since nbe_brick_encode");
    HIPCHK(hipSetDevice(c->device));
    c->pyx = true; c->pz = false; c->zx = true; c->phase = phase;
    return 0;
}

int nbe_brick_interior(nbe_ctx* c) {
    if (!c) return fail("null context");
    if (brick_resume(c, 2)) return 1;
    BrickOff off{c};
    const HeadOut ho{};
    if (network_stream(c, c->sst.tin, ho, c->sst.S)) return 1;
    HIPCHK(hipGetLastError());
    return 0;
}

int nbe_brick_exchange(nbe_ctx* c, const void* recv_lo, const void* recv_hi, void* send2_lo, void* send2_hi) {
    if (!c || !recv_lo || !recv_hi || !send2_lo || !send2_hi) return fail("null argument");
    if (brick_resume(c, 3)) return 1;
    BrickOff off{c};
    c->bio.recv_lo = recv_lo; c->bio.recv_hi = recv_hi; c->bio.send_lo = send2_lo; c->bio.send_hi = send2_hi;
    if (c->flags) {                                               // (strict float32 contexts have no range shift: nothing to compare)
        const int64_t body = brick_halo_bytes(c, BRICK_H1, (c->sst.H - 2) / 2, (c->sst.W - 2) / 2);
        unsigned bits; memcpy(&bits, &c->sst.act_scale, 4);
        launch_tag_word(nullptr, bits, (const unsigned*)((const char*)recv_lo + body), c->flags + 1, 2u, c->stream);
        launch_tag_word(nullptr, bits, (const unsigned*)((const char*)recv_hi + body), c->flags + 1, 2u, c->stream);
    }
    const HeadOut ho{};
    if (network_stream(c, c->sst.tin, ho, c->sst.S)) return 1;
    HIPCHK(hipGetLastError());
    return 0;
}

int nbe_brick_finish(nbe_ctx* c, const void* recv_lo, const void* recv_hi, const void* skip_recv_lo, const void* skip_recv_hi,
                     void* skip_ready_event, float Dz, float vel_fac, void* disp, void* vel, int out_dtype) {
    if (!c || !recv_lo || !recv_hi || !skip_recv_lo || !skip_recv_hi || !disp) return fail("null argument");
    if (c->vel && !vel) return fail("velocity output pointer is NULL but compute_vel is set");
    if (out_dtype != NBE_F32 && out_dtype != NBE_F16) return fail("out_dtype must be NBE_F32 or NBE_F16");
    if (brick_resume(c, 4)) return 1;
    BrickOff off{c};
    if (c->sst.Dz != Dz || c->sst.vel_fac != vel_fac || c->sst.act_scale != c->act_scale)
        return fail("nbe_brick_finish: Dz, vel_fac and the range shift must be those of the nbe_brick_encode call it completes");
    c->bio.recv_lo = recv_lo; c->bio.recv_hi = recv_hi; c->bio.skip_recv_lo = skip_recv_lo; c->bio.skip_recv_hi = skip_recv_hi;
    c->bio.skip_ready = (hipEvent_t)skip_ready_event;
    const int b0 = c->sst.D - 96, S1 = c->sst.H - 2, S2 = c->sst.W - 2;
    const HeadOut ho{disp, vel, out_dtype, b0, S1, S2, 0, 0, 0, Dz, vel_fac};
    if (network_stream(c, c->sst.tin, ho, c->sst.S)) return 1;
    HIPCHK(hipGetLastError());
    return 0;
}

}  // extern "C"
