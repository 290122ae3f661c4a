// Engine behind the C ABI (include/nbe.h).  Host code only; every device operation is a launch from nbe_kernels.hip.
// This unit is the place to start reading: the error state, the context (create, destroy, setters), the cosmology scalars,
// modulation (nbe_set_cosmology), the range shift of the f16-based arithmetic, and nbe_forward.  The rest, by unit:
//   nbe_engine_internal.h   the context struct and its parts (Arena, Layer, Tensor, Progress), prototypes that cross units
//   nbe_engine_net.cpp      tensors in the arena, run_conv, the blocks, the U-Net schedule on whole tensors and in z-slabs
//                           (style_nbody_emulator_vel_core.py:105-195)
//   nbe_engine_weights.cpp  what a layer needs on the device: packings, load_weights, gauge wiring, Winograd-z weights
//   nbe_engine_box.cpp      workspace sizing, a tile and its hipGraph, the tile planner, the sub-box loop
//                           (subbox.py:139-219), the host pipe and the pinned-host pool
//   nbe_engine_brick.cpp    the brick protocol of the sharded box
//   nbe_engine_probe.cpp    branch probe and profiler
//   nbe_engine_test.cpp     the hooks the tests reach single layers and blocks through
#include "nbe_engine_internal.h"

static thread_local std::string g_err;

int fail(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return 1;
}

// error message of the context-free entry points in other translation units (nbe_density.hip)
namespace nbe { int api_fail(const char* msg) { g_err = msg; return 1; } }

bool is_device_ptr(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeDevice;
}

int require_ready(nbe_ctx* c) {
    if (!c->have_weights) return fail("No parameters loaded. Call nbe_load_style_weights / nbe_load_premod_weights first.");
    if (c->style && !c->modulated) return fail("style weights are loaded but nbe_set_cosmology(Om, Dz) has not been called");
    return 0;
}

// ------------------------------------------------------------------------------------------------
// cosmology scalars (cosmology.py:24-40, :101-141), double precision, own 2F1 series
// ------------------------------------------------------------------------------------------------
static double hyp2f1_series(double a, double b, double c, double z) {
    double term = 1.0, sum = 1.0;
    for (int n = 0; n < 200000; ++n) {
        term *= (a + n) * (b + n) / ((c + n) * (n + 1.0)) * z;
        sum += term;
        if (std::fabs(term) < 1e-17 * std::fabs(sum)) break;
    }
    return sum;
}
static double hyp2f1(double a, double b, double c, double x) {
    if (x < 0) return std::pow(1.0 - x, -a) * hyp2f1_series(a, c - b, c, x / (x - 1.0));   // Pfaff
    return hyp2f1_series(a, b, c, x);
}
static const double A2 = 1.0, B2 = 1.0 / 3.0, C2 = 11.0 / 6.0;

extern "C" double nbe_growth_factor(double z, double Om) {
    const double a = 1.0 / (1.0 + z), OL = 1.0 - Om;
    return a * hyp2f1(A2, B2, C2, -OL * a * a * a / Om) / hyp2f1(A2, B2, C2, -OL / Om);
}
static double growth_rate(double z, double Om) {
    const double a = 1.0 / (1.0 + z), x = -(1.0 - Om) * a * a * a / Om;
    const double F = hyp2f1(A2, B2, C2, x);
    const double dF = (A2 * B2 / C2) * hyp2f1(A2 + 1, B2 + 1, C2 + 1, x);
    return 1.0 + 3.0 * x * dF / F;
}
extern "C" double nbe_vel_norm(double z, double Om) {
    const double H = 100.0 * std::sqrt(Om * std::pow(1.0 + z, 3) + (1.0 - Om));
    return nbe_growth_factor(z, Om) * growth_rate(z, Om) * H / (1.0 + z);
}

// ------------------------------------------------------------------------------------------------
// Range shift (include/nbe.h, "Range").  LeakyReLU is positively homogeneous and the convolutions are linear, so the
// network with input x and biases b satisfies f(s x; s b) = s f(x; b) for s > 0, exactly in floating point when s is a
// power of two.  The f16-based modes use that to keep their operands where f16 has both range and precision: s = 2^k
// brings max(|x| Dz / 6, max |b|) into [0.5, 1) (float16) or [2^5, 2^6) (f16x3: H3_RANGE_UP) whatever the caller's units are.
// ------------------------------------------------------------------------------------------------
int prepare_range(nbe_ctx* c, const float* dev_src, int64_t n, float Dz, const float* host_src) {
    c->input_finite = true;
    float s = 1.f;
    if (prec_is_half(c->prec)) {
        if (!c->flags) { HIPCHK(hipMalloc((void**)&c->flags, 8)); HIPCHK(hipMemsetAsync(c->flags, 0, 8, c->stream)); }
        float amax = c->preset_absmax;
        if (amax < 0.f && host_src) {                           // pipelined host path: the box is not on the device yet
            const unsigned bits = host_absmax_bits(host_src, n);
            memcpy(&amax, &bits, 4);
        } else if (amax < 0.f) {
            HIPCHK(hipMemsetAsync(c->flags, 0, 4, c->stream));
            launch_absmax(dev_src, n, c->flags, c->stream);
            unsigned bits = 0;
            HIPCHK(hipMemcpyAsync(&bits, c->flags, 4, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            memcpy(&amax, &bits, 4);
        }
        if (!std::isfinite(amax)) c->input_finite = false;     // NaN / infinity in: NaN / infinity out, as in the reference
        else {
            const float m = std::max(amax * std::fabs(Dz) / 6.0f, c->bias_max);
            if (m > 0.f && std::isfinite(m)) {
                int e = 0;
                (void)std::frexp(m, &e);                        // m = f * 2^e, f in [0.5, 1)
                e = std::max(-100, std::min(100, e));
                s = std::ldexp(1.0f, -e + (c->prec == PREC_F16X3 ? H3_RANGE_UP : 0));
            }
        }
    }
    c->act_scale = s;
    if (s != c->bias_scale || c->bias_dirty) {
        for (auto& kv : c->layers) {
            Layer& L = kv.second;
            const int nb = L.pw.ctiles * 32 * L.pw.ni;
            launch_scale(L.bias0, L.pw.bias, nb, s, c->stream);
            if (L.fskip) launch_scale(L.bias0, L.bias_f, nb, s, c->stream, L.fskip->bias0);   // fused block: b_1 + b_s
        }
        c->bias_scale = s; c->bias_dirty = false;
    }
    c->range_pending = true;
    return 0;
}

// after a call: did the head write a non-finite value although the input was finite?  (synchronises the stream)
int check_range(nbe_ctx* c) {
    if (!c->range_pending || !c->flags) { c->range_pending = false; return 0; }
    c->range_pending = false;
    unsigned bad = 0;
    HIPCHK(hipMemcpyAsync(&bad, c->flags + 1, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemsetAsync(c->flags + 1, 0, 4, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (bad & 2u)
        return fail("brick mode: a neighbour's faces were computed with another range shift -- every rank must call "
                    "nbe_set_input_range with the box-wide max |x| before nbe_brick_encode");
    if (bad && c->input_finite) {
        fail("non-finite values in the output of a finite input: an activation left the range of the %s arithmetic "
             "(|value| >= 65504 * 2^%d after the range shift); rerun this call with NBE_PREC_F32",
             c->prec == PREC_F16 ? "float16" : "f16x3", -(int)std::lround(std::log2(c->act_scale)));
        return 2;
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------------
extern "C" {

const char* nbe_last_error(void) { return g_err.c_str(); }
int nbe_version(void) { return 100; }

int nbe_create(int device_id, nbe_ctx** out) {
    if (!out) return fail("nbe_create: out is NULL");
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0)
        return fail("nbe_create: no HIP device is visible; this library has no CPU fallback");
    if (device_id < 0 || device_id >= ndev) return fail("nbe_create: device %d out of range (0..%d)", device_id, ndev - 1);
    HIPCHK(hipSetDevice(device_id));
    hipDeviceProp_t prop;
    HIPCHK(hipGetDeviceProperties(&prop, device_id));
    if (!strstr(prop.gcnArchName, "gfx950"))
        return fail("nbe_create: device %d is %s; the kernels are built for gfx950 (MI355X) only", device_id, prop.gcnArchName);
    nbe_ctx* c = new nbe_ctx();
    c->device = device_id;
    HIPCHK(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    if (const char* e = getenv("NBE_MAX_TILE")) c->max_tile = atoi(e) > 0 ? atoi(e) : 0;
    if (const char* e = getenv("NBE_SLAB")) c->slab_forced = atoi(e) >= 0 ? (atoi(e) & ~1) : -1;
    if (const char* e = getenv("NBE_PERIODIC")) c->pyx_allowed = atoi(e) != 0;
    *out = c;
    return 0;
}

int nbe_destroy(nbe_ctx* c) {
    if (!c) return 0;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream);
    prof_collect(c);
    free_layers(c);
    (void)hipFree(c->probe.bits); (void)hipFree(c->probe.count);
    (void)hipFree(c->ws); (void)hipFree(c->box_in); (void)hipFree(c->box_out); (void)hipFree(c->gauge_flag); (void)hipFree(c->wino_flag); (void)hipFree(c->flags);
    drop_graphs(c);
    if (c->ev_g0) (void)hipEventDestroy(c->ev_g0);
    if (c->ev_g1) (void)hipEventDestroy(c->ev_g1);
    for (auto e : c->ev_pool) (void)hipEventDestroy(e);
    for (int i = 0; i < nbe_ctx::NSTAGE; ++i) { if (c->stage_buf[i]) (void)hipHostFree(c->stage_buf[i]); if (c->stage_free[i]) (void)hipEventDestroy(c->stage_free[i]); }
    if (c->ev_up) (void)hipEventDestroy(c->ev_up);
    if (c->ev_down) (void)hipEventDestroy(c->ev_down);
    if (c->up_stream) (void)hipStreamDestroy(c->up_stream);
    if (c->down_stream) (void)hipStreamDestroy(c->down_stream);
    (void)hipStreamDestroy(c->own_stream);
    delete c;
    return 0;
}

int nbe_set_stream(nbe_ctx* c, void* s) {
    if (!c) return fail("null context");
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = (hipStream_t)s;      // NULL is the device's default (null) stream, as everywhere in HIP
    return 0;
}

int nbe_use_own_stream(nbe_ctx* c) {
    if (!c) return fail("null context");
    HIPCHK(hipStreamSynchronize(c->stream));
    c->stream = c->own_stream;
    return 0;
}

int nbe_synchronize(nbe_ctx* c) {
    if (!c) return fail("null context");
    HIPCHK(hipStreamSynchronize(c->stream));
    return 0;
}

int nbe_set_arch(nbe_ctx* c, int in_chan, int out_chan, int mid_chan, float eps, int compute_vel) {
    if (!c) return fail("null context");
    if (in_chan < 1 || in_chan > 16) return fail("in_chan=%d unsupported (1..16)", in_chan);
    if (out_chan < 1 || out_chan > 64) return fail("out_chan=%d unsupported (1..64)", out_chan);
    if (out_chan != in_chan) return fail("out_chan (%d) must equal in_chan (%d): the head adds the cropped input (core :187)", out_chan, in_chan);
    if (mid_chan < 8 || mid_chan % 8 != 0) return fail("mid_chan=%d unsupported (multiple of 8 required)", mid_chan);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    free_layers(c);
    c->in_chan = in_chan; c->out_chan = out_chan; c->mid = mid_chan; c->eps = eps; c->vel = compute_vel != 0;
    return 0;
}

int nbe_set_cosmology(nbe_ctx* c, float Om, float Dz) {
    if (!c) return fail("null context");
    if (!c->have_weights) return fail("No parameters loaded. Call nbe_load_style_weights first.");
    if (!c->style) return 0;
    if (c->modulated && c->mod_Om == Om && c->mod_Dz == Dz) return 0;
    c->sst.valid = false;                                        // a pending brick was encoded with the previous modulation
    HIPCHK(hipSetDevice(c->device));
    // s = ((Om - 0.3) * 5, Dz - 1) in float32 (core :126-128)
    const float s0 = (Om - 0.3f) * 5.0f, s1 = Dz - 1.0f;
    bool use_gauge = c->gauge;
    if (use_gauge) {
        // alpha of every layer first (the tangent weights of the general layers need their neighbours'); a style
        // factor that is zero at this cosmology has no alpha: fall back to the three-product kernels for this call
        HIPCHK(hipMemsetAsync(c->gauge_flag, 0, 4, c->stream));
        for (auto& kv : c->layers)
            launch_style_alpha(kv.second.sw, kv.second.sb, kv.second.cin, s0, s1, kv.second.alpha, c->gauge_flag, c->stream);
        int bad = 0;
        HIPCHK(hipMemcpyAsync(&bad, c->gauge_flag, 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        use_gauge = bad == 0;
    }
    for (auto& kv : c->layers) {
        Layer& L = kv.second;
        // (map order: a block's conv_1, which writes its beta, comes before its skip, which folds it in as b_sub)
        launch_modulate(L.weight, L.sw, L.sb, L.cout, L.cin, L.k * L.k * L.k, s0, s1, c->eps, L.first ? 1 : 0,
                        L.wn, c->vel ? L.dwn : nullptr, c->stream, use_gauge ? L.a_in : nullptr, use_gauge ? L.beta : nullptr,
                        (use_gauge && c->prec != PREC_F16) ? L.b_sub : nullptr);
        if (use_gauge && c->prec == PREC_F16 && c->vel && L.b_sub && L.dwn_f)     // float16 model: the fused stages' version beside it
            launch_modulate(L.weight, L.sw, L.sb, L.cout, L.cin, L.k * L.k * L.k, s0, s1, c->eps, L.first ? 1 : 0,
                            L.wn, L.dwn_f, c->stream, L.a_in, nullptr, L.b_sub);
        launch_pack(L.wn, L.cout, L.cin, L.kind, L.pw, L.pw.w, c->stream);
        if (L.pwn.w) launch_pack(L.wn, L.cout, L.cin, L.kind, L.pwn, L.pwn.w, c->stream);
        if (L.pwn.dw) launch_pack(L.dwn, L.cout, L.cin, L.kind, L.pwn, L.pwn.dw, c->stream);
        if (c->vel && !(use_gauge && L.g6)) launch_pack(L.dwn, L.cout, L.cin, L.kind, L.pw, L.pw.dw, c->stream);
    }
    c->gauge_active = use_gauge;
    c->fuse = use_gauge && prec_is_half(c->prec);               // blocks with Layer::fskip run their skip inside conv_1
    if (pack_wino(c)) return 1;
    HIPCHK(hipGetLastError());
    c->modulated = true; c->mod_Om = Om; c->mod_Dz = Dz;
    ++c->epoch;                                                  // captured graphs hold the schedule of the previous modulation
    return 0;
}

int nbe_forward(nbe_ctx* c, const void* x, int D, int H, int W, float Dz, float vel_fac, void* disp, void* vel) {
    if (!c || !x || !disp) return fail("null argument");
    if (require_ready(c)) return 1;
    if (c->vel && !vel) return fail("velocity output pointer is NULL but compute_vel is set");
    if (check_dims(D, H, W)) return 1;
    HIPCHK(hipSetDevice(c->device));
    const int OD = D - 96, OH = H - 96, OW = W - 96;
    const int64_t in_bytes = (int64_t)c->in_chan * D * H * W * 4, out_bytes = (int64_t)c->out_chan * OD * OH * OW * 4;
    const bool xin_dev = is_device_ptr(x), out_dev = is_device_ptr(disp);
    c->slab = 0; c->pyx = false; c->pz = false;               // single inputs run on whole tensors, no periodicity
    if (ensure_workspace(c, D, H, W)) return 1;
    const float* xd = (const float*)x;
    if (!xin_dev) {
        if (in_bytes > c->box_in_bytes) { (void)hipFree(c->box_in); HIPCHK(hipMalloc((void**)&c->box_in, in_bytes)); c->box_in_bytes = in_bytes; }
        HIPCHK(hipMemcpyAsync(c->box_in, x, in_bytes, hipMemcpyHostToDevice, c->stream));
        xd = c->box_in;
    }
    char *dd = (char*)disp, *vd = (char*)vel;
    if (!out_dev) {
        const int64_t need = out_bytes * 2;
        if (need > c->box_out_bytes) { (void)hipFree(c->box_out); HIPCHK(hipMalloc((void**)&c->box_out, need)); c->box_out_bytes = need; }
        dd = c->box_out; vd = c->box_out + out_bytes;
    }
    if (prepare_range(c, xd, (int64_t)c->in_chan * D * H * W, Dz)) return 1;
    if (c->probe.on) {
        const int oe[3] = {OD, OH, OW};
        c->probe.tile = true;
        for (int d = 0; d < 3; ++d) {
            c->probe.o[d] = c->probe.p[d];
            if (c->probe.p[d] < 0 || c->probe.p[d] + c->probe.nout > oe[d]) return fail("branch probe: the block does not fit the output of this input");
        }
    }
    if (run_subbox(c, xd, D, H, W, 0, 0, 0, D, H, W, Dz, vel_fac, dd, vd, NBE_F32, OD, OH, OW, 0, 0, 0)) return 1;
    HIPCHK(hipGetLastError());
    if (!out_dev) {
        HIPCHK(hipMemcpyAsync(disp, dd, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if (c->vel) HIPCHK(hipMemcpyAsync(vel, vd, out_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (!out_dev || !xin_dev) {
        HIPCHK(hipStreamSynchronize(c->stream));
        return check_range(c);                                  // host arrays: the call is synchronous anyway
    }
    return 0;
}

int nbe_set_precision(nbe_ctx* c, int prec) {
    if (!c) return fail("null context");
    if (prec != PREC_F32 && prec != PREC_F16X3 && prec != PREC_F16) return fail("precision must be NBE_PREC_F32 (0), NBE_PREC_F16X3 (1) or NBE_PREC_F16 (2)");
    if (c->have_weights && prec != c->prec)
        return fail("nbe_set_precision must be called before the weights are loaded (they are packed per precision)");
    if (prec != c->prec) c->bp_slab = 0;                        // planes_for(mid, prec): another workspace layout, another brick plan
    c->prec = prec;
    return 0;
}

int nbe_set_periodic(nbe_ctx* c, int on) {
    if (!c) return fail("null context");
    c->pyx_allowed = on != 0;
    return 0;
}

int nbe_set_slab(nbe_ctx* c, int slab) {
    if (!c) return fail("null context");
    if (slab > 0 && (slab & 1)) return fail("slab must be even");
    c->slab_forced = slab < 0 ? -1 : slab;
    c->bp_slab = 0;                                             // a cached brick plan was made under the previous setting
    return 0;
}

int nbe_set_max_tile(nbe_ctx* c, int max_tile) {
    if (!c) return fail("null context");
    if (max_tile < 0) return fail("max_tile must be >= 0 (0 = keep the caller's sub-box grid)");
    c->max_tile = max_tile;
    return 0;
}

int nbe_check_finite(nbe_ctx* c) {
    if (!c) return fail("null context");
    HIPCHK(hipSetDevice(c->device));
    return check_range(c);
}

int nbe_set_input_range(nbe_ctx* c, float absmax) {
    if (!c) return fail("null context");
    c->preset_absmax = (absmax >= 0.f || std::isnan(absmax)) ? absmax : -1.f;
    return 0;
}

int nbe_query(nbe_ctx* c, int what, double* out) {
    if (!c || !out) return fail("null argument");
    switch (what) {
    case NBE_Q_GAUGE_ACTIVE: *out = c->gauge_active ? 1 : 0; break;
    case NBE_Q_SLAB: *out = c->slab; break;
    case NBE_Q_PERIODIC_YX: *out = c->pyx ? 1 : 0; break;
    case NBE_Q_PERIODIC_Z: *out = c->pz ? 1 : 0; break;
    case NBE_Q_RANGE_SHIFT: *out = std::log2((double)c->act_scale); break;
    case NBE_Q_WORKSPACE_BYTES: *out = (double)c->ws_bytes; break;
    case NBE_Q_HOST_PIPE: *out = c->last_piped ? 1 : 0; break;
    case NBE_Q_GRAPH_REPLAYS: *out = (double)c->graph_replays; break;
    case NBE_Q_PLAN_TILES: *out = (double)c->plan_tiles; break;
    case NBE_Q_PLAN_SHORT_GB: *out = c->plan_short_gb; break;
    default: return fail("nbe_query: unknown item %d", what);
    }
    return 0;
}

int64_t nbe_workspace_bytes(nbe_ctx* c) { return c ? c->ws_bytes : 0; }

}  // extern "C"
