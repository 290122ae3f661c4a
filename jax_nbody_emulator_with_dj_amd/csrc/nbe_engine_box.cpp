// Boxes: workspace sizing, one tile and its hipGraph replay, the tile planner, the sub-box loop (subbox.py:139-219) with
// the pipelined host path, and the pinned-host pool.
#include "nbe_engine_internal.h"

#include <sched.h>

// ---- host-side helpers of the pipelined host path -------------------------------------------------------------
static int host_threads() {
    static const int n = [] {
        if (const char* e = getenv("NBE_HOST_THREADS")) return std::max(1, atoi(e));
        unsigned hw = std::thread::hardware_concurrency();
        cpu_set_t set;                                          // the cores this process may actually use
        if (sched_getaffinity(0, sizeof set, &set) == 0) hw = std::min<unsigned>(hw ? hw : 64, (unsigned)CPU_COUNT(&set));
        return (int)std::max(1u, std::min(hw ? hw : 4u, 16u));
    }();
    return n;
}
template <typename F>
static void parallel_for(int nt, F&& fn) {                      // fn(i, nt) on nt threads (the caller runs share 0)
    std::vector<std::thread> th;
    for (int i = 1; i < nt; ++i) th.emplace_back([&fn, i, nt] { fn(i, nt); });
    fn(0, nt);
    for (auto& t : th) t.join();
}
static void parallel_memcpy(void* dst, const void* src, size_t bytes) {
    const int nt = bytes < (size_t(8) << 20) ? 1 : host_threads();
    parallel_for(nt, [&](int i, int n) {
        const size_t per = ((bytes + n - 1) / n + 4095) & ~size_t(4095), b = std::min(bytes, per * i), e = std::min(bytes, b + per);
        if (e > b) memcpy((char*)dst + b, (const char*)src + b, e - b);
    });
}
// bit pattern of max |x| over a host array (the host-side twin of launch_absmax)
unsigned host_absmax_bits(const float* x, int64_t n) {
    const int nt = n < (1 << 22) ? 1 : host_threads();
    std::vector<unsigned> part(nt, 0u);
    parallel_for(nt, [&](int i, int k) {
        const int64_t per = (n + k - 1) / k, b = std::min(n, per * i), e = std::min(n, b + per);
        const unsigned* u = (const unsigned*)x;
        unsigned m0 = 0, m1 = 0, m2 = 0, m3 = 0;
        int64_t j = b;
        for (; j + 4 <= e; j += 4) {
            m0 = std::max(m0, u[j] & 0x7fffffffu); m1 = std::max(m1, u[j + 1] & 0x7fffffffu);
            m2 = std::max(m2, u[j + 2] & 0x7fffffffu); m3 = std::max(m3, u[j + 3] & 0x7fffffffu);
        }
        for (; j < e; ++j) m0 = std::max(m0, u[j] & 0x7fffffffu);
        part[i] = std::max(std::max(m0, m1), std::max(m2, m3));
    });
    unsigned m = 0;
    for (unsigned v : part) m = std::max(m, v);
    return m;
}
static bool is_pinned_host_ptr(const void* p) {
    hipPointerAttribute_t at;
    if (hipPointerGetAttributes(&at, p) != hipSuccess) { (void)hipGetLastError(); return false; }
    return at.type == hipMemoryTypeHost;
}

// ---- pinned host memory pool (nbe_host_alloc / nbe_host_free) ---------------------------------------------------
static std::mutex g_pin_mu;
static std::multimap<size_t, void*> g_pin_free;                 // size -> buffer, ready for reuse
static std::map<void*, size_t> g_pin_live;                      // handed out
static size_t g_pin_free_bytes = 0;
static size_t pin_pool_cap() {
    static const size_t cap = (size_t)((getenv("NBE_PINNED_POOL_GB") ? atof(getenv("NBE_PINNED_POOL_GB")) : 16.0) * (1ull << 30));
    return cap;
}

// ------------------------------------------------------------------------------------------------
// Pipelined host path (HostPipe).  The tile is the whole periodic box; tile plane t is box plane (o0 + t) mod S0.
// ------------------------------------------------------------------------------------------------
static constexpr int PIPE_CHUNK = 32;                            // box planes per staged upload

// box planes behind tile planes [t0, t1) -> device box (enqueued on up_stream; pageable sources go through the pinned
// staging ring, filled by host threads)
static int pipe_upload(nbe_ctx* c, int t0, int t1) {
    auto& P = c->pipe;
    const int64_t plane = (int64_t)P.S1 * P.S2;
    const int D = P.S0 + 96;                                      // (a tile is at most the box + its halo deep)
    t0 = std::max(t0, 0); t1 = std::min(t1, D);
    int t = t0;
    while (t < t1) {
        const int b = ((P.o0 + t) % P.S0 + P.S0) % P.S0;
        if (P.up[b]) { ++t; continue; }
        int run = 1;
        while (t + run < t1 && b + run < P.S0 && !P.up[b + run] && run < PIPE_CHUNK) ++run;
        const size_t bytes = (size_t)run * plane * 4;            // per channel
        float* dbox = c->box_in;
        if (P.in_pinned) {
            for (int ch = 0; ch < P.C; ++ch)
                HIPCHK(hipMemcpyAsync(dbox + ((int64_t)ch * P.S0 + b) * plane, P.hbox + ((int64_t)ch * P.S0 + b) * plane,
                                      bytes, hipMemcpyHostToDevice, c->up_stream));
        } else {
            const int slot = P.nstage % nbe_ctx::NSTAGE;
            if (P.nstage >= nbe_ctx::NSTAGE) HIPCHK(hipEventSynchronize(c->stage_free[slot]));   // its last DMA has finished
            for (int ch = 0; ch < P.C; ++ch)
                parallel_memcpy(c->stage_buf[slot] + ch * bytes, P.hbox + ((int64_t)ch * P.S0 + b) * plane, bytes);
            for (int ch = 0; ch < P.C; ++ch)
                HIPCHK(hipMemcpyAsync(dbox + ((int64_t)ch * P.S0 + b) * plane, c->stage_buf[slot] + ch * bytes, bytes,
                                      hipMemcpyHostToDevice, c->up_stream));
            HIPCHK(hipEventRecord(c->stage_free[slot], c->up_stream));
            ++P.nstage;
        }
        for (int k = 0; k < run; ++k) P.up[b + k] = 1;
        t += run;
    }
    return 0;
}

// tile planes [t0, t1) of the input tensor: upload what is missing, gather them (core :132-134 scaling), then start the
// upload of the `look` planes that follow so that it runs under the kernels enqueued next
int pipe_input(nbe_ctx* c, const Tensor& tin, int t0, int t1, int look, float scale) {
    auto& P = c->pipe;
    if (P.gz < t0) P.gz = t0;                                    // planes before t0 are never read
    if (t1 > P.gz) {
        if (pipe_upload(c, P.gz, t1)) return 1;
        HIPCHK(hipEventRecord(c->ev_up, c->up_stream));
        HIPCHK(hipStreamWaitEvent(c->stream, c->ev_up, 0));
        const Tensor v = zview(tin, P.gz, t1 - P.gz);
        const int h = tin.pad ? 1 : 48;
        launch_gather(c->box_in, P.C, P.S0, P.S1, P.S2, P.o0 + P.gz, P.slabwise ? P.o1 : -h, P.slabwise ? P.o2 : -h, v.p, scale,
                      c->prec, c->stream);
        P.gz = t1;
    }
    return look > 0 ? pipe_upload(c, t1, t1 + look) : 0;
}

// output planes [z, z + n) of every channel of both fields: device staging -> the caller's pinned arrays, on the
// down stream, behind the head launch that produced them
int pipe_output(nbe_ctx* c, int z, int n, int a1, int a2, int e1, int e2) {
    auto& P = c->pipe;
    if (e1 < 0) e1 = P.O1;
    if (e2 < 0) e2 = P.O2;
    HIPCHK(hipEventRecord(c->ev_down, c->stream));
    HIPCHK(hipStreamWaitEvent(c->down_stream, c->ev_down, 0));
    const int64_t plane = (int64_t)P.O1 * P.O2 * P.esz;
    const bool whole = a1 == 0 && a2 == 0 && e1 == P.O1 && e2 == P.O2;
    for (int f = 0; f < (P.hvel ? 2 : 1); ++f) {
        char* h = f ? P.hvel : P.hdisp;
        char* d = f ? P.dvel : P.ddisp;
        for (int ch = 0; ch < c->out_chan; ++ch) {
            if (whole) {
                const int64_t off = ((int64_t)ch * P.O0 + z) * plane;
                HIPCHK(hipMemcpyAsync(h + off, d + off, (size_t)n * plane, hipMemcpyDeviceToHost, c->down_stream));
            } else {                                             // a tile's (n, e1, e2) block of the (C, O0, O1, O2) arrays
                hipMemcpy3DParms mp;
                memset(&mp, 0, sizeof mp);
                mp.srcPtr = make_hipPitchedPtr(d, (size_t)P.O2 * P.esz, (size_t)P.O2 * P.esz, (size_t)P.O1);
                mp.dstPtr = make_hipPitchedPtr(h, (size_t)P.O2 * P.esz, (size_t)P.O2 * P.esz, (size_t)P.O1);
                mp.srcPos = make_hipPos((size_t)a2 * P.esz, (size_t)a1, (size_t)ch * P.O0 + z);
                mp.dstPos = mp.srcPos;
                mp.extent = make_hipExtent((size_t)e2 * P.esz, (size_t)e1, (size_t)n);
                mp.kind = hipMemcpyDeviceToHost;
                HIPCHK(hipMemcpy3DAsync(&mp, c->down_stream));
            }
        }
    }
    return 0;
}

// bytes of workspace a (D,H,W) input needs with the schedule (slab, pyx, pz): a dry run of the network through the arena
// (no launches) with that schedule in place of the current one, which it leaves as it was; < 0 on error
static int64_t workspace_need(nbe_ctx* c, int D, int H, int W, int slab, bool pyx, bool pz) {
    const int keep_slab = c->slab; const bool keep_pyx = c->pyx, keep_pz = c->pz;
    c->slab = slab; c->pyx = pyx; c->pz = pz;
    c->dry = true;
    c->arena.reset();
    Tensor tin = talloc(c, c->in_chan, D, H, W), y;
    tin.pad = c->pyx ? 1 : 0;
    HeadOut ho{};
    const int rc = c->slab > 0 ? network_stream(c, tin, ho, c->slab) : network(c, tin, &y);
    c->dry = false;
    c->slab = keep_slab; c->pyx = keep_pyx; c->pz = keep_pz;
    return rc ? -1 : c->arena.high;
}

// size the workspace for a (D,H,W) input with a dry run of the current schedule, then (re)allocate it
int ensure_workspace(nbe_ctx* c, int D, int H, int W) {
    const int64_t need = workspace_need(c, D, H, W, c->slab, c->pyx, c->pz);
    if (need < 0) return 1;
    if (need > c->ws_bytes) {
        c->sst.valid = false;
        if (c->ws) { HIPCHK(hipStreamSynchronize(c->stream)); HIPCHK(hipFree(c->ws)); c->ws = nullptr; c->ws_bytes = 0; }
        HIPCHK(hipMalloc((void**)&c->ws, need));
        // padded channel planes are read (against zero weights) but never written: they must hold finite values
        HIPCHK(hipMemsetAsync(c->ws, 0, need, c->stream));
        c->ws_bytes = need;
    }
    return 0;
}

// one sub-box: `box` is a device-resident (C, Db, Hb, Wb) volume, the crop origin may be negative (periodic)
int run_subbox(nbe_ctx* c, const float* box, int Db, int Hb, int Wb, int o0, int o1, int o2,
                      int D, int H, int W, float Dz, float vel_fac, void* disp, void* velo, int out_dtype,
                      int OD, int OH, int OW, int a0, int a1, int a2) {
    c->sst.valid = false;                                        // a tile reuses the arena: a pending brick's tensors are gone
    c->arena.reset();
    Tensor tin = talloc(c, c->in_chan, D, H, W), y;
    tin.pad = c->pyx ? 1 : 0;                                   // periodic-yx: (H, W) = box extent + 2, gathered from origin - 1
    if (tin.pad) set_org(tin, 0, 48, 48);                        // its interior sits 48 voxels into the padded frame
    // core :132-134: x = x * (Dz / 6); the pipelined host path gathers slab by slab as the box arrives (pipe_input)
    if (!c->pipe.active && !c->pipe.slabwise)
        launch_gather(box, c->in_chan, Db, Hb, Wb, o0, o1, o2, tin.p, Dz / 6.0f * c->act_scale, c->prec, c->stream);
    const HeadOut ho{disp, velo, out_dtype, OD, OH, OW, a0, a1, a2, Dz, vel_fac};
    if (c->slab > 0) return network_stream(c, tin, ho, c->slab);
    if (network(c, tin, &y)) return 1;
    run_head(c, y, tin, ho, 0);
    return 0;
}

void drop_graphs(nbe_ctx* c) {
    for (auto& kv : c->graphs) {
        if (kv.second.exec) (void)hipGraphExecDestroy(kv.second.exec);
        if (kv.second.graph) (void)hipGraphDestroy(kv.second.graph);
    }
    c->graphs.clear();
}

// One tile through run_subbox, replayed from a captured hipGraph when the identical tile (same pointers, geometry,
// scalars, weights epoch) has been run before.  The first request runs eagerly on the caller's stream (one-time
// hipFuncSetAttribute calls, lazily created state); the second is captured on the context's own stream -- the caller's
// may be the legacy null stream, which cannot be captured -- and every later one is a single hipGraphLaunch, fenced
// against the caller's stream by two events.  Not used with profiling, progress callbacks or the pipelined host path
// (they synchronise or use other streams inside the schedule).  NBE_GRAPH=0 turns it off.
static int run_tile(nbe_ctx* c, const float* box, int Db, int Hb, int Wb, int o0, int o1, int o2,
                    int D, int H, int W, float Dz, float vel_fac, void* disp, void* velo, int out_dtype,
                    int OD, int OH, int OW, int a0, int a1, int a2) {
    const bool off = getenv("NBE_GRAPH") && atoi(getenv("NBE_GRAPH")) == 0;
    if (off || c->prof || c->prog_cb || c->pipe.active || c->pipe.slabwise || c->dry || c->probe.on)
        return run_subbox(c, box, Db, Hb, Wb, o0, o1, o2, D, H, W, Dz, vel_fac, disp, velo, out_dtype, OD, OH, OW, a0, a1, a2);
    nbe_ctx::GraphKey k;
    memset(&k, 0, sizeof k);
    k.box = box; k.disp = disp; k.velo = velo; k.ws = c->ws;
    const int geo[18] = {Db, Hb, Wb, o0, o1, o2, D, H, W, out_dtype, OD, OH, OW, a0, a1, a2, c->slab, c->prec};
    memcpy(k.geo, geo, sizeof geo);
    k.f[0] = Dz; k.f[1] = vel_fac; k.f[2] = c->act_scale;
    // (the A/B switch that launchers read per launch is part of the key: a captured graph holds the kernels it chose)
    k.epoch = c->epoch; k.flags = (c->pyx ? 1 : 0) | (c->pz ? 2 : 0) | (c->gauge_active ? 4 : 0) | (c->fuse ? 8 : 0) | (wino_env_off() ? 16 : 0);
    nbe_ctx::GraphVal& g = c->graphs[k];
    g.used = ++c->graph_clock;
    if (!g.exec && g.seen++ == 0) {                              // first time: eager
        if (c->graphs.size() > 16) {                             // keep the cache small: drop the least recently used
            auto lru = c->graphs.begin();
            for (auto it = c->graphs.begin(); it != c->graphs.end(); ++it) if (it->second.used < lru->second.used) lru = it;
            if (lru->second.exec) (void)hipGraphExecDestroy(lru->second.exec);
            if (lru->second.graph) (void)hipGraphDestroy(lru->second.graph);
            c->graphs.erase(lru);
        }
        return run_subbox(c, box, Db, Hb, Wb, o0, o1, o2, D, H, W, Dz, vel_fac, disp, velo, out_dtype, OD, OH, OW, a0, a1, a2);
    }
    if (!c->ev_g0) { HIPCHK(hipEventCreateWithFlags(&c->ev_g0, hipEventDisableTiming)); HIPCHK(hipEventCreateWithFlags(&c->ev_g1, hipEventDisableTiming)); }
    hipStream_t user = c->stream;
    if (!g.exec) {                                               // second time: capture on the own stream
        c->stream = c->own_stream;
        hipError_t e = hipStreamBeginCapture(c->own_stream, hipStreamCaptureModeThreadLocal);
        int rc = 0;
        if (e == hipSuccess) {
            rc = run_subbox(c, box, Db, Hb, Wb, o0, o1, o2, D, H, W, Dz, vel_fac, disp, velo, out_dtype, OD, OH, OW, a0, a1, a2);
            e = hipStreamEndCapture(c->own_stream, &g.graph);
            if (e == hipSuccess && !rc) e = hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0);
        }
        c->stream = user;
        if (rc || e != hipSuccess || !g.exec) {                  // capture is an optimisation: fall back to eager for good
            (void)hipGetLastError();
            if (g.graph) { (void)hipGraphDestroy(g.graph); g.graph = nullptr; }
            g.exec = nullptr; g.seen = -1000000;
            return run_subbox(c, box, Db, Hb, Wb, o0, o1, o2, D, H, W, Dz, vel_fac, disp, velo, out_dtype, OD, OH, OW, a0, a1, a2);
        }
    }
    if (user != c->own_stream) { HIPCHK(hipEventRecord(c->ev_g0, user)); HIPCHK(hipStreamWaitEvent(c->own_stream, c->ev_g0, 0)); }
    HIPCHK(hipGraphLaunch(g.exec, c->own_stream));
    if (user != c->own_stream) { HIPCHK(hipEventRecord(c->ev_g1, c->own_stream)); HIPCHK(hipStreamWaitEvent(user, c->ev_g1, 0)); }
    ++c->graph_replays;
    return 0;
}

extern "C" {

// Sub-boxes tiling the region [origin, origin + region) of a periodic box; results are written into an
// output array of spatial size `osize` at `oorigin` + the sub-box anchor inside the region.
int nbe_plan_tiles(const int64_t region[3], const int ndiv[3], int max_tile, int out_ndiv[3]) {
    if (!region || !ndiv || !out_ndiv) return fail("null argument");
    bool ok = max_tile > 0;
    for (int a = 0; a < 3 && ok; ++a) {
        if (ndiv[a] < 1 || region[a] < 1) return fail("sizes and ndiv must be positive");
        const int64_t crop = region[a] / ndiv[a];
        // merging is exact only when every anchor keeps the 2^3 stride lattice phase (crop % 8 == 0)
        // and nothing is left over (subbox.py:49 floors; the remainder stays zero)
        if (crop % 8 != 0 || crop * ndiv[a] != region[a]) ok = false;
    }
    for (int a = 0; a < 3; ++a) {
        out_ndiv[a] = ndiv[a];
        if (!ok) continue;
        const int64_t crop = region[a] / ndiv[a];
        int best = 1;
        for (int m = 1; m <= ndiv[a]; ++m)
            if (ndiv[a] % m == 0 && crop * m <= max_tile) best = m;
        out_ndiv[a] = ndiv[a] / best;
    }
    return 0;
}

}  // extern "C"

// Schedule for a (D,H,W) input under a memory budget: 0 = whole tensors, S > 0 = z-slab schedule with S planes per
// slab (the deepest that fits), -1 = nothing fits.  *need receives the workspace bytes of the choice.
int choose_slab(nbe_ctx* c, int D, int H, int W, int64_t budget, int64_t* need_out, bool pyx, bool pz) {
    const int forced = c->slab_forced;
    int result = -1;
    // deeper slabs than 128 planes buy < 1 % (the 2-plane overlaps are already < 5 % there) for tens of GB of workspace
    const int cand[4] = {0, 128, 64, 32};
    for (int i = 0; i < 4 && result < 0; ++i) {
        int S = cand[i];
        if (pyx && S == 0) { if (forced == 0) break; continue; }  // periodic-yx exists only in the slab schedule
        if (forced == 0 && S != 0) break;
        if (forced > 0) { if (i > (pyx ? 1 : 0)) break; S = forced & ~1; }
        if (!pyx && S > 0 && D - 8 <= S) continue;                // a single slab is the whole-tensor schedule
        const int64_t need = workspace_need(c, D, H, W, S, pyx, pyx && pz);
        if (need >= 0 && need <= budget) { result = S; if (need_out) *need_out = need; }
    }
    return result;
}

// The schedule of a tile of e0 x e1 x e2 output voxels under a memory budget, installed in c (c->slab, c->pyx, c->pz):
// periodic-yx when the tile spans the periodic box in y and x (spans_yx), then also periodic in z when it is the box's
// whole z extent (whole_z); padded otherwise.  false: nothing fits, c is left as it was -- unless fallback32 (nothing fits
// the budget: the padded schedule in 32-plane slabs, the smallest footprint, when the slab depth is not forced).
static bool choose_schedule(nbe_ctx* c, int e0, int e1, int e2, bool spans_yx, bool whole_z, int64_t budget, bool fallback32) {
    const int D = e0 + 96;                                       // input depth: the 48 planes of context on either side
    if (spans_yx && !check_dims_pyx(D, e1 + 2, e2 + 2)) {
        const int sl = choose_slab(c, D, e1 + 2, e2 + 2, budget, nullptr, true, whole_z);
        if (sl > 0) { c->slab = sl; c->pyx = true; c->pz = whole_z; return true; }
    }
    if (check_dims(D, e1 + 96, e2 + 96)) return false;
    int sl = choose_slab(c, D, e1 + 96, e2 + 96, budget, nullptr);
    if (sl < 0 && fallback32 && c->slab_forced < 0 && D - 8 > 32) sl = 32;
    if (sl < 0) return false;
    c->slab = sl; c->pyx = false; c->pz = false;
    return true;
}

// The grid process_region will run: among all merges of the caller's sub-boxes (exact only when crop % 8 == 0 on
// every axis) with tile edge <= max_tile, the one with the largest tile volume whose workspace fits the device
// memory that is free now (plus what this context already holds, minus `reserve`); ties go to the tile that is
// longest along the last (fastest) axis.  512^3 / ndiv 4 on a 288 GB MI355X: four tiles of 256 x 256 x 512
// (input 352 x 352 x 608, a ~175 GB workspace), 12 % fewer FLOPs than eight tiles of 256^3.
int64_t plan_budget(nbe_ctx* c, int64_t reserve) {
    size_t free_b = 0, total_b = 0;
    if (hipMemGetInfo(&free_b, &total_b) != hipSuccess) { (void)hipGetLastError(); return -1; }
    // NBE_MEM_FRACTION (default 1): share of the free memory this context may plan with -- for rigs that run several
    // ranks on one card, where every rank sees the same free memory at the same time
    static const double frac = getenv("NBE_MEM_FRACTION") ? std::min(1.0, std::max(0.01, atof(getenv("NBE_MEM_FRACTION")))) : 1.0;
    return (int64_t)(((double)free_b + (double)c->ws_bytes) * frac) - reserve - ((int64_t)3 << 30);
}

static int plan_tiles_mem(nbe_ctx* c, const int64_t region[3], const int ndiv[3], int64_t reserve, bool full_yx,
                          bool full_z, int out_ndiv[3]) {
    for (int a = 0; a < 3; ++a) out_ndiv[a] = ndiv[a];
    c->slab = 0;
    c->pyx = false; c->pz = false;
    if (!c->have_weights) return 0;
    full_yx = full_yx && c->pyx_allowed;
    const int64_t budget = plan_budget(c, reserve);
    if (budget < 0) return 0;
    // the caller's own grid; from here on c holds the schedule of the best tile so far
    choose_schedule(c, (int)(region[0] / ndiv[0]), (int)(region[1] / ndiv[1]), (int)(region[2] / ndiv[2]),
                    full_yx && ndiv[1] == 1 && ndiv[2] == 1, full_z && ndiv[0] == 1, budget, false);
    (void)nbe_last_error();
    if (c->max_tile <= 0) return 0;
    int64_t crop[3];
    for (int a = 0; a < 3; ++a) {
        if (ndiv[a] < 1 || region[a] < 1) return fail("sizes and ndiv must be positive");
        crop[a] = region[a] / ndiv[a];
        if (crop[a] % 8 != 0 || crop[a] * ndiv[a] != region[a]) return 0;      // merging would not be exact
    }
    int64_t best_vol = 0, best_w = 0, miss_vol = 0, miss_need = 0;
    for (int m0 = 1; m0 <= ndiv[0]; ++m0) {
        if (ndiv[0] % m0 || crop[0] * m0 > c->max_tile) continue;
        for (int m1 = 1; m1 <= ndiv[1]; ++m1) {
            if (ndiv[1] % m1 || crop[1] * m1 > c->max_tile) continue;
            for (int m2 = 1; m2 <= ndiv[2]; ++m2) {
                if (ndiv[2] % m2 || crop[2] * m2 > c->max_tile) continue;
                const int64_t e0 = crop[0] * m0, e1 = crop[1] * m1, e2 = crop[2] * m2, vol = e0 * e1 * e2;
                const int64_t w = e2 * 1000000 + e1 * 1000 + e0;               // tie-break: long last axis
                if (vol < best_vol || (vol == best_vol && w <= best_w)) continue;
                const bool spans = full_yx && m1 == ndiv[1] && m2 == ndiv[2], whole_z = full_z && e0 == region[0];
                if (!choose_schedule(c, (int)e0, (int)e1, (int)e2, spans, whole_z, budget, false)) {
                    (void)nbe_last_error();
                    if (vol > miss_vol) {                        // what the largest merge that did not fit would have needed
                        const int ext = spans ? 2 : 96;
                        const int64_t need = workspace_need(c, (int)e0 + 96, (int)e1 + ext, (int)e2 + ext, 32, spans, spans && whole_z);
                        (void)nbe_last_error();
                        if (need > 0) { miss_vol = vol; miss_need = need; }
                    }
                    continue;
                }
                best_vol = vol; best_w = w;
                out_ndiv[0] = ndiv[0] / m0; out_ndiv[1] = ndiv[1] / m1; out_ndiv[2] = ndiv[2] / m2;
            }
        }
    }
    c->plan_tiles = out_ndiv[0] * out_ndiv[1] * out_ndiv[2];
    c->plan_short_gb = 0.0;
    if (miss_vol > best_vol) {                                   // a larger exact merge exists and only memory kept the planner from it
        c->plan_short_gb = std::max(0.0, (double)(miss_need - budget) / 1e9);
        static const bool quiet = getenv("NBE_QUIET") && atoi(getenv("NBE_QUIET")) != 0;
        const int64_t key = miss_vol * 1000 + c->plan_tiles;
        if (!quiet && key != c->plan_logged) {
            fprintf(stderr, "nbe: box %lld x %lld x %lld runs as %d x %d x %d tiles: a larger tile needs at least %.0f GB of workspace (even in "
                            "32-plane slabs), %.0f GB are free for it on device %d -- expect 1.1 - 1.4 x the time of the larger plan\n",
                    (long long)region[0], (long long)region[1], (long long)region[2], out_ndiv[0], out_ndiv[1], out_ndiv[2],
                    miss_need / 1e9, budget / 1e9, c->device);
            c->plan_logged = key;
        }
    }
    return 0;
}

extern "C" {
int nbe_plan_tiles_ctx(nbe_ctx* c, const int64_t region[3], const int ndiv[3], int periodic_box, int out_ndiv[3]) {
    if (!c || !region || !ndiv || !out_ndiv) return fail("null argument");
    HIPCHK(hipSetDevice(c->device));
    return plan_tiles_mem(c, region, ndiv, 0, periodic_box != 0, periodic_box != 0, out_ndiv);
}

}  // extern "C"

// One process_box / process_region call: its arguments, and what the three steps below derive from them in turn.
struct RegionCall {
    const void* box; const int64_t *bsize, *origin, *region; const int* ndiv_in; const int* order; int norder;
    float Dz, vel_fac; void *disp, *vel; int out_dtype; const int64_t *osize, *oorigin; bool zero_out;
    nbe_progress_cb cb; void* user;
    int S0, S1, S2, O0, O1, O2;                                   // box and output array extents
    int esz; int64_t in_bytes, out_bytes;                         // bytes of the input box and of one output field
    bool in_dev, out_dev;
    int ndiv[3];                                                  // region_plan: the grid that runs
    int c0, c1, c2, hal, D, H, W;                                 // ... a tile's output extent, y/x context and input extent
    const float* bd; char *dd, *vd; bool piped;                   // region_stage: the device box, the device outputs
};

// Step 1: the grid and the schedule (c->slab, c->pyx, c->pz), with the workspace allocated.
static int region_plan(nbe_ctx* c, RegionCall& r) {
    const int64_t *origin = r.origin, *region = r.region, *bsize = r.bsize;
    const int *ndiv_in = r.ndiv_in, *order = r.order;
    // Internal tiling: with an explicit sub-box list the caller's grid is used as given; otherwise adjacent
    // sub-boxes may be merged into larger tiles (nbe_plan_tiles) -- identical results, less halo recompute.
    int* ndiv_eff = r.ndiv;
    for (int a = 0; a < 3; ++a) ndiv_eff[a] = ndiv_in[a];
    {
        // host arrays in / out are staged in device buffers that are allocated below: keep room for them
        const int64_t reserve = (r.in_dev ? 0 : std::max<int64_t>(0, r.in_bytes - c->box_in_bytes)) +
                                (r.out_dev ? 0 : std::max<int64_t>(0, r.out_bytes * (c->vel ? 2 : 1) - c->box_out_bytes));
        // the region is the periodic box itself in y and x: tiles that span it may run in periodic-yx mode
        const bool full_yx = c->pyx_allowed && origin[1] == 0 && origin[2] == 0 && region[1] == bsize[1] && region[2] == bsize[2];
        const bool full_z = origin[0] == 0 && region[0] == bsize[0];        // ... and in z
        auto tile_dims = [&](int* d, int* h, int* w) {            // input dims of a tile of the current grid / mode
            const int ext = c->pyx ? 2 : 96;
            *d = (int)(region[0] / ndiv_eff[0]) + 96; *h = (int)(region[1] / ndiv_eff[1]) + ext; *w = (int)(region[2] / ndiv_eff[2]) + ext;
        };
        // schedule (whole tensors or z-slabs, padded or periodic-yx) of a given grid under the memory that is free now
        auto schedule_for_grid = [&]() {
            c->slab = 0; c->pyx = false; c->pz = false;
            const int64_t budget = plan_budget(c, reserve);
            if (budget < 0 || !c->have_weights) return;
            choose_schedule(c, (int)(region[0] / ndiv_eff[0]), (int)(region[1] / ndiv_eff[1]), (int)(region[2] / ndiv_eff[2]),
                            full_yx && ndiv_eff[1] == 1 && ndiv_eff[2] == 1, full_z && ndiv_eff[0] == 1, budget, true);
            (void)nbe_last_error();
        };
        if (order) schedule_for_grid();                          // explicit sub-box list: the caller's grid as given
        else if (plan_tiles_mem(c, region, ndiv_in, reserve, full_yx, full_z, ndiv_eff)) return 1;
        // fall back to cubic tiles <= 256, then to the caller's grid, when the workspace cannot be allocated after all
        for (int attempt = 0; attempt < 2 && !order; ++attempt) {
            if (ndiv_eff[0] == ndiv_in[0] && ndiv_eff[1] == ndiv_in[1] && ndiv_eff[2] == ndiv_in[2]) break;
            int d, h, w; tile_dims(&d, &h, &w);
            if (!ensure_workspace(c, d, h, w)) break;
            (void)hipGetLastError();
            if (attempt == 0 && c->max_tile > 256) { if (nbe_plan_tiles(region, ndiv_in, 256, ndiv_eff)) return 1; }
            else { ndiv_eff[0] = ndiv_in[0]; ndiv_eff[1] = ndiv_in[1]; ndiv_eff[2] = ndiv_in[2]; }
            schedule_for_grid();
        }
    }
    const int* ndiv = ndiv_eff;
    r.c0 = (int)(region[0] / ndiv[0]); r.c1 = (int)(region[1] / ndiv[1]); r.c2 = (int)(region[2] / ndiv[2]);   // subbox.py:49 (floor)
    r.hal = c->pyx ? 1 : 48;                                      // y/x context gathered with the tile
    r.D = r.c0 + 96; r.H = r.c1 + 2 * r.hal; r.W = r.c2 + 2 * r.hal;
    if (c->pyx ? check_dims_pyx(r.D, r.H, r.W) : check_dims(r.D, r.H, r.W)) return 1;
    for (int i = 0; i < 3; ++i)
        if (r.oorigin[i] < 0 || r.oorigin[i] + region[i] > r.osize[i]) return fail("output region does not fit the output array");
    HIPCHK(hipSetDevice(c->device));
    return ensure_workspace(c, r.D, r.H, r.W);
}

// Step 2: the host pipe (c->pipe) where the call qualifies for it, and the device staging of host arrays.
static int region_stage(nbe_ctx* c, RegionCall& r) {
    const void* box = r.box; void *disp = r.disp, *vel = r.vel;
    const int64_t *origin = r.origin, *region = r.region, *oorigin = r.oorigin;
    const int* order = r.order; const int* ndiv = r.ndiv;
    const int S0 = r.S0, S1 = r.S1, S2 = r.S2, O0 = r.O0, O1 = r.O1, O2 = r.O2, c0 = r.c0, c1 = r.c1, c2 = r.c2, esz = r.esz;
    const int64_t in_bytes = r.in_bytes, out_bytes = r.out_bytes;
    const bool in_dev = r.in_dev, out_dev = r.out_dev;
    r.bd = (const float*)box;
    // Host arrays in and out, the whole periodic box as one tile in the z-slab schedule, pinned outputs: pipelined
    // (HostPipe).  Anything else: the box goes up in one piece before the first tile and the fields come down after the last.
    const bool pipe_off = getenv("NBE_HOST_PIPE") && atoi(getenv("NBE_HOST_PIPE")) == 0;   // read per call: A/B in one process
    auto& P = c->pipe;
    P.active = false;
    P.tiles = false; P.slabwise = false;
    const bool whole_box = S0 == O0 && S1 == O1 && S2 == O2 && oorigin[0] == 0 && oorigin[1] == 0 && oorigin[2] == 0 &&
                           origin[0] == 0 && origin[1] == 0 && origin[2] == 0 && region[0] == S0 && region[1] == S1 && region[2] == S2;
    const bool one_tile = c->slab > 0 && c->pyx && c->pz && ndiv[0] * ndiv[1] * ndiv[2] == 1;
    // several tiles that cover the box exactly (nothing left for the zeros of subbox.py:168-170): pipelined tile by tile
    const bool many = !one_tile && (int64_t)c0 * ndiv[0] == S0 && (int64_t)c1 * ndiv[1] == S1 && (int64_t)c2 * ndiv[2] == S2;
    if (!in_dev && !out_dev && !order && !pipe_off && whole_box && (one_tile || many)) {
        P.active = one_tile; P.tiles = many;
        P.hbox = (const float*)box; P.in_pinned = is_pinned_host_ptr(box);
        P.C = c->in_chan; P.S0 = S0; P.S1 = S1; P.S2 = S2; P.o0 = (int)origin[0] - 48;
        P.up.assign(S0, 0); P.gz = 0; P.nstage = 0;
        P.out_async = is_pinned_host_ptr(disp) && (!c->vel || is_pinned_host_ptr(vel));
        P.hdisp = (char*)disp; P.hvel = c->vel ? (char*)vel : nullptr; P.esz = esz; P.O0 = O0; P.O1 = O1; P.O2 = O2;
        if (!c->up_stream) {
            HIPCHK(hipStreamCreateWithFlags(&c->up_stream, hipStreamNonBlocking));
            HIPCHK(hipStreamCreateWithFlags(&c->down_stream, hipStreamNonBlocking));
            HIPCHK(hipEventCreateWithFlags(&c->ev_up, hipEventDisableTiming));
            HIPCHK(hipEventCreateWithFlags(&c->ev_down, hipEventDisableTiming));
            for (int i = 0; i < nbe_ctx::NSTAGE; ++i) HIPCHK(hipEventCreateWithFlags(&c->stage_free[i], hipEventDisableTiming));
        }
        const int64_t sb = (int64_t)PIPE_CHUNK * S1 * S2 * 4 * c->in_chan;
        if (!P.in_pinned && sb > c->stage_bytes) {
            for (int i = 0; i < nbe_ctx::NSTAGE; ++i) {
                if (c->stage_buf[i]) (void)hipHostFree(c->stage_buf[i]);
                c->stage_buf[i] = nullptr;
                HIPCHK(hipHostMalloc((void**)&c->stage_buf[i], sb, hipHostMallocDefault));
            }
            c->stage_bytes = sb;
        }
    }
    c->last_piped = P.active || P.tiles;
    r.piped = P.active || P.tiles;
    if (!in_dev) {
        if (in_bytes > c->box_in_bytes) { (void)hipFree(c->box_in); c->box_in = nullptr; c->box_in_bytes = 0;
                                          HIPCHK(hipMalloc((void**)&c->box_in, in_bytes)); c->box_in_bytes = in_bytes; }
        if (r.piped) {
            // whatever still reads the device box from the previous call must have finished before the uploads start
            HIPCHK(hipStreamSynchronize(c->stream));
        } else {
            HIPCHK(hipMemcpyAsync(c->box_in, box, in_bytes, hipMemcpyHostToDevice, c->stream));
        }
        r.bd = c->box_in;
    }
    r.dd = (char*)disp; r.vd = (char*)vel;
    if (!out_dev) {
        const int64_t need = out_bytes * (c->vel ? 2 : 1);
        if (need > c->box_out_bytes) { (void)hipFree(c->box_out); c->box_out = nullptr; c->box_out_bytes = 0;
                                       HIPCHK(hipMalloc((void**)&c->box_out, need)); c->box_out_bytes = need; }
        r.dd = c->box_out; r.vd = c->box_out + out_bytes;
        P.ddisp = r.dd; P.dvel = c->vel ? r.vd : nullptr;
    }
    return 0;
}

// Step 3: the tiles, in order, and what comes back to the host after them.
static int region_tiles(nbe_ctx* c, RegionCall& r) {
    const void* box = r.box; void *disp = r.disp, *vel = r.vel;
    const int64_t *origin = r.origin, *oorigin = r.oorigin;
    const int* order = r.order; const int norder = r.norder; const int* ndiv = r.ndiv;
    const int S0 = r.S0, S1 = r.S1, S2 = r.S2, O0 = r.O0, O1 = r.O1, O2 = r.O2;
    const int c0 = r.c0, c1 = r.c1, c2 = r.c2, hal = r.hal, D = r.D, H = r.H, W = r.W;
    const int64_t out_bytes = r.out_bytes;
    const bool in_dev = r.in_dev, out_dev = r.out_dev, piped = r.piped;
    const float Dz = r.Dz, vel_fac = r.vel_fac;
    const float* bd = r.bd; char *dd = r.dd, *vd = r.vd;
    nbe_progress_cb cb = r.cb; void* user = r.user;
    auto& P = c->pipe;
    // subbox.py:168-170: outputs start as zeros (voxels beyond ndiv*crop_size stay zero); the one-tile plan of the
    // pipelined path writes every voxel
    if ((r.zero_out || !out_dev) && !piped) {
        HIPCHK(hipMemsetAsync(dd, 0, out_bytes, c->stream));
        if (c->vel) HIPCHK(hipMemsetAsync(vd, 0, out_bytes, c->stream));
    }
    const bool trace = piped && getenv("NBE_PIPE_TRACE") && atoi(getenv("NBE_PIPE_TRACE")) != 0;
    const auto t_start = std::chrono::steady_clock::now();
    auto ms_since = [&]() { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_start).count(); };
    double t_up0 = 0, t_range = 0, t_enq = 0;
    std::unique_ptr<Progress> reporter;
    if (cb) reporter.reset(new Progress(cb, user, c->device));
    struct ProgGuard { nbe_ctx* c; ~ProgGuard() { c->prog = nullptr; c->prog_cb = nullptr; } } prog_guard{c};
    c->prog = reporter.get();
    // tiles in the z-slab schedule gather slab by slab as their planes land (the first tile of a 1024^3 box would otherwise
    // wait for 608 planes = 7.6 GB before its first kernel)
    P.slabwise = P.tiles && c->slab > 0;
    if (piped) {
        // start the upload of the first tile's first slab (outside the z-slab schedule: of the whole tile), then reduce
        // max|x| on the host while the DMA runs
        P.o0 = -48;
        const int zs = c->pyx && c->pz ? 40 : 0;                 // (the one-tile plan is periodic in z: its encoder starts at plane 40)
        if (P.active || P.slabwise ? pipe_upload(c, zs, zs + std::min(c->slab, PIPE_EDGE) + 8) : pipe_upload(c, 0, D)) return 1;
        t_up0 = ms_since();
        if (prepare_range(c, nullptr, (int64_t)c->in_chan * S0 * S1 * S2, Dz, (const float*)box)) return 1;
        t_range = ms_since();
    } else if (prepare_range(c, bd, (int64_t)c->in_chan * S0 * S1 * S2, Dz)) return 1;
    const int total = ndiv[0] * ndiv[1] * ndiv[2];
    const int n = order ? norder : total;
    for (int k = 0; k < n; ++k) {
        const int idx = order ? order[k] : k;
        if (idx < 0 || idx >= total) return fail("sub-box index %d out of range (0..%d)", idx, total - 1);
        // subbox.py:60-66: row-major over ndiv, last axis fastest
        const int a0 = (idx / (ndiv[1] * ndiv[2])) * c0, a1 = ((idx / ndiv[2]) % ndiv[1]) * c1, a2 = (idx % ndiv[2]) * c2;
        c->prog_cb = cb; c->prog_user = user; c->prog_k = k; c->prog_n = n;
        if (P.tiles) {                                           // this tile's planes (most were sent under the tile before)
            P.o0 = a0 - 48; P.o1 = a1 - hal; P.o2 = a2 - hal; P.gz = 0;
            if (!P.slabwise) {
                if (pipe_upload(c, 0, D)) return 1;
                HIPCHK(hipEventRecord(c->ev_up, c->up_stream));
                HIPCHK(hipStreamWaitEvent(c->stream, c->ev_up, 0));
            }
        }
        if (c->probe.on) {                                       // branch probe: armed for the tile that holds the block
            auto& Pb = c->probe;
            const int ta[3] = {(int)oorigin[0] + a0, (int)oorigin[1] + a1, (int)oorigin[2] + a2}, te[3] = {c0, c1, c2};
            Pb.tile = true;
            for (int d = 0; d < 3; ++d) {
                Pb.o[d] = Pb.p[d] - ta[d];
                if (Pb.o[d] < 0 || Pb.o[d] + Pb.nout > te[d] || Pb.o[d] % 8 != 0) Pb.tile = false;
            }
        }
        if (run_tile(c, bd, S0, S1, S2, (int)origin[0] + a0 - 48, (int)origin[1] + a1 - hal, (int)origin[2] + a2 - hal,
                       D, H, W, Dz, vel_fac, dd, vd, r.out_dtype, O0, O1, O2,
                       (int)oorigin[0] + a0, (int)oorigin[1] + a1, (int)oorigin[2] + a2)) return 1;
        if (P.tiles) {
            if (P.out_async && pipe_output(c, a0, c0, a1, a2, c1, c2)) return 1;
            if (k + 1 < n) {                                     // the next tile's planes go up under this tile's kernels
                const int idn = k + 1;
                P.o0 = (idn / (ndiv[1] * ndiv[2])) * c0 - 48;
                if (pipe_upload(c, 0, D)) return 1;              // (what this tile's slabs have not already brought up)
            }
        }
        if (reporter) reporter->post(piped && P.out_async ? c->down_stream : c->stream, (k + 1) * 1000, n * 1000);
    }
    c->prog_cb = nullptr;
    HIPCHK(hipGetLastError());
    if (!out_dev && !(piped && P.out_async)) {
        HIPCHK(hipMemcpyAsync(disp, dd, out_bytes, hipMemcpyDeviceToHost, c->stream));
        if (c->vel) HIPCHK(hipMemcpyAsync(vel, vd, out_bytes, hipMemcpyDeviceToHost, c->stream));
    }
    if (!out_dev || !in_dev) {
        t_enq = ms_since();
        HIPCHK(hipStreamSynchronize(c->stream));
        const double t_comp = ms_since();
        if (piped) { HIPCHK(hipStreamSynchronize(c->up_stream)); HIPCHK(hipStreamSynchronize(c->down_stream)); }
        reporter.reset();                                        // every report has been delivered when this returns
        if (trace)
            fprintf(stderr, "nbe pipe: first upload staged %.1f ms, max|x| on %d host threads %.1f ms, all work enqueued %.1f ms, "
                            "kernels done %.1f ms, last slab on the host %.1f ms (input %s, outputs %s)\n",
                    t_up0, host_threads(), t_range - t_up0, t_enq, t_comp, ms_since(), P.in_pinned ? "pinned" : "pageable",
                    P.out_async ? "pinned" : "pageable");
        return check_range(c);                                  // host arrays: the call is synchronous anyway
    }
    if (reporter) { HIPCHK(hipStreamSynchronize(c->stream)); reporter.reset(); }   // a call with a progress callback is synchronous
    return 0;
}

static int process_region(nbe_ctx* c, const void* box, const int64_t bsize[3], const int64_t origin[3],
                          const int64_t region[3], const int ndiv_in[3], const int* order, int norder,
                          float Dz, float vel_fac, void* disp, void* vel, int out_dtype,
                          const int64_t osize[3], const int64_t oorigin[3], bool zero_out,
                          nbe_progress_cb cb, void* user) {
    if (require_ready(c)) return 1;
    if (c->vel && !vel) return fail("velocity output pointer is NULL but compute_vel is set");
    if (out_dtype != NBE_F32 && out_dtype != NBE_F16) return fail("out_dtype must be NBE_F32 or NBE_F16");
    for (int i = 0; i < 3; ++i) {
        if (ndiv_in[i] < 1 || bsize[i] < 1 || region[i] < 1 || osize[i] < 1) return fail("sizes and ndiv must be positive");
        if (bsize[i] > 2000000000LL / 4 || osize[i] > 2000000000LL / 4) return fail("box axis too large");
    }
    RegionCall r{};
    r.box = box; r.bsize = bsize; r.origin = origin; r.region = region; r.ndiv_in = ndiv_in; r.order = order; r.norder = norder;
    r.Dz = Dz; r.vel_fac = vel_fac; r.disp = disp; r.vel = vel; r.out_dtype = out_dtype; r.osize = osize; r.oorigin = oorigin;
    r.zero_out = zero_out; r.cb = cb; r.user = user;
    r.S0 = (int)bsize[0]; r.S1 = (int)bsize[1]; r.S2 = (int)bsize[2];
    r.O0 = (int)osize[0]; r.O1 = (int)osize[1]; r.O2 = (int)osize[2];
    r.esz = out_dtype == NBE_F16 ? 2 : 4;
    r.in_bytes = (int64_t)r.S0 * r.S1 * r.S2 * c->in_chan * 4;
    r.out_bytes = (int64_t)r.O0 * r.O1 * r.O2 * c->out_chan * r.esz;
    HIPCHK(hipSetDevice(c->device));
    r.in_dev = is_device_ptr(box); r.out_dev = is_device_ptr(disp);
    if (region_plan(c, r)) return 1;
    // (the guard stands before the pipe is set up: no error path leaves its flags set for the context's next call)
    struct PipeGuard { nbe_ctx::HostPipe& p; ~PipeGuard() { p.active = false; p.tiles = false; p.slabwise = false; } } pipe_guard{c->pipe};
    if (region_stage(c, r)) return 1;
    return region_tiles(c, r);
}

extern "C" {

int nbe_process_box(nbe_ctx* c, const void* box, const int64_t size[3], const int ndiv[3], const int pad[6],
                    float Dz, float vel_fac, void* disp, void* vel, int out_dtype, nbe_progress_cb cb, void* user) {
    if (!c || !box || !disp || !size || !ndiv || !pad) return fail("null argument");
    for (int i = 0; i < 6; ++i)
        if (pad[i] != 48) return fail("padding must be 48 on every side (receptive field of the network, subbox.py:43); got %d", pad[i]);
    const int64_t zero[3] = {0, 0, 0};
    return process_region(c, box, size, zero, size, ndiv, nullptr, 0, Dz, vel_fac, disp, vel, out_dtype, size, zero,
                          true, cb, user);
}

int nbe_process_region(nbe_ctx* c, const void* box, const int64_t box_size[3], const int64_t origin[3],
                       const int64_t region[3], const int ndiv[3], const int* order, int norder,
                       float Dz, float vel_fac, void* disp, void* vel, int out_dtype,
                       const int64_t out_size[3], const int64_t out_origin[3]) {
    if (!c || !box || !disp || !box_size || !origin || !region || !ndiv || !out_size || !out_origin) return fail("null argument");
    return process_region(c, box, box_size, origin, region, ndiv, order, norder, Dz, vel_fac, disp, vel, out_dtype,
                          out_size, out_origin, false, nullptr, nullptr);
}

void* nbe_host_alloc(size_t bytes) {
    if (bytes == 0) bytes = 1;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_free.lower_bound(bytes);
        if (it != g_pin_free.end() && it->first <= bytes + bytes / 8) {      // close enough in size: reuse
            void* p = it->second; const size_t sz = it->first;
            g_pin_free.erase(it); g_pin_free_bytes -= sz; g_pin_live[p] = sz;
            return p;
        }
    }
    void* p = nullptr;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); fail("nbe_host_alloc: hipHostMalloc(%zu) failed", bytes); return nullptr; }
    std::lock_guard<std::mutex> lk(g_pin_mu);
    g_pin_live[p] = bytes;
    return p;
}

int nbe_host_free(void* p) {
    if (!p) return 0;
    size_t sz = 0;
    {
        std::lock_guard<std::mutex> lk(g_pin_mu);
        auto it = g_pin_live.find(p);
        if (it == g_pin_live.end()) return fail("nbe_host_free: %p was not allocated by nbe_host_alloc", p);
        sz = it->second; g_pin_live.erase(it);
        if (g_pin_free_bytes + sz <= pin_pool_cap()) { g_pin_free.emplace(sz, p); g_pin_free_bytes += sz; return 0; }
    }
    (void)hipHostFree(p);
    return 0;
}

int nbe_host_trim(void) {
    std::lock_guard<std::mutex> lk(g_pin_mu);
    for (auto& kv : g_pin_free) (void)hipHostFree(kv.second);
    g_pin_free.clear(); g_pin_free_bytes = 0;
    return 0;
}

}  // extern "C"
