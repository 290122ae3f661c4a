// What the engine's translation units (nbe_engine*.cpp) share: the context and its parts, and the functions that cross
// units.  Internal to libnbe.so -- the C ABI is include/nbe.h.
#pragma once

#include "../../include/nbe.h"
#include "nbe_conv_select.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <deque>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#pragma GCC visibility push(hidden)          // nothing below is exported from the shared object

using namespace nbe;

int fail(const char* fmt, ...);                  // sets nbe_last_error(); returns 1

#define HIPCHK(expr)                                                                        \
    do {                                                                                    \
        hipError_t e_ = (expr);                                                             \
        if (e_ != hipSuccess) return fail("%s failed: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

static inline int roundup(int v, int m) { return (v + m - 1) / m * m; }

// ------------------------------------------------------------------------------------------------
// workspace: first-fit allocator over one device block; a dry run sizes it
// ------------------------------------------------------------------------------------------------
struct Arena {
    struct Blk { int64_t off, size; bool used; };
    std::vector<Blk> blks;
    int64_t high = 0;
    void reset() { blks.clear(); blks.push_back({0, INT64_MAX / 2, false}); high = 0; }
    int64_t alloc(int64_t bytes) {
        bytes = (bytes + 255) & ~int64_t(255);
        for (size_t i = 0; i < blks.size(); ++i) {
            if (!blks[i].used && blks[i].size >= bytes) {
                Blk rest{blks[i].off + bytes, blks[i].size - bytes, false};
                blks[i].size = bytes; blks[i].used = true;
                if (rest.size > 0) blks.insert(blks.begin() + i + 1, rest);
                if (blks[i].off + bytes > high) high = blks[i].off + bytes;
                return blks[i].off;
            }
        }
        return -1;
    }
    void release(int64_t off) {
        for (size_t i = 0; i < blks.size(); ++i) {
            if (blks[i].off == off && blks[i].used) {
                blks[i].used = false;
                if (i + 1 < blks.size() && !blks[i + 1].used) { blks[i].size += blks[i + 1].size; blks.erase(blks.begin() + i + 1); }
                if (i > 0 && !blks[i - 1].used) { blks[i - 1].size += blks[i].size; blks.erase(blks.begin() + i); }
                return;
            }
        }
    }
};

struct Layer {
    std::string block, layer;
    int cout = 0, cin = 0, k = 0, kind = 0;       // kind: 0 conv3, 1 skip, 2 down, 3 up
    bool first = false;                           // conv_l00/{conv_0,skip}: input linear in Dz
    float *weight = nullptr, *sw = nullptr, *sb = nullptr;   // raw style parameters (device)
    float *wn = nullptr, *dwn = nullptr;          // modulated OIDHW (device)
    PackedW pw;
    PackedW pwn;                                  // narrow (16-cout tile) packing of w for the gauged 3x3x3 kernel: cout <= 16
    // tangent gauge (style path, see conv_h3g_kernel): dw = w_n (.) (alpha[ci] + beta[co])
    float* bias0 = nullptr;                       // the bias as loaded (device, padded like pw.bias, which holds bias0 * act_scale)
    float *alpha = nullptr, *beta = nullptr;      // this layer's own factors (device; cin / cout entries, zero-padded)
    const float* gout = nullptr;                  // gauge of the output tensor = alpha of its 3x3x3 consumer (+ channel offset)
    const float* a_in = nullptr;                  // general kernels: gauge of the input tensor, folded into dw
    bool g6 = false;                              // 3x3x3 layer whose input arrives in its own gauge: two products, no dw
    // Skip fusion (conv_h3g_kernel): a block's conv_1 computes the block's 1x1x1 skip as extra groups on the block input.
    const Layer* fskip = nullptr;                 // conv_1: the block's skip layer, when the block can run fused
    const float* b_sub = nullptr;                 // skip: beta of the block's conv_1, folded into dW_s~ when fused
    float* bias_f = nullptr;                      // conv_1: (b_1 + b_s) * act_scale (device, padded like pw.bias)
    // float16 model: a fused skip exists in the Winograd-z kernel only, and a launch that has no Winograd-z form (an odd number
    // of planes, NBE_WINO=0) runs the block unfused -- so the skip keeps its tangent weights in both versions: dwn without
    // conv_1's beta (pw.dw, the skip's own launch) and dwn_f with it folded in (pw.ww, the fused stages)
    float* dwn_f = nullptr;
};

// pad > 0: the tensor carries a periodic halo of `pad` voxels in y and x around its interior (periodic-yx mode)
// org: index, in the frame of the tensor the oracle forms for this layer on the tile's padded input, of the interior
// voxel (0, 0, 0) -- only the branch probe reads it (whole tensors of a padded tile: all zero)
struct Tensor { Planes p; int64_t off = -1; int pad = 0; int org[3] = {0, 0, 0}; };

struct ProfEntry { std::string name; double ms = 0; int64_t launches = 0; double flops = 0; };

// Progress reports that do not stall the stream.  The reference's process_box shows a tqdm bar by default
// (subbox.py:139-146, :186-193), so the default call carries a callback: the schedule records an event where a unit of work
// ends (a decoder slab's results on their way to the host, a tile) and this thread calls the callback once the event has
// completed -- nothing on the enqueueing side waits for the GPU.
struct Progress {
    struct Item { hipEvent_t ev; int done, total; };
    nbe_progress_cb cb; void* user; int device;
    std::thread th; std::mutex mu; std::condition_variable cv; std::deque<Item> q; bool stop = false;
    Progress(nbe_progress_cb cb_, void* user_, int dev) : cb(cb_), user(user_), device(dev) {
        th = std::thread([this] {
            (void)hipSetDevice(device);
            for (;;) {
                Item it;
                {
                    std::unique_lock<std::mutex> lk(mu);
                    cv.wait(lk, [this] { return stop || !q.empty(); });
                    if (q.empty()) return;
                    it = q.front(); q.pop_front();
                }
                (void)hipEventSynchronize(it.ev);
                (void)hipEventDestroy(it.ev);
                cb(it.done, it.total, user);
            }
        });
    }
    void post(hipStream_t s, int done, int total) {              // "done of total" holds once everything enqueued on s so far has run
        hipEvent_t ev;
        if (hipEventCreateWithFlags(&ev, hipEventDisableTiming) != hipSuccess) return;
        (void)hipEventRecord(ev, s);
        { std::lock_guard<std::mutex> lk(mu); q.push_back({ev, done, total}); }
        cv.notify_one();
    }
    ~Progress() {                                               // reports what is queued, then joins
        { std::lock_guard<std::mutex> lk(mu); stop = true; }
        cv.notify_one();
        if (th.joinable()) th.join();
    }
};

struct nbe_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    int in_chan = 3, out_chan = 3, mid = 64;
    float eps = 1e-8f;
    bool vel = true;
    bool have_weights = false, style = false, modulated = false;
    float mod_Om = NAN, mod_Dz = NAN;
    std::map<std::string, Layer> layers;
    // workspace
    Arena arena;
    char* ws = nullptr;
    int64_t ws_bytes = 0;
    bool dry = false;
    int slab = 0;                                 // z-slab schedule: planes per slab of the full-resolution levels (0 = whole tensors)
    int slab_forced = -1;                         // -1: chosen by memory; 0: never; S > 0: always S (nbe_set_slab, env NBE_SLAB)
    bool pyx = false;                             // current tile runs in periodic-yx mode (it spans the periodic box in y and x)
    bool pyx_allowed = true;                      // env NBE_PERIODIC=0 turns the mode off
    bool pz = false;                              // ... and the tile also spans the box in z (only with pyx)
    // Brick mode of the sharded box (nbe_brick_encode / _interior / _exchange / _finish): the tile is one rank's z-slab of
    // the periodic box, periodic in y and x; in z it runs like pz, except that what the levels read beyond the brick's own
    // planes comes from the neighbours (four exchanges between the calls, network_stream) instead of periodic wrap-around.
    bool zx = false;
    int phase = 0;                                // 0: whole schedule; 1 .. 4: the four brick calls (network_stream)
    struct BrickIO { void *send_lo = nullptr, *send_hi = nullptr; const void *recv_lo = nullptr, *recv_hi = nullptr;
                     void *skip_send_lo = nullptr, *skip_send_hi = nullptr; const void *skip_recv_lo = nullptr, *skip_recv_hi = nullptr;
                     hipEvent_t skip_ready = nullptr; } bio;
    struct StreamState {                          // what the next brick call resumes with (tensors in the arena, which is left alone in between)
        bool valid = false;
        int stage = 0;                            // the last phase that ran (1 encode, 2 interior, 3 edges)
        Tensor skip0, td, tin, t, h, y1, cat1, t2;
        int D = 0, H = 0, W = 0, S = 0;
        std::vector<Arena::Blk> blks; int64_t high = 0;
        float Dz = 0.f, vel_fac = 0.f, act_scale = 1.f; const char* ws = nullptr;   // what the later calls must be made with
    } sst;
    // progress inside a tile (z-slab schedule): tile k of n, reported in thousandths of a tile
    nbe_progress_cb prog_cb = nullptr; void* prog_user = nullptr; int prog_k = 0, prog_n = 1;
    Progress* prog = nullptr;                     // the reporter of the running call (process_region owns it)
    int max_tile = 512;                           // cap on the internal tile edge (output voxels); 0 = caller's grid as given
    int prec = PREC_F32;                          // arithmetic of the convolutions (nbe_set_precision)
    bool gauge = false;                           // the loaded network is wired for gauged tangents (style weights, velocity)
    bool gauge_active = false;                    // ... and the current modulation uses them (no style factor is zero)
    bool fuse = false;                            // ... and the blocks' skips run fused into their conv_1 (f16x3 only)
    bool novel_fuse = false;                      // displacement-only f16x3: the blocks are wired for conv_h3w_kernel<SKIP, NOVEL>
    int64_t bp_size[3] = {0, 0, 0}; int bp_slab = 0; int64_t bp_need = 0;   // the brick plan that nbe_brick_plan / nbe_brick_encode last made
    int plan_tiles = 0;                           // tiles per box of the last plan (nbe_query)
    double plan_short_gb = 0.0;                   // > 0: a larger exact merge existed but its workspace lacked this much memory
    int64_t plan_logged = 0;                      // the situation the last stderr line was about (one line per situation)
    int* gauge_flag = nullptr;                    // device flag of launch_style_alpha
    // Winograd-z form of the gauged 3x3x3 layers (conv_h3w_kernel): packed beside pw.w for every gauged wide layer;
    // wino_ok is cleared when a weight of the current modulation leaves the f16 range at the kernel's 2^14 scale
    int* wino_flag = nullptr; bool wino_ok = false;
    bool direct_z = false;                        // the block being scheduled takes the direct kernels (conv_c: lower_levels)
    // Range shift of the f16-based arithmetic (include/nbe.h, "Range"): activations and biases of a call are multiplied
    // by act_scale = 2^k (exact), the head divides it out.  flags[0]: bit pattern of max |input| (launch_absmax),
    // flags[1]: a non-finite value was written by the head.
    float act_scale = 1.f;                        // 2^k of the current call
    float bias_scale = 1.f;                       // 2^k the device biases currently carry
    bool bias_dirty = true;                       // the scaled biases (pw.bias, bias_f) have to be rewritten (new weights)
    float bias_max = 0.f;                         // max |bias| over all layers (host, at load time)
    float preset_absmax = -1.f;                   // >= 0: max |input| supplied by the caller (nbe_set_input_range)
    bool input_finite = true;                     // the input of the current call had no NaN / infinity
    bool range_pending = false;                   // a call has run since the last nbe_check_finite
    unsigned* flags = nullptr;                    // device: [0] absmax bits, [1] non-finite output
    // device-resident boxes of process_box
    float* box_in = nullptr; int64_t box_in_bytes = 0;
    char* box_out = nullptr; int64_t box_out_bytes = 0;
    // Host-array calls of process_box (the reference's call shape, subbox.py:168-170, :195-215), pipelined: the input
    // box goes up in z-chunks through pinned staging buffers while the encoder slabs run, every finished output slab
    // comes down on a copy stream under the next slab's kernels (HostPipe, below)
    struct HostPipe {
        bool active = false, out_async = false;
        bool tiles = false;                       // several tiles: tile k+1's planes go up and tile k-1's results come down under tile k
        bool slabwise = false;                    // ... and the running tile gathers slab by slab as its planes land (z-slab schedule)
        int o1 = 0, o2 = 0;                       // y / x origin of the running tile's gather (tiles mode; the one-tile plan: -halo)
        const float* hbox = nullptr;              // caller's (C, S0, S1, S2) array
        bool in_pinned = false;
        int C = 0, S0 = 0, S1 = 0, S2 = 0, o0 = 0;    // o0: box plane of tile plane 0 (may be negative: periodic)
        std::vector<char> up;                     // box plane uploaded?
        int gz = 0;                               // tile planes [.., gz) have been gathered
        char *hdisp = nullptr, *hvel = nullptr;   // caller's output arrays (pinned)
        char *ddisp = nullptr, *dvel = nullptr;   // device staging of the outputs
        int esz = 4, O0 = 0, O1 = 0, O2 = 0;
        int nstage = 0;                           // chunks staged so far (ring position)
    } pipe;
    bool last_piped = false;                      // the last process_box / process_region call ran pipelined
    hipStream_t up_stream = nullptr, down_stream = nullptr;
    static constexpr int NSTAGE = 3;
    char* stage_buf[NSTAGE] = {nullptr, nullptr, nullptr}; int64_t stage_bytes = 0;
    hipEvent_t stage_free[NSTAGE] = {nullptr, nullptr, nullptr};
    hipEvent_t ev_up = nullptr, ev_down = nullptr;
    // hipGraph replay of a tile's schedule (run_tile): everything a tile enqueues -- ~300 launches for the 512^3 box as
    // one tile -- is captured the second time the same tile is asked for and replayed from then on
    struct GraphKey {
        const void *box, *disp, *velo, *ws;
        int geo[18]; float f[3]; int epoch, flags;
        bool operator<(const GraphKey& o) const { return memcmp(this, &o, sizeof *this) < 0; }
    };
    struct GraphVal { hipGraphExec_t exec = nullptr; hipGraph_t graph = nullptr; int seen = 0; uint64_t used = 0; };
    std::map<GraphKey, GraphVal> graphs;
    uint64_t graph_clock = 0, graph_replays = 0;
    int epoch = 0;                                // bumped whenever weights, modulation or schedule switches change
    hipEvent_t ev_g0 = nullptr, ev_g1 = nullptr;
    // Branch probe (test instrumentation, include/nbe.h): which LeakyReLU branch every activation in the dependency
    // cone of a block of output voxels took
    struct Probe {
        bool on = false, tile = false;            // armed; the tile being run contains the block
        int p[3] = {0, 0, 0}, nout = 0;           // block origin (output array coordinates) and edge
        int o[3] = {0, 0, 0};                     // ... in the frame of the running tile's padded input (level 0)
        struct Slot { std::string name; int C, n, nw, level; int64_t off; };
        std::vector<Slot> slots;
        unsigned* bits = nullptr; int64_t words = 0;
        unsigned* count = nullptr;                // per slot: words written
    } probe;
    int* paths = nullptr;                         // nbe_test_block: run_conv records which paths the launches took (NBE_PATH_*)
    // profiling
    bool prof = false;
    std::vector<ProfEntry> prof_entries;
    struct Pending { int entry; hipEvent_t a, b; };
    std::vector<Pending> pending;
    std::vector<hipEvent_t> ev_pool;
};

// Where the head writes: the (C, OD, OH, OW) output boxes and the anchor of this tile in them.
struct HeadOut { void* disp; void* velo; int out_dtype; int OD, OH, OW, a0, a1, a2; float Dz, vel_fac; };

// pipelined host path (nbe_engine_box.cpp)
static constexpr int PIPE_EDGE = 32;                             // planes of the first encoder slab and of the last decoder slab

// What a brick needs from its z neighbours below the full-resolution level is exchanged instead of recomputed, at the two
// places where it is smallest: BRICK_H1 planes of the down_l0 output per side (what conv_l1 reads beyond the brick's own
// planes for the level-1 skip connection: 4 + 2) and BRICK_H2 planes of the down_l1 output (what levels 2 and 3 read: 10).
// Own planes of the level-1 input sit at [BRICK_H1, BRICK_H1 + B) of t.
static constexpr int BRICK_H1 = 6, BRICK_H2 = 10;
// ... and at the full-resolution level: BRICK_H0 planes of the skip connection (conv_l01's output) per side, which the decoder's
// first block reads beyond the brick's own planes -- exchanged while levels 1-3 run, instead of 8 more planes through the four
// layers of the level-0 encoder
static constexpr int BRICK_H0 = 4;

// ---- nbe_engine.cpp: context state, range shift ------------------------------------------------------------------
bool is_device_ptr(const void* p);
int require_ready(nbe_ctx* c);
int prepare_range(nbe_ctx* c, const float* dev_src, int64_t n, float Dz, const float* host_src = nullptr);
int check_range(nbe_ctx* c);

// ---- nbe_engine_net.cpp: tensors in the arena, one layer, the blocks, the U-Net schedule ---------------------------
int planes_for(int C, int prec);
Tensor talloc(nbe_ctx* c, int C, int D, int H, int W, bool zero_rest = true);
Tensor tallocp(nbe_ctx* c, int C, int D, int Hi, int Wi, int pad, bool zero_rest = true);
void fill_halo(nbe_ctx* c, const Tensor& t);
void tfree(nbe_ctx* c, Tensor& t);
Tensor zview(const Tensor& t, int z0, int nz);
void set_org(Tensor& t, int z, int y, int x);
bool wino_f16_layer(int prec, bool vel, int cin_pad);
bool wino_env_off();
bool up8_launch(const nbe_ctx* c, const Layer& L, bool has_dx);
int run_conv(nbe_ctx* c, const Layer& L, const ConvLaunch& cl_in, bool has_dx);
const Layer* find_layer(nbe_ctx* c, const char* block, const char* layer);
bool block_fused(const nbe_ctx* c, const Layer* L1, int nres);
bool two_source_width(const nbe_ctx* c);
Tensor alloc_hidden(nbe_ctx* c, int cmid, int nz, const Tensor& x, bool fused);
int resblock_part(nbe_ctx* c, const char* name, const Tensor& x, const Tensor& h, const Tensor& s,
                  int js, int ns, int jh, int nh, bool has_dx, bool final_act, const int* zr, const Tensor* x2 = nullptr,
                  bool halo_s = true);
int resblock(nbe_ctx* c, const char* name, const Tensor& x, bool has_dx, bool final_act, int cout, int cmid, Tensor* out,
             Tensor* hidden_out = nullptr, const int* zr = nullptr, const Tensor* x2 = nullptr);
int down_conv(nbe_ctx* c, const Layer& L, const Tensor& x, Tensor& o, bool probe, const int* zr = nullptr);
int downblock(nbe_ctx* c, const char* name, const Tensor& x, Tensor* out);
int upblock(nbe_ctx* c, const char* name, const Tensor& x, const Tensor& cat, int xcrop = 0, int g0 = -1);
void crop_into(nbe_ctx* c, const Tensor& src, int crop, const Tensor& dst, int cz = -1);
int check_dims(int D, int H, int W);
int check_dims_pyx(int D, int H, int W);
void run_head(nbe_ctx* c, const Tensor& y, const Tensor& xin, const HeadOut& h, int zoff);
int network(nbe_ctx* c, const Tensor& tin, Tensor* yout);
int network_stream(nbe_ctx* c, const Tensor& tin, const HeadOut& ho, int S);

// ---- nbe_engine_weights.cpp: what a layer needs on the device -------------------------------------------------------
PackedW layer_geometry(int prec, int kind, int cout, int cin);
bool packs_narrow(int prec, bool vel, const Layer& L);
bool packs_wino(int prec, bool vel, const Layer& L);
bool packs_wino_skip(int prec, bool vel, bool style, const Layer& L);
bool packs_stem(int prec, const Layer& L);
int alloc_wino(PackedW& pw);
int alloc_stem(PackedW& pw);
int wino_flag_round_trip(nbe_ctx* c, const std::function<void()>& packs);
void release_layer(Layer& L);
void free_layers(nbe_ctx* c);
int pack_wino(nbe_ctx* c);

// ---- nbe_engine_box.cpp: workspace, tiles, host pipe -----------------------------------------------------------------
unsigned host_absmax_bits(const float* x, int64_t n);
int pipe_input(nbe_ctx* c, const Tensor& tin, int t0, int t1, int look, float scale);
int pipe_output(nbe_ctx* c, int z, int n, int a1 = 0, int a2 = 0, int e1 = -1, int e2 = -1);
int ensure_workspace(nbe_ctx* c, int D, int H, int W);
int run_subbox(nbe_ctx* c, const float* box, int Db, int Hb, int Wb, int o0, int o1, int o2,
               int D, int H, int W, float Dz, float vel_fac, void* disp, void* velo, int out_dtype,
               int OD, int OH, int OW, int a0, int a1, int a2);
void drop_graphs(nbe_ctx* c);
int64_t plan_budget(nbe_ctx* c, int64_t reserve);
int choose_slab(nbe_ctx* c, int D, int H, int W, int64_t budget, int64_t* need_out, bool pyx = false, bool pz = false);

// ---- nbe_engine_brick.cpp: the steps of a brick inside network_stream -----------------------------------------------
void brick_send(nbe_ctx* c, const Tensor& t, int in, int n, void* lo, void* hi);
void brick_recv(nbe_ctx* c, const Tensor& like, const void* lo, const void* hi, int n, const Tensor& dst, int wrap);
int brick_interior(nbe_ctx* c, nbe_ctx::StreamState& st);
int brick_edges(nbe_ctx* c, nbe_ctx::StreamState& st);
int brick_level2(nbe_ctx* c, nbe_ctx::StreamState& st, Tensor* t_out);

// ---- nbe_engine_probe.cpp: branch probe and profiler ---------------------------------------------------------------
void probe_act(nbe_ctx* c, const Layer& L, const Planes& out, int g0, const int org[3], int ez, int ey, int ex, bool periodic,
               const int* zr = nullptr);
int prof_entry(nbe_ctx* c, const std::string& name);
hipEvent_t get_event(nbe_ctx* c);
void prof_collect(nbe_ctx* c);

#pragma GCC visibility pop
