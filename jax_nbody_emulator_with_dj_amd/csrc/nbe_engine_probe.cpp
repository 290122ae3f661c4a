// Instrumentation: the branch probe (include/nbe.h, test instrumentation) and the per-kernel profiler.
#include "nbe_engine_internal.h"

// Record the branch bits of the activation tensor a launch of layer L has just written: `out` points at the launch's
// output voxel (0, 0, 0), `ext` voxels from there, whose index in the oracle's frame is `org`; periodic in y / x with the
// extent as period when `periodic`.
// zr = {lo, hi, period}: the layer's tensor exists for the planes [lo, hi) of a box that is periodic along z (the level-0
// encoder of a tile that is the whole box computes N + a few planes, down_l0 exactly N / 2; what lies outside is a periodic image)
void probe_act(nbe_ctx* c, const Layer& L, const Planes& out, int g0, const int org[3], int ez, int ey, int ex, bool periodic,
               const int* zr) {
    auto& P = c->probe;
    if (!P.on || !P.tile || c->dry) return;
    const std::string name = L.block + "/" + L.layer;
    for (size_t i = 0; i < P.slots.size(); ++i) {
        const auto& S = P.slots[i];
        if (S.name != name) continue;
        ProbeLaunch a;
        a.x = out.x; a.pstride = out.pstride; a.H = out.H; a.W = out.W; a.g0 = g0; a.prec = c->prec; a.C = S.C;
        a.ext[0] = ez; a.ext[1] = ey; a.ext[2] = ex;
        a.org[0] = org[0]; a.org[1] = org[1]; a.org[2] = org[2];
        a.per[0] = 0; a.per[1] = periodic ? ey : 0; a.per[2] = periodic ? ex : 0;
        a.zlo = zr ? zr[0] : 0; a.zhi = zr ? zr[1] : 0; a.zper = zr ? zr[2] : 0;
        for (int d = 0; d < 3; ++d) a.o[d] = P.o[d] >> S.level;
        a.n = S.n; a.nw = S.nw;
        if (a.zper <= 0 && (a.o[0] + S.n <= org[0] || a.o[0] >= org[0] + ez)) return;      // this launch's planes lie outside the cone
        a.bits = P.bits + S.off; a.count = P.count + i;
        launch_probe_signs(a, c->stream);
        return;
    }
}

int prof_entry(nbe_ctx* c, const std::string& name) {
    for (size_t i = 0; i < c->prof_entries.size(); ++i) if (c->prof_entries[i].name == name) return (int)i;
    c->prof_entries.push_back({name, 0, 0, 0});
    return (int)c->prof_entries.size() - 1;
}
hipEvent_t get_event(nbe_ctx* c) {
    if (!c->ev_pool.empty()) { hipEvent_t e = c->ev_pool.back(); c->ev_pool.pop_back(); return e; }
    hipEvent_t e; (void)hipEventCreate(&e); return e;
}
void prof_collect(nbe_ctx* c) {
    if (c->pending.empty()) return;
    (void)hipStreamSynchronize(c->stream);
    for (auto& p : c->pending) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, p.a, p.b);
        c->prof_entries[p.entry].ms += ms;
        c->ev_pool.push_back(p.a); c->ev_pool.push_back(p.b);
    }
    c->pending.clear();
}

extern "C" {

// ---- branch probe (test instrumentation) ------------------------------------------------------------------------------
static void probe_free(nbe_ctx* c) {
    (void)hipFree(c->probe.bits); (void)hipFree(c->probe.count);
    c->probe = nbe_ctx::Probe();
}

int nbe_probe_begin(nbe_ctx* c, const int64_t origin[3], int nout) {
    if (!c || !origin) return fail("null argument");
    if (nout < 8 || nout % 8 != 0 || nout > 128) return fail("branch probe: the block edge must be a multiple of 8 in 8..128");
    for (int d = 0; d < 3; ++d) if (origin[d] < 0 || origin[d] % 8 != 0) return fail("branch probe: the block origin must be a non-negative multiple of 8");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    probe_free(c);
    auto& P = c->probe;
    P.nout = nout;
    for (int d = 0; d < 3; ++d) P.p[d] = (int)origin[d];
    // the activation tensors of the cone of an (nout + 96)^3 input, in execution order (core :105-195)
    const int m = c->mid, n0 = nout + 96;
    const int m1 = (n0 - 8) / 2, m2 = (m1 - 4) / 2, m3 = (m2 - 4) / 2, u2 = 2 * (m3 - 4), u1 = 2 * (u2 - 4), u0 = 2 * (u1 - 4);
    struct Row { const char* name; int C, n, level; };
    const Row rows[] = {
        {"conv_l00/conv_0", m, n0 - 2, 0}, {"conv_l00/conv_1", m, n0 - 4, 0}, {"conv_l01/conv_0", m, n0 - 6, 0}, {"conv_l01/conv_1", m, n0 - 8, 0},
        {"down_l0/conv_0", m, m1, 1}, {"conv_l1/conv_0", m, m1 - 2, 1}, {"conv_l1/conv_1", m, m1 - 4, 1},
        {"down_l1/conv_0", m, m2, 2}, {"conv_l2/conv_0", m, m2 - 2, 2}, {"conv_l2/conv_1", m, m2 - 4, 2},
        {"down_l2/conv_0", m, m3, 3}, {"conv_c/conv_0", m, m3 - 2, 3}, {"conv_c/conv_1", m, m3 - 4, 3},
        {"up_r2/conv_0", m, u2, 2}, {"conv_r2/conv_0", 2 * m, u2 - 2, 2}, {"conv_r2/conv_1", m, u2 - 4, 2},
        {"up_r1/conv_0", m, u1, 1}, {"conv_r1/conv_0", 2 * m, u1 - 2, 1}, {"conv_r1/conv_1", m, u1 - 4, 1},
        {"up_r0/conv_0", m, u0, 0}, {"conv_r00/conv_0", 2 * m, u0 - 2, 0}, {"conv_r00/conv_1", m, u0 - 4, 0},
        {"conv_r01/conv_0", m, u0 - 6, 0},
    };
    int64_t off = 0;
    for (const Row& r : rows) {
        nbe_ctx::Probe::Slot sl{r.name, r.C, r.n, (r.n + 31) / 32, r.level, off};
        off += (int64_t)sl.C * sl.n * sl.n * sl.nw;
        P.slots.push_back(sl);
    }
    P.words = off;
    HIPCHK(hipMalloc((void**)&P.bits, off * 4));
    HIPCHK(hipMemset(P.bits, 0, off * 4));
    HIPCHK(hipMalloc((void**)&P.count, P.slots.size() * 4));
    HIPCHK(hipMemset(P.count, 0, P.slots.size() * 4));
    P.on = true; P.tile = false;
    return 0;
}

int nbe_probe_slots(nbe_ctx* c) { return c ? (int)c->probe.slots.size() : 0; }

int nbe_probe_layout(nbe_ctx* c, int slot, char* name, int cap, int dims[3], int64_t* word_offset) {
    if (!c || slot < 0 || slot >= (int)c->probe.slots.size()) return fail("branch probe: slot out of range");
    const auto& S = c->probe.slots[slot];
    if (name && cap > 0) { strncpy(name, S.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (dims) { dims[0] = S.C; dims[1] = S.n; dims[2] = S.nw; }
    if (word_offset) *word_offset = S.off;
    return 0;
}

int nbe_probe_read(nbe_ctx* c, void* words, int64_t nwords) {
    if (!c || !words) return fail("null argument");
    auto& P = c->probe;
    if (!P.on) return fail("branch probe: nbe_probe_begin has not been called");
    if (nwords != P.words) return fail("branch probe: the buffer must hold %lld words", (long long)P.words);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    std::vector<unsigned> cnt(P.slots.size());
    HIPCHK(hipMemcpy(cnt.data(), P.count, cnt.size() * 4, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < P.slots.size(); ++i) {
        const auto& S = P.slots[i];
        const int64_t want = (int64_t)S.C * S.n * S.n * S.nw;
        if ((int64_t)cnt[i] != want)
            return fail("branch probe: %s was recorded %u times over %lld words (the block must lie inside one tile of the plan; "
                        "brick mode is not probed)", S.name.c_str(), cnt[i], (long long)want);
    }
    HIPCHK(hipMemcpy(words, P.bits, P.words * 4, hipMemcpyDeviceToHost));
    return 0;
}

int nbe_probe_end(nbe_ctx* c) {
    if (!c) return fail("null context");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    probe_free(c);
    return 0;
}

int nbe_profile_enable(nbe_ctx* c, int on) { if (!c) return fail("null context"); prof_collect(c); c->prof = on != 0; return 0; }
int nbe_profile_reset(nbe_ctx* c) { if (!c) return fail("null context"); prof_collect(c); c->prof_entries.clear(); return 0; }
int nbe_profile_count(nbe_ctx* c) { if (!c) return 0; prof_collect(c); return (int)c->prof_entries.size(); }
int nbe_profile_entry(nbe_ctx* c, int i, char* name, int cap, double* ms, int64_t* launches, double* flops) {
    if (!c || i < 0 || i >= (int)c->prof_entries.size()) return fail("profile entry out of range");
    const ProfEntry& e = c->prof_entries[i];
    if (name && cap > 0) { strncpy(name, e.name.c_str(), cap - 1); name[cap - 1] = 0; }
    if (ms) *ms = e.ms; if (launches) *launches = e.launches; if (flops) *flops = e.flops;
    return 0;
}

int nbe_debug_phase_cycles(nbe_ctx* c, double* out16) {
    if (!c || !out16) return fail("null argument");
    h3q_read_stamps(out16, c->stream);
    return 0;
}

}  // extern "C"
