// Pieces shared by the context-free entry points (nbe_density.hip, nbe_lpt.hip, nbe_fof.hip, nbe_pairs.hip,
// nbe_profiles.hip): how a mode of torch's row-major half spectrum is decoded, and how such an entry point reports an
// error, checks an argument of a catalogue and sizes a launch.  Each is written once, here.
#pragma once

#include "nbe_catalog.h"

#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>

namespace nbe { int api_fail(const char* msg); }

namespace {

// frequency index of position i on an axis of n points (numpy.fft.fftfreq * n)
__device__ inline long long freq(long long i, long long n) { return i <= n / 2 ? i : i - n; }

// Mode i of the row-major half spectrum (r0, r1, r2/2+1) of an (r0, r1, r2) mesh: its integer frequencies, their
// |m|^2 = q and its weight in the full grid (the modes whose mirror image the half spectrum leaves out count twice)
struct HalfMode { long long f0, f1, f2, q; int w; };

__device__ inline HalfMode half_mode(long long i, long long r0, long long r1, long long r2) {
    const long long h2 = r2 / 2 + 1;
    const long long i2 = i % h2, r = i / h2, i1 = r % r1, i0 = r / r1;
    HalfMode m;
    m.f0 = freq(i0, r0); m.f1 = freq(i1, r1); m.f2 = i2;
    m.q = m.f0 * m.f0 + m.f1 * m.f1 + i2 * i2;
    m.w = (i2 == 0 || (r2 % 2 == 0 && i2 == r2 / 2)) ? 1 : 2;
    return m;
}

[[maybe_unused]] int fail(const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    return nbe::api_fail(buf);
}

[[maybe_unused]] int launched(const char* what) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? 0 : fail("%s: launch failed: %s", what, hipGetErrorString(e));
}

[[maybe_unused]] int grid_for(long long n, int threads) {
    long long g = (n + threads - 1) / threads;
    return (int)(g < 1 ? 1 : g > 65536 ? 65536 : g);
}

// the grid of a catalogue kernel of 256 threads with one row a thread, capped by the caller's max_blocks
[[maybe_unused]] int fof_grid(long long count, int max_blocks) {
    const int g = grid_for(count, 256);
    return max_blocks > 0 && max_blocks < g ? max_blocks : g;
}

// The arguments of the catalogue entry points, one check per kind; `what` is the entry point's name.
[[maybe_unused]] bool count_ok(long long count) { return count >= 1 && count <= (1LL << 30); }

[[maybe_unused]] int check_count(const char* what, long long count) {
    return count_ok(count) ? 0 : fail("%s: bad particle count %lld", what, count);
}

[[maybe_unused]] int check_ncell(const char* what, int ncell) {
    return ncell >= 3 && ncell <= NBE_FOF_MAX_CELLS ? 0 : fail("%s: ncell %d not in 3 .. %d", what, ncell, NBE_FOF_MAX_CELLS);
}

[[maybe_unused]] int check_boxsize(const char* what, double boxsize) {
    return boxsize > 0.0 && std::isfinite(boxsize) ? 0 : fail("%s: bad boxsize %g", what, boxsize);
}

// thresholds[0 .. nbins] into *bins, and *s = isqrt of the last: they increase strictly from -1 or more, and the cells are
// at least s + 1 units wide (the adjacency argument of nbe_catalog.h): ncell (s + 1) <= 2^30
[[maybe_unused]] int check_thresholds(const char* what, const int64_t* thresholds, int nbins, int ncell, nbe::PairBins* bins,
                                      int* s) {
    for (int b = 0; b <= nbins; ++b) {
        bins->T[b] = thresholds[b];
        if (b ? thresholds[b] <= thresholds[b - 1] : thresholds[0] < -1)
            return fail("%s: the thresholds must increase strictly from -1 or more", what);
    }
    const long long room = (1LL << nbe::kCoordBits) / ncell - 1, top = bins->T[nbins];
    if (top < 0 || top >= (room + 1) * (room + 1))
        return fail("%s: threshold %lld needs cells wider than 2^30 / %d", what, top, ncell);
    *s = (int)nbe::pair_isqrt(top);
    return 0;
}

}  // namespace
