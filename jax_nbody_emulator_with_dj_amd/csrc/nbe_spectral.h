// Pieces shared by the context-free entry points (nbe_density.hip, nbe_lpt.hip): how a mode of torch's row-major half
// spectrum is decoded, and how such an entry point reports an error and sizes a launch.  Each is written once, here.
#pragma once

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

}  // namespace
