// The emulator's input (include/nbe.h, "Input fields"): a linear density field brought to the particle grid and turned
// into the first-order LPT displacement, and the divergence of a vector field on the same grid.  Replaces
// resize_density_grid and its helpers (scripts/utils.py:186-234, :261-346, :349-425, :531-555, :590-591) and
// dj.evaluate_lpt_psi_at_a(n_order=1) (scripts/core.py:396-397); the divergence has no counterpart there.  The transforms
// are the caller's (rocFFT); these are the passes between them.  The last section draws the linear field itself from a
// seed and a tabulated P(k), or colours somebody else's white noise (scripts/core.py:263-302).  The second-order LPT
// section adds what DISCO-DJ's n_order=2 would: the Hessian of the potential, the quadratic source (the one kernel here
// that walks voxels, not rows) and the displacement of both orders in one pass.  No context: no weights.
//
// Every other kernel walks rows: a (64, 4) workgroup takes four rows (i0, i1) of the destination at a time, decodes the row
// once (the only 64-bit division) and strides its 64 lanes along the contiguous axis, so that a wave-instruction reads
// and writes one run of a row.  Factors are formed in float64 and every output word is rounded to float32 once.  No LDS,
// no atomics: every destination word has one writer, so the results do not depend on the launch geometry.
//
// Spectra are torch's row-major half spectra (n, n, n/2+1) complex64.  Wave vectors are integers m, k = 2 pi m / L; axis
// position i holds m = freq(i, n) (nbe_spectral.h), so an even axis stores its Nyquist row as +n/2.

#include "../../include/nbe.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace {

constexpr int kLanes = 64;              // along the contiguous axis
constexpr int kRows = 4;                // rows per workgroup
constexpr double kPi = 3.141592653589793;

#define NBE_FOR_ROWS(r, rows) \
    for (long long r = blockIdx.x * (long long)kRows + threadIdx.y; r < (rows); r += (long long)gridDim.x * kRows)

// ---- first-order LPT ---------------------------------------------------------------------------------------------------

// psi_c = scale i k_c / |k|^2 delta = i c m_c / |m|^2 delta with c = scale L / (2 pi); i (x + i y) = -y + i x
__global__ __launch_bounds__(kLanes * kRows) void zeldovich_kernel(const float2* __restrict__ delta,
                                                                   float2* __restrict__ psi, long long n, double c) {
    const long long h = n / 2 + 1, rows = n * n, plane = rows * h;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;          // the position of a row without a sign
    NBE_FOR_ROWS(r, rows) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const long long m0 = freq(i0, n), m1 = freq(i1, n), q01 = m0 * m0 + m1 * m1;
        const double c0 = i0 == nyq ? 0.0 : c * (double)m0, c1 = i1 == nyq ? 0.0 : c * (double)m1;
        const float2* src = delta + r * h;
        float2* dst = psi + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const long long q = q01 + i2 * i2;
            const double inv = q ? 1.0 / (double)q : 0.0;
            const double f0 = c0 * inv, f1 = c1 * inv, f2 = i2 == nyq ? 0.0 : c * (double)i2 * inv;
            const float2 v = src[i2];
            dst[i2] = make_float2((float)(-f0 * v.y), (float)(f0 * v.x));
            dst[plane + i2] = make_float2((float)(-f1 * v.y), (float)(f1 * v.x));
            dst[2 * plane + i2] = make_float2((float)(-f2 * v.y), (float)(f2 * v.x));
        }
    }
}

// theta = div v: theta_k = i (2 pi / L) ((m_0 v_0 + m_1 v_1) + m_2 v_2), with component c left out on its own Nyquist row
// as zeldovich_kernel leaves it out.  The products of an integer below 2^11 and a float32 are exact in float64.
__global__ __launch_bounds__(kLanes * kRows) void divergence_kernel(const float2* __restrict__ v,
                                                                    float2* __restrict__ theta, long long n, double kf) {
    const long long h = n / 2 + 1, rows = n * n, plane = rows * h;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;
    NBE_FOR_ROWS(r, rows) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const double c0 = i0 == nyq ? 0.0 : (double)freq(i0, n), c1 = i1 == nyq ? 0.0 : (double)freq(i1, n);
        const float2* src = v + r * h;
        float2* dst = theta + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const double c2 = i2 == nyq ? 0.0 : (double)i2;
            const float2 v0 = src[i2], v1 = src[plane + i2], v2 = src[2 * plane + i2];
            const double re = (c0 * v0.x + c1 * v1.x) + c2 * v2.x, im = (c0 * v0.y + c1 * v1.y) + c2 * v2.y;
            dst[i2] = make_float2((float)(-kf * im), (float)(kf * re));
        }
    }
}

// ---- second-order LPT ------------------------------------------------------------------------------------------------------

// The pairs (i, j) of the Hessian's components 0 .. 5: the diagonal first, then (0,1), (0,2), (1,2)
constexpr int kPairs = NBE_LPT2_COMPONENTS;

// phi,ij = d_i d_j / |m|^2 delta with nabla^2 phi = delta: d_c = m_c, or 0 on the row |m_c| = n/2 of an even n, which is
// zeldovich_kernel's derivative applied once per factor.  Components first .. first + count - 1 go to out[0 .. count - 1];
// the six factors are formed for every mode and the loop over them is unrolled, so that they stay in registers.
__global__ __launch_bounds__(kLanes * kRows) void lpt2_hessian_kernel(const float2* __restrict__ delta,
                                                                      float2* __restrict__ out, long long n, int first,
                                                                      int count) {
    const long long h = n / 2 + 1, rows = n * n, plane = rows * h;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;
    NBE_FOR_ROWS(r, rows) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const long long m0 = freq(i0, n), m1 = freq(i1, n), q01 = m0 * m0 + m1 * m1;
        const long long d0 = i0 == nyq ? 0 : m0, d1 = i1 == nyq ? 0 : m1;
        const float2* src = delta + r * h;
        float2* dst = out + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const long long q = q01 + i2 * i2, d2 = i2 == nyq ? 0 : i2;
            const long long num[kPairs] = {d0 * d0, d1 * d1, d2 * d2, d0 * d1, d0 * d2, d1 * d2};
            const float2 v = src[i2];
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                if (p < first || p >= first + count) continue;
                const double f = q ? (double)num[p] / (double)q : 0.0;
                dst[(p - first) * plane + i2] = make_float2((float)(f * v.x), (float)(f * v.y));
            }
        }
    }
}

// S = ((h0 h1 + h0 h2) + h1 h2) - ((h3^2 + h4^2) + h5^2) in float64, rounded once.  The product of two float32 is exact
// in float64, so a product fused into the add that follows it gives the same bits.
__device__ inline float lpt2_source_word(float h0, float h1, float h2, float h3, float h4, float h5) {
    const double a0 = h0, a1 = h1, a2 = h2, a3 = h3, a4 = h4, a5 = h5;
    return (float)(((a0 * a1 + a0 * a2) + a1 * a2) - ((a3 * a3 + a4 * a4) + a5 * a5));
}

constexpr int kVoxelThreads = 256;      // the real-space pass: a grid-stride loop over the voxels
constexpr int kVoxelBlocks = 2048;      // 8 workgroups for each of 256 compute units; the loop takes the rest

// One voxel a lane and step.  The path for an odd n, where component c starts at byte 4 c n^3, which 16 does not divide.
__global__ __launch_bounds__(kVoxelThreads) void lpt2_source_kernel(const float* __restrict__ hess,
                                                                    float* __restrict__ out, long long cells) {
    const long long step = (long long)gridDim.x * kVoxelThreads;
    for (long long i = blockIdx.x * (long long)kVoxelThreads + threadIdx.x; i < cells; i += step)
        out[i] = lpt2_source_word(hess[i], hess[cells + i], hess[2 * cells + i], hess[3 * cells + i],
                                  hess[4 * cells + i], hess[5 * cells + i]);
}

// Four voxels a lane and step, 16 bytes per access: for cells % 4 == 0 and 16-byte aligned pointers (an even n)
__global__ __launch_bounds__(kVoxelThreads) void lpt2_source4_kernel(const float4* __restrict__ hess,
                                                                     float4* __restrict__ out, long long quads) {
    const long long step = (long long)gridDim.x * kVoxelThreads;
    for (long long i = blockIdx.x * (long long)kVoxelThreads + threadIdx.x; i < quads; i += step) {
        const float4 h0 = hess[i], h1 = hess[quads + i], h2 = hess[2 * quads + i], h3 = hess[3 * quads + i],
                     h4 = hess[4 * quads + i], h5 = hess[5 * quads + i];
        out[i] = make_float4(lpt2_source_word(h0.x, h1.x, h2.x, h3.x, h4.x, h5.x),
                             lpt2_source_word(h0.y, h1.y, h2.y, h3.y, h4.y, h5.y),
                             lpt2_source_word(h0.z, h1.z, h2.z, h3.z, h4.z, h5.z),
                             lpt2_source_word(h0.w, h1.w, h2.w, h3.w, h4.w, h5.w));
    }
}

// psi_c = i c d_c / |m|^2 (a delta + b S) with c = L / (2 pi): zeldovich_kernel on the sum of two spectra, which saves
// the pass that would add them and the three transforms of a second displacement
__global__ __launch_bounds__(kLanes * kRows) void lpt2_displacement_kernel(const float2* __restrict__ delta,
                                                                           const float2* __restrict__ source,
                                                                           float2* __restrict__ psi, long long n, double c,
                                                                           double a, double b) {
    const long long h = n / 2 + 1, rows = n * n, plane = rows * h;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;
    NBE_FOR_ROWS(r, rows) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const long long m0 = freq(i0, n), m1 = freq(i1, n), q01 = m0 * m0 + m1 * m1;
        const double c0 = i0 == nyq ? 0.0 : c * (double)m0, c1 = i1 == nyq ? 0.0 : c * (double)m1;
        const float2* sd = delta + r * h;
        const float2* ss = source + r * h;
        float2* dst = psi + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const long long q = q01 + i2 * i2;
            const double inv = q ? 1.0 / (double)q : 0.0;
            const double f0 = c0 * inv, f1 = c1 * inv, f2 = i2 == nyq ? 0.0 : c * (double)i2 * inv;
            const float2 v = sd[i2], s = ss[i2];
            const double x = a * v.x + b * s.x, y = a * v.y + b * s.y;
            dst[i2] = make_float2((float)(-f0 * y), (float)(f0 * x));
            dst[plane + i2] = make_float2((float)(-f1 * y), (float)(f1 * x));
            dst[2 * plane + i2] = make_float2((float)(-f2 * y), (float)(f2 * x));
        }
    }
}

// ---- Fourier interpolation -----------------------------------------------------------------------------------------------

// The source wave numbers that feed destination wave number m on one axis: none (cnt 0) beyond the source's band, one
// (with weight 1/2 on an even source's Nyquist row when upsampling, which splits that row evenly onto +-n_in/2), or both
// signs for a destination Nyquist row when downsampling.
struct AxisTerms { int cnt; long long m[2]; double w; };

__device__ inline AxisTerms axis_terms(long long m, long long n_in, long long n_out) {
    AxisTerms t;
    t.cnt = 1; t.m[0] = m; t.m[1] = -m; t.w = 1.0;
    const long long a = m < 0 ? -m : m;
    if (n_out > n_in) {
        if (2 * a > n_in) t.cnt = 0;
        else if (2 * a == n_in) t.w = 0.5;
    } else if (n_out < n_in && 2 * a == n_out) {
        t.cnt = 2;
    }
    return t;
}

// Where the terms of a destination row (m0, m1) start in the source half spectrum: pos for a source wave number along
// axis 2 that is >= 0, neg for a negative one, which is the conjugate of the stored mode at (-a, -b, -c).
struct RowTerms { AxisTerms t0, t1; long long pos[2][2], neg[2][2]; long long q01; };

__device__ inline long long axis_index(long long m, long long n) { return m < 0 ? m + n : m; }

__device__ inline RowTerms row_terms(long long i0, long long i1, long long n_in, long long n_out) {
    const long long m0 = freq(i0, n_out), m1 = freq(i1, n_out), h_in = n_in / 2 + 1;
    RowTerms R;
    R.t0 = axis_terms(m0, n_in, n_out);
    R.t1 = axis_terms(m1, n_in, n_out);
    R.q01 = m0 * m0 + m1 * m1;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b) {
            const bool live = a < R.t0.cnt && b < R.t1.cnt;          // indices of dead terms are never formed
            const long long ma = live ? R.t0.m[a] : 0, mb = live ? R.t1.m[b] : 0;
            R.pos[a][b] = (axis_index(ma, n_in) * n_in + axis_index(mb, n_in)) * h_in;
            R.neg[a][b] = (axis_index(-ma, n_in) * n_in + axis_index(-mb, n_in)) * h_in;
        }
    return R;
}

// Destination mode (row R, i2) of the resized spectrum: scale * w * the sum of its source terms, added in float64 in the
// fixed order (axis 0, axis 1, axis 2) and multiplied once, so that no product can be fused into a sum and every kernel
// that calls this gets the same bits.
__device__ inline float2 resized_mode(const float2* __restrict__ src, const RowTerms& R, long long i2, long long n_in,
                                      long long n_out, double scale, int sphere) {
    const AxisTerms t2 = axis_terms(i2, n_in, n_out);
    const long long q = R.q01 + i2 * i2;
    if (R.t0.cnt == 0 || R.t1.cnt == 0 || t2.cnt == 0 || (sphere && 4 * q > n_in * n_in)) return make_float2(0.0f, 0.0f);
    double re = 0.0, im = 0.0;
#pragma unroll                                              // constant indices keep the terms in registers
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                if (a >= R.t0.cnt || b >= R.t1.cnt || c >= t2.cnt) continue;
                const long long mc = t2.m[c];
                const float2 v = mc >= 0 ? src[R.pos[a][b] + mc] : src[R.neg[a][b] - mc];
                re += (double)v.x;
                im += mc >= 0 ? (double)v.y : -(double)v.y;
            }
    const double f = scale * (R.t0.w * R.t1.w * t2.w);
    return make_float2((float)(re * f), (float)(im * f));
}

__global__ __launch_bounds__(kLanes * kRows) void spectrum_resize_kernel(const float2* __restrict__ src, long long n_in,
                                                                         float2* __restrict__ dst, long long n_out,
                                                                         double scale, int sphere) {
    const long long h = n_out / 2 + 1;
    NBE_FOR_ROWS(r, n_out * n_out) {
        const long long i0 = r / n_out, i1 = r - i0 * n_out;
        const RowTerms R = row_terms(i0, i1, n_in, n_out);
        float2* out = dst + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes)
            out[i2] = resized_mode(src, R, i2, n_in, n_out, scale, sphere);
    }
}

// ---- mode injection --------------------------------------------------------------------------------------------------------

// Philox4x32-10 (Salmon et al. 2011): counter c, key (k0, k1)
__device__ inline void philox4x32_10(uint32_t c[4], uint32_t k0, uint32_t k1) {
    for (int round = 0; round < 10; ++round) {
        const uint64_t p0 = 0xD2511F53ull * c[0], p1 = 0xCD9E8D57ull * c[2];
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0; c[1] = (uint32_t)p1; c[2] = n2; c[3] = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
}

// A tabulated P(k) in device memory and its fitted log-log tail: carried by every argument block that evaluates it
struct PkTable {
    const double* k; const double* pk; int n;
    double tail_slope, tail_intercept;
};

struct InjectArgs {
    const float2* src; float2* dst;
    long long n_in, n_out;
    PkTable table;
    double kf;                  // 2 pi / L
    double amp;                 // n_out^3 / sqrt(L^3): sigma = amp sqrt(P)
    double scale;               // (n_out / n_in)^3
    uint32_t key0, key1;
};

// P(k): np.interp inside the table, pk[0] below it, the fitted power law above it, clamped at 0
__device__ inline double table_power(const PkTable& T, double k) {
    const double* kt = T.k;
    const double* pt = T.pk;
    const int last = T.n - 1;
    double p;
    if (k < kt[0]) p = pt[0];
    else if (k > kt[last]) p = exp(T.tail_intercept + T.tail_slope * log(k));
    else if (k == kt[last]) p = pt[last];
    else {
        int lo = 0, hi = last;                              // kt[lo] <= k < kt[hi]
        while (hi - lo > 1) {
            const int mid = (lo + hi) / 2;
            if (kt[mid] <= k) lo = mid; else hi = mid;
        }
        const double slope = (pt[lo + 1] - pt[lo]) / (kt[lo + 1] - kt[lo]);
        p = slope * (k - kt[lo]) + pt[lo];
    }
    return p > 0.0 ? p : 0.0;
}

// the two uniforms of a counter: U = (x + 1/2) 2^-32 from the first two words of Philox4x32-10
__device__ inline void philox_uniforms(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                       double* u1, double* u2) {
    uint32_t x[4] = {c0, c1, c2, c3};
    philox4x32_10(x, k0, k1);
    *u1 = ((double)x[0] + 0.5) * 0x1p-32;
    *u2 = ((double)x[1] + 0.5) * 0x1p-32;
}

__global__ __launch_bounds__(kLanes * kRows) void spectrum_inject_kernel(InjectArgs A) {
    const long long n = A.n_out, h = n / 2 + 1;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;
    NBE_FOR_ROWS(r, n * n) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const RowTerms R = row_terms(i0, i1, A.n_in, n);
        // on the planes that are their own mirror image, (i0, i1) and its mirror row form a pair: the smaller index draws
        const long long p0 = i0 ? n - i0 : 0, p1 = i1 ? n - i1 : 0, mirror = p0 * n + p1;
        float2* out = A.dst + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const long long q = R.q01 + i2 * i2;
            if (4 * q <= A.n_in * A.n_in) {
                out[i2] = resized_mode(A.src, R, i2, A.n_in, n, A.scale, 1);
                continue;
            }
            const bool paired = i2 == 0 || i2 == nyq;
            const bool second = paired && mirror < r, self = paired && mirror == r;
            double u1, u2, s, c;
            philox_uniforms((uint32_t)(second ? p0 : i0), (uint32_t)(second ? p1 : i1), (uint32_t)i2, 0u, A.key0, A.key1,
                            &u1, &u2);
            sincospi(2.0 * u2, &s, &c);
            const double sigma = A.amp * sqrt(table_power(A.table, A.kf * sqrt((double)q)));
            const double mag = sigma * sqrt(-2.0 * log(u1));
            if (self) {
                out[i2] = make_float2((float)(mag * c), 0.0f);
            } else {
                const double g = mag * 0.7071067811865476;
                out[i2] = make_float2((float)(g * c), (float)(second ? -(g * s) : g * s));
            }
        }
    }
}

// ---- the linear field from a seed ------------------------------------------------------------------------------------------

constexpr int kFixedAmplitude = NBE_IC_FIXED_AMPLITUDE, kInvertPhase = NBE_IC_INVERT_PHASE, kWhiteNoise = NBE_IC_WHITE_NOISE;

struct GaussianArgs {
    float2* dst;
    long long n;
    PkTable table;              // unused for white noise
    double kf;                  // 2 pi / L
    double amp;                 // scale n^3, or n^(3/2) for white noise
    double volume;              // L^3: sigma = amp sqrt(P / volume)
    uint32_t key0, key1;
    int flags;
};

// The whole half spectrum of a Gaussian field.  The pairing of spectrum_inject_kernel; the
// counter is the drawing row's signed wave vector and a last word of 1, so that a mode draws the same numbers on every mesh
// that holds it and never shares a counter with the injection.  Products only, so sigma for n and 2n, and with it every
// word, differ by exactly 8.
__global__ __launch_bounds__(kLanes * kRows) void gaussian_spectrum_kernel(GaussianArgs A) {
    const long long n = A.n, h = n / 2 + 1;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;
    const double sign = A.flags & kInvertPhase ? -1.0 : 1.0;
    NBE_FOR_ROWS(r, n * n) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const long long p0 = i0 ? n - i0 : 0, p1 = i1 ? n - i1 : 0, mirror = p0 * n + p1;
        const long long m0 = freq(i0, n), m1 = freq(i1, n), q01 = m0 * m0 + m1 * m1;
        const long long w0 = freq(p0, n), w1 = freq(p1, n);          // the mirror row's wave numbers
        float2* out = A.dst + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const long long q = q01 + i2 * i2;
            if (q == 0) {
                out[i2] = make_float2(0.0f, 0.0f);
                continue;
            }
            const bool paired = i2 == 0 || i2 == nyq;
            const bool second = paired && mirror < r, self = paired && mirror == r;
            double u1, u2, s, c;
            philox_uniforms((uint32_t)(int32_t)(second ? w0 : m0), (uint32_t)(int32_t)(second ? w1 : m1), (uint32_t)i2, 1u,
                            A.key0, A.key1, &u1, &u2);
            sincospi(2.0 * u2, &s, &c);
            const double sigma = A.flags & kWhiteNoise ? A.amp
                                                       : A.amp * sqrt(table_power(A.table, A.kf * sqrt((double)q)) / A.volume);
            if (A.flags & kFixedAmplitude) {
                if (self) out[i2] = make_float2((float)(sign * (c >= 0.0 ? sigma : -sigma)), 0.0f);
                else out[i2] = make_float2((float)(sign * (sigma * c)), (float)(sign * (second ? -(sigma * s) : sigma * s)));
                continue;
            }
            const double mag = sigma * sqrt(-2.0 * log(u1));
            if (self) {
                out[i2] = make_float2((float)(sign * (mag * c)), 0.0f);
            } else {
                const double g = mag * 0.7071067811865476;
                out[i2] = make_float2((float)(sign * (g * c)), (float)(sign * (second ? -(g * s) : g * s)));
            }
        }
    }
}

// in place: the spectrum of a white-noise field times amp sqrt(n^3 P(|k|) / L^3), 0 at m = 0
__global__ __launch_bounds__(kLanes * kRows) void spectrum_colour_kernel(float2* __restrict__ f, long long n, PkTable T,
                                                                         double kf, double amp, double cells,
                                                                         double volume) {
    const long long h = n / 2 + 1;
    NBE_FOR_ROWS(r, n * n) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const long long m0 = freq(i0, n), m1 = freq(i1, n), q01 = m0 * m0 + m1 * m1;
        float2* row = f + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const long long q = q01 + i2 * i2;
            if (q == 0) {
                row[i2] = make_float2(0.0f, 0.0f);
                continue;
            }
            const double w = amp * sqrt(cells * table_power(T, kf * sqrt((double)q)) / volume);
            const float2 v = row[i2];
            row[i2] = make_float2((float)(v.x * w), (float)(v.y * w));
        }
    }
}

// ---- Gaussian filter, block average, trilinear interpolation ---------------------------------------------------------------

// in place: exp(-|k|^2 sigma^2 / 2) = exp(a |m|^2), a = -2 pi^2 (sigma / L)^2
__global__ __launch_bounds__(kLanes * kRows) void gaussian_filter_kernel(float2* __restrict__ f, long long n, double a) {
    const long long h = n / 2 + 1;
    NBE_FOR_ROWS(r, n * n) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const long long m0 = freq(i0, n), m1 = freq(i1, n), q01 = m0 * m0 + m1 * m1;
        float2* row = f + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const double w = exp(a * (double)(q01 + i2 * i2));
            const float2 v = row[i2];
            row[i2] = make_float2((float)(v.x * w), (float)(v.y * w));
        }
    }
}

// mean of each ratio^3 block, summed in float64 in the order (a, b, c) of the block's axes
__global__ __launch_bounds__(kLanes * kRows) void block_average_kernel(const float* __restrict__ src, long long n_in,
                                                                       float* __restrict__ dst, long long n_out) {
    const long long ratio = n_in / n_out;
    const double cells = (double)(ratio * ratio * ratio);
    NBE_FOR_ROWS(r, n_out * n_out) {
        const long long i0 = r / n_out, i1 = r - i0 * n_out;
        const float* block = src + (i0 * ratio * n_in + i1 * ratio) * n_in;
        float* out = dst + r * n_out;
        for (long long i2 = threadIdx.x; i2 < n_out; i2 += kLanes) {
            double sum = 0.0;
            for (long long a = 0; a < ratio; ++a)
                for (long long b = 0; b < ratio; ++b) {
                    const float* p = block + (a * n_in + b) * n_in + i2 * ratio;
                    if (ratio == 2) {                       // the rows of a pair of cells: one 8-byte load per lane
                        const float2 v = *reinterpret_cast<const float2*>(p);
                        sum += (double)v.x;
                        sum += (double)v.y;
                    } else {
                        for (long long c = 0; c < ratio; ++c) sum += (double)p[c];
                    }
                }
            out[i2] = (float)(sum / cells);
        }
    }
}

// periodic trilinear interpolation at the fine nodes i n_in / n_out (an integer ratio): nested lerps in float64, so that
// a fine node on a coarse node (t = 0) returns the coarse value itself
__device__ inline double lerp(double a, double b, double t) { return (1.0 - t) * a + t * b; }

__global__ __launch_bounds__(kLanes * kRows) void trilinear_kernel(const float* __restrict__ src, long long n_in,
                                                                   float* __restrict__ dst, long long n_out) {
    const int ratio = (int)(n_out / n_in), ni = (int)n_in;
    const double step = 1.0 / (double)ratio;
    NBE_FOR_ROWS(r, n_out * n_out) {
        const long long i0 = r / n_out, i1 = r - i0 * n_out;
        const long long j0 = i0 / ratio, j1 = i1 / ratio;
        const double t0 = (double)(i0 - j0 * ratio) * step, t1 = (double)(i1 - j1 * ratio) * step;
        const long long j0p = j0 + 1 == n_in ? 0 : j0 + 1, j1p = j1 + 1 == n_in ? 0 : j1 + 1;
        const float* r00 = src + (j0 * n_in + j1) * n_in;
        const float* r01 = src + (j0 * n_in + j1p) * n_in;
        const float* r10 = src + (j0p * n_in + j1) * n_in;
        const float* r11 = src + (j0p * n_in + j1p) * n_in;
        float* out = dst + r * n_out;
        for (int i2 = threadIdx.x; i2 < (int)n_out; i2 += kLanes) {
            const int j2 = i2 / ratio, j2p = j2 + 1 == ni ? 0 : j2 + 1;
            const double t2 = (double)(i2 - j2 * ratio) * step;
            const double a = lerp(lerp((double)r00[j2], (double)r00[j2p], t2), lerp((double)r01[j2], (double)r01[j2p], t2), t1);
            const double b = lerp(lerp((double)r10[j2], (double)r10[j2p], t2), lerp((double)r11[j2], (double)r11[j2p], t2), t1);
            out[i2] = (float)lerp(a, b, t0);
        }
    }
}

// ---- velocity shear -------------------------------------------------------------------------------

// Sigma_ij = -scale (d_i v_j + d_j v_i) / 2 of a vector mesh (the V-web's tensor, Hoffman et al. 2012, where scale = 1 / H0),
// in lpt2_hessian_kernel's pair order and pieces and with divergence_kernel's derivative i kf d_c, d_c = 0 on the Nyquist
// row of an even n: out = i f (d_i v_j + d_j v_i) / 2 with f = -scale kf.  The products of an integer below 2^11 and a
// float32 are exact in float64, so the bracket is rounded once, halving is exact, and a diagonal component is d_i v_i.
// (After every other kernel of this file, so that none of them moves in the code object.)
__global__ __launch_bounds__(kLanes * kRows) void shear_kernel(const float2* __restrict__ v, float2* __restrict__ out,
                                                               long long n, double f, int first, int count) {
    const long long h = n / 2 + 1, rows = n * n, plane = rows * h;
    const long long nyq = n % 2 == 0 ? n / 2 : -1;
    NBE_FOR_ROWS(r, rows) {
        const long long i0 = r / n, i1 = r - i0 * n;
        const double d0 = i0 == nyq ? 0.0 : (double)freq(i0, n), d1 = i1 == nyq ? 0.0 : (double)freq(i1, n);
        const float2* src = v + r * h;
        float2* dst = out + r * h;
        for (long long i2 = threadIdx.x; i2 < h; i2 += kLanes) {
            const double d2 = i2 == nyq ? 0.0 : (double)i2;
            const float2 v0 = src[i2], v1 = src[plane + i2], v2 = src[2 * plane + i2];
            const double re[kPairs] = {d0 * v0.x, d1 * v1.x, d2 * v2.x, 0.5 * (d0 * v1.x + d1 * v0.x),
                                       0.5 * (d0 * v2.x + d2 * v0.x), 0.5 * (d1 * v2.x + d2 * v1.x)};
            const double im[kPairs] = {d0 * v0.y, d1 * v1.y, d2 * v2.y, 0.5 * (d0 * v1.y + d1 * v0.y),
                                       0.5 * (d0 * v2.y + d2 * v0.y), 0.5 * (d1 * v2.y + d2 * v1.y)};
#pragma unroll
            for (int p = 0; p < kPairs; ++p) {
                if (p < first || p >= first + count) continue;
                dst[(p - first) * plane + i2] = make_float2((float)(-f * im[p]), (float)(f * re[p]));
            }
        }
    }
}

bool size_ok(int64_t n) { return n >= NBE_LPT_MIN_N && n <= NBE_LPT_MAX_N; }

dim3 row_grid(long long n) { return dim3((unsigned)grid_for(n * n, kRows)); }

const dim3 kBlock(kLanes, kRows);

double cube(double x) { return x * x * x; }

// a grid of at most max_blocks workgroups (max_blocks <= 0: as it is); the kernels loop over what is left
dim3 capped(dim3 grid, int max_blocks) {
    if (max_blocks > 0 && grid.x > (unsigned)max_blocks) grid.x = (unsigned)max_blocks;
    return grid;
}

// whether the byte ranges [a, a + abytes) and [b, b + bbytes) share a byte
bool overlap(const void* a, long long abytes, const void* b, long long bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

}  // namespace

extern "C" {

int nbe_zeldovich_spectrum(const void* spectrum, int64_t n, double boxsize, double scale, void* psi_spectrum,
                           void* stream) {
    if (!spectrum || !psi_spectrum) return fail("nbe_zeldovich_spectrum: NULL argument");
    if (!size_ok(n)) return fail("nbe_zeldovich_spectrum: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize) || !std::isfinite(scale))
        return fail("nbe_zeldovich_spectrum: bad boxsize %g or scale %g", boxsize, scale);
    hipLaunchKernelGGL(zeldovich_kernel, row_grid(n), kBlock, 0, (hipStream_t)stream, (const float2*)spectrum,
                       (float2*)psi_spectrum, (long long)n, scale * boxsize / (2.0 * kPi));
    return launched("nbe_zeldovich_spectrum");
}

int nbe_divergence_spectrum(const void* spectra, int64_t n, double boxsize, void* out, void* stream) {
    if (!spectra || !out || spectra == out) return fail("nbe_divergence_spectrum: NULL or aliased argument");
    if (!size_ok(n)) return fail("nbe_divergence_spectrum: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize)) return fail("nbe_divergence_spectrum: bad boxsize %g", boxsize);
    hipLaunchKernelGGL(divergence_kernel, row_grid(n), kBlock, 0, (hipStream_t)stream, (const float2*)spectra,
                       (float2*)out, (long long)n, 2.0 * kPi / boxsize);
    return launched("nbe_divergence_spectrum");
}

int nbe_lpt2_hessian_spectrum(const void* spectrum, int64_t n, int first, int count, void* out, int max_blocks,
                              void* stream) {
    if (!spectrum || !out) return fail("nbe_lpt2_hessian_spectrum: NULL argument");
    if (!size_ok(n)) return fail("nbe_lpt2_hessian_spectrum: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (first < 0 || count < 1 || first > kPairs - count)
        return fail("nbe_lpt2_hessian_spectrum: components %d .. %d not in 0 .. %d", first, first + count - 1, kPairs - 1);
    const long long words = 8 * n * n * (n / 2 + 1);
    if (overlap(spectrum, words, out, count * words)) return fail("nbe_lpt2_hessian_spectrum: out aliases spectrum");
    hipLaunchKernelGGL(lpt2_hessian_kernel, capped(row_grid(n), max_blocks), kBlock, 0, (hipStream_t)stream,
                       (const float2*)spectrum, (float2*)out, (long long)n, first, count);
    return launched("nbe_lpt2_hessian_spectrum");
}

int nbe_shear_spectrum(const void* spectra, int64_t n, double boxsize, double scale, int first, int count, void* out,
                       int max_blocks, void* stream) {
    if (!spectra || !out) return fail("nbe_shear_spectrum: NULL argument");
    if (!size_ok(n)) return fail("nbe_shear_spectrum: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize) || !std::isfinite(scale))
        return fail("nbe_shear_spectrum: bad boxsize %g or scale %g", boxsize, scale);
    if (first < 0 || count < 1 || first > kPairs - count)
        return fail("nbe_shear_spectrum: components %d .. %d not in 0 .. %d", first, first + count - 1, kPairs - 1);
    const long long words = 8 * n * n * (n / 2 + 1);
    if (overlap(spectra, 3 * words, out, count * words)) return fail("nbe_shear_spectrum: out aliases spectra");
    hipLaunchKernelGGL(shear_kernel, capped(row_grid(n), max_blocks), kBlock, 0, (hipStream_t)stream,
                       (const float2*)spectra, (float2*)out, (long long)n, -scale * (2.0 * kPi / boxsize), first, count);
    return launched("nbe_shear_spectrum");
}

int nbe_lpt2_source(const void* hess, int64_t n, void* out, int max_blocks, void* stream) {
    if (!hess || !out) return fail("nbe_lpt2_source: NULL argument");
    if (!size_ok(n)) return fail("nbe_lpt2_source: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    const long long cells = n * n * n;
    if (overlap(hess, kPairs * 4 * cells, out, 4 * cells)) return fail("nbe_lpt2_source: out aliases hess");
    const bool wide = cells % 4 == 0 && ((uintptr_t)hess | (uintptr_t)out) % 16 == 0;
    const long long items = wide ? cells / 4 : cells;
    long long blocks = (items + kVoxelThreads - 1) / kVoxelThreads;
    if (blocks > kVoxelBlocks) blocks = kVoxelBlocks;
    const dim3 grid = capped(dim3((unsigned)blocks), max_blocks);
    if (wide)
        hipLaunchKernelGGL(lpt2_source4_kernel, grid, dim3(kVoxelThreads), 0, (hipStream_t)stream, (const float4*)hess,
                           (float4*)out, items);
    else
        hipLaunchKernelGGL(lpt2_source_kernel, grid, dim3(kVoxelThreads), 0, (hipStream_t)stream, (const float*)hess,
                           (float*)out, items);
    return launched("nbe_lpt2_source");
}

int nbe_lpt2_spectrum(const void* delta_k, const void* source_k, int64_t n, double boxsize, double scale1, double scale2,
                      void* psi_spectrum, int max_blocks, void* stream) {
    if (!delta_k || !source_k || !psi_spectrum) return fail("nbe_lpt2_spectrum: NULL argument");
    if (!size_ok(n)) return fail("nbe_lpt2_spectrum: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize) || !std::isfinite(scale1) || !std::isfinite(scale2))
        return fail("nbe_lpt2_spectrum: bad boxsize %g or scales %g, %g", boxsize, scale1, scale2);
    const long long words = 8 * n * n * (n / 2 + 1);
    if (overlap(delta_k, words, psi_spectrum, 3 * words) || overlap(source_k, words, psi_spectrum, 3 * words))
        return fail("nbe_lpt2_spectrum: psi_spectrum aliases an input");
    hipLaunchKernelGGL(lpt2_displacement_kernel, capped(row_grid(n), max_blocks), kBlock, 0, (hipStream_t)stream,
                       (const float2*)delta_k, (const float2*)source_k, (float2*)psi_spectrum, (long long)n,
                       boxsize / (2.0 * kPi), scale1, scale2);
    return launched("nbe_lpt2_spectrum");
}

int nbe_spectrum_resize(const void* src, int64_t n_in, void* dst, int64_t n_out, int sphere, void* stream) {
    if (!src || !dst || src == dst) return fail("nbe_spectrum_resize: NULL or aliased argument");
    if (!size_ok(n_in) || !size_ok(n_out))
        return fail("nbe_spectrum_resize: sizes %lld -> %lld not in %d .. %d", (long long)n_in, (long long)n_out,
                    NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    hipLaunchKernelGGL(spectrum_resize_kernel, row_grid(n_out), kBlock, 0, (hipStream_t)stream, (const float2*)src,
                       (long long)n_in, (float2*)dst, (long long)n_out, cube((double)n_out / (double)n_in), sphere != 0);
    return launched("nbe_spectrum_resize");
}

int nbe_spectrum_inject(const void* src, int64_t n_in, void* dst, int64_t n_out, const void* k_table,
                        const void* pk_table, int ntable, double tail_slope, double tail_intercept, double boxsize,
                        uint64_t seed, void* stream) {
    if (!src || !dst || src == dst || !k_table || !pk_table) return fail("nbe_spectrum_inject: NULL or aliased argument");
    if (!size_ok(n_in) || !size_ok(n_out) || n_out < n_in)
        return fail("nbe_spectrum_inject: sizes %lld -> %lld not in %d .. %d, or not upwards", (long long)n_in,
                    (long long)n_out, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (ntable < 2) return fail("nbe_spectrum_inject: a table of %d points (at least 2)", ntable);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize) || !std::isfinite(tail_slope) || !std::isfinite(tail_intercept))
        return fail("nbe_spectrum_inject: bad boxsize %g or tail (%g, %g)", boxsize, tail_slope, tail_intercept);
    InjectArgs A;
    A.src = (const float2*)src; A.dst = (float2*)dst;
    A.n_in = n_in; A.n_out = n_out;
    A.table = PkTable{(const double*)k_table, (const double*)pk_table, ntable, tail_slope, tail_intercept};
    A.kf = 2.0 * kPi / boxsize;
    A.amp = cube((double)n_out) / sqrt(cube(boxsize));
    A.scale = cube((double)n_out / (double)n_in);
    A.key0 = (uint32_t)seed; A.key1 = (uint32_t)(seed >> 32);
    hipLaunchKernelGGL(spectrum_inject_kernel, row_grid(n_out), kBlock, 0, (hipStream_t)stream, A);
    return launched("nbe_spectrum_inject");
}

int nbe_gaussian_spectrum(void* dst, int64_t n, const void* k_table, const void* pk_table, int ntable,
                          double tail_slope, double tail_intercept, double boxsize, double scale, uint64_t seed, int flags,
                          int max_blocks, void* stream) {
    const bool white = flags & kWhiteNoise;
    if (!dst || (!white && (!k_table || !pk_table))) return fail("nbe_gaussian_spectrum: NULL argument");
    if (!size_ok(n)) return fail("nbe_gaussian_spectrum: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (flags & ~(kFixedAmplitude | kInvertPhase | kWhiteNoise)) return fail("nbe_gaussian_spectrum: unknown flags %d", flags);
    if (!white) {
        if (ntable < 2) return fail("nbe_gaussian_spectrum: a table of %d points (at least 2)", ntable);
        if (!(boxsize > 0.0) || !std::isfinite(boxsize) || !(scale > 0.0) || !std::isfinite(scale) ||
            !std::isfinite(tail_slope) || !std::isfinite(tail_intercept))
            return fail("nbe_gaussian_spectrum: bad boxsize %g, scale %g or tail (%g, %g)", boxsize, scale, tail_slope,
                        tail_intercept);
    }
    GaussianArgs A;
    A.dst = (float2*)dst; A.n = n; A.flags = flags;
    A.key0 = (uint32_t)seed; A.key1 = (uint32_t)(seed >> 32);
    if (white) {
        A.table = PkTable{nullptr, nullptr, 0, 0.0, 0.0};
        A.kf = 0.0; A.volume = 1.0;
        A.amp = sqrt(cube((double)n));
    } else {
        A.table = PkTable{(const double*)k_table, (const double*)pk_table, ntable, tail_slope, tail_intercept};
        A.kf = 2.0 * kPi / boxsize; A.volume = cube(boxsize);
        A.amp = scale * cube((double)n);
    }
    dim3 grid = row_grid(n);
    if (max_blocks > 0 && grid.x > (unsigned)max_blocks) grid.x = (unsigned)max_blocks;
    hipLaunchKernelGGL(gaussian_spectrum_kernel, grid, kBlock, 0, (hipStream_t)stream, A);
    return launched("nbe_gaussian_spectrum");
}

int nbe_spectrum_colour(void* spectrum, int64_t n, const void* k_table, const void* pk_table, int ntable,
                        double tail_slope, double tail_intercept, double boxsize, double scale, void* stream) {
    if (!spectrum || !k_table || !pk_table) return fail("nbe_spectrum_colour: NULL argument");
    if (!size_ok(n)) return fail("nbe_spectrum_colour: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (ntable < 2) return fail("nbe_spectrum_colour: a table of %d points (at least 2)", ntable);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize) || !(scale > 0.0) || !std::isfinite(scale) ||
        !std::isfinite(tail_slope) || !std::isfinite(tail_intercept))
        return fail("nbe_spectrum_colour: bad boxsize %g, scale %g or tail (%g, %g)", boxsize, scale, tail_slope,
                    tail_intercept);
    const PkTable T{(const double*)k_table, (const double*)pk_table, ntable, tail_slope, tail_intercept};
    hipLaunchKernelGGL(spectrum_colour_kernel, row_grid(n), kBlock, 0, (hipStream_t)stream, (float2*)spectrum, (long long)n,
                       T, 2.0 * kPi / boxsize, scale, cube((double)n), cube(boxsize));
    return launched("nbe_spectrum_colour");
}

int nbe_gaussian_filter(void* spectrum, int64_t n, double sigma_over_L, void* stream) {
    if (!spectrum) return fail("nbe_gaussian_filter: NULL argument");
    if (!size_ok(n)) return fail("nbe_gaussian_filter: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (!(sigma_over_L >= 0.0) || !std::isfinite(sigma_over_L))
        return fail("nbe_gaussian_filter: bad sigma / L %g", sigma_over_L);
    hipLaunchKernelGGL(gaussian_filter_kernel, row_grid(n), kBlock, 0, (hipStream_t)stream, (float2*)spectrum,
                       (long long)n, -2.0 * kPi * kPi * sigma_over_L * sigma_over_L);
    return launched("nbe_gaussian_filter");
}

int nbe_block_average(const void* src, int64_t n_in, void* dst, int64_t n_out, void* stream) {
    if (!src || !dst || src == dst) return fail("nbe_block_average: NULL or aliased argument");
    if (!size_ok(n_in) || n_out < 1 || n_out > n_in || n_in % n_out)
        return fail("nbe_block_average: %lld -> %lld is not a division by an integer (sizes up to %d)", (long long)n_in,
                    (long long)n_out, NBE_LPT_MAX_N);
    hipLaunchKernelGGL(block_average_kernel, row_grid(n_out), kBlock, 0, (hipStream_t)stream, (const float*)src,
                       (long long)n_in, (float*)dst, (long long)n_out);
    return launched("nbe_block_average");
}

int nbe_trilinear_upsample(const void* src, int64_t n_in, void* dst, int64_t n_out, void* stream) {
    if (!src || !dst || src == dst) return fail("nbe_trilinear_upsample: NULL or aliased argument");
    if (!size_ok(n_out) || n_in < 1 || n_in > n_out || n_out % n_in)
        return fail("nbe_trilinear_upsample: %lld -> %lld is not a multiplication by an integer (sizes up to %d)",
                    (long long)n_in, (long long)n_out, NBE_LPT_MAX_N);
    hipLaunchKernelGGL(trilinear_kernel, row_grid(n_out), kBlock, 0, (hipStream_t)stream, (const float*)src,
                       (long long)n_in, (float*)dst, (long long)n_out);
    return launched("nbe_trilinear_upsample");
}

}  // extern "C"
