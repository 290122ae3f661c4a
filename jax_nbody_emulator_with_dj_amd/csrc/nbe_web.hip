// Cosmic-web classification (include/nbe.h, "Cosmic web"): the eigenvalues of a symmetric 3x3
// tensor field and the T-web / V-web type of every voxel from them.  The reference has neither step: these stand in for
// the T-web of Hahn et al. (2007) / Forero-Romero et al. (2009) and the V-web of Hoffman et al. (2012) as their authors'
// codes compute them on a smoothed mesh.  The tensors themselves come from nbe_lpt.hip (nbe_lpt2_hessian_spectrum,
// nbe_shear_spectrum) and the caller's transforms.  No context: no weights.
//
// Both kernels are grid-stride loops around the bodies of nbe_web.h, a voxel a lane and step or, where n^3 is a multiple of
// 4 and the pointers are aligned, four voxels with 16-byte accesses (nbe_lpt2_source's rule; component c starts at byte
// 4 c n^3, so an odd n has no aligned form).  Every eigenvalue word has one writer.  The counts are sums of ones: a lane
// keeps them packed in registers, a workgroup adds its lanes' in LDS and then once into the global words with 64-bit
// integer atomics, so every grid gives the same integers.

#include "../../include/nbe.h"
#include "nbe_spectral.h"
#include "nbe_web.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace {

using nbe::kWebNaN;
using nbe::kWebNaNType;

constexpr int kWebThreads = 256;
constexpr int kWebBlocks = 2048;                           // 8 workgroups for each of 256 compute units
constexpr int kMaxThresholds = NBE_WEB_MAX_THRESHOLDS;
constexpr int kSlots = 5;                                  // counts[t][0 .. 3] and the NaN slot

__global__ __launch_bounds__(kWebThreads) void eigenvalues_kernel(const float* __restrict__ t, float* __restrict__ eig,
                                                                  long long cells) {
    const long long step = (long long)gridDim.x * kWebThreads;
    for (long long i = blockIdx.x * (long long)kWebThreads + threadIdx.x; i < cells; i += step) {
        float e[3];
        nbe::web_eigenvalues(t[i], t[cells + i], t[2 * cells + i], t[3 * cells + i], t[4 * cells + i], t[5 * cells + i], e);
        eig[i] = e[0]; eig[cells + i] = e[1]; eig[2 * cells + i] = e[2];
    }
}

__global__ __launch_bounds__(kWebThreads) void eigenvalues4_kernel(const float4* __restrict__ t, float4* __restrict__ eig,
                                                                   long long quads) {
    const long long step = (long long)gridDim.x * kWebThreads;
    for (long long i = blockIdx.x * (long long)kWebThreads + threadIdx.x; i < quads; i += step) {
        const float4 h0 = t[i], h1 = t[quads + i], h2 = t[2 * quads + i], h3 = t[3 * quads + i], h4 = t[4 * quads + i],
                     h5 = t[5 * quads + i];
        float x[3], y[3], z[3], w[3];
        nbe::web_eigenvalues(h0.x, h1.x, h2.x, h3.x, h4.x, h5.x, x);
        nbe::web_eigenvalues(h0.y, h1.y, h2.y, h3.y, h4.y, h5.y, y);
        nbe::web_eigenvalues(h0.z, h1.z, h2.z, h3.z, h4.z, h5.z, z);
        nbe::web_eigenvalues(h0.w, h1.w, h2.w, h3.w, h4.w, h5.w, w);
        eig[i] = make_float4(x[0], y[0], z[0], w[0]);
        eig[quads + i] = make_float4(x[1], y[1], z[1], w[1]);
        eig[2 * quads + i] = make_float4(x[2], y[2], z[2], w[2]);
    }
}

struct ClassifyArgs {
    const float* eig;           // (3, cells)
    unsigned char* types;       // (cells) or NULL
    unsigned long long* counts; // (nthresholds, 5) int64
    long long cells;
    int nthresholds, which;
    float th[kMaxThresholds];   // NaN beyond nthresholds: nothing is greater than it
};

// A lane counts its voxels of type m under threshold t in bits 16 m .. 16 m + 15 of acc[t], and hands them to the
// workgroup's LDS words before a field could overflow.
constexpr int kFlushEvery = 32768;

template <int TC>
__device__ inline void flush(unsigned long long* acc, unsigned& nans, unsigned long long* lds, int nthresholds) {
#pragma unroll
    for (int t = 0; t < TC; ++t) {
        if (t < nthresholds) {
#pragma unroll
            for (int m = 0; m < 4; ++m) {
                const unsigned v = (unsigned)(acc[t] >> (16 * m)) & 0xffffu;
                if (v) atomicAdd(&lds[t * kSlots + m], (unsigned long long)v);
            }
        }
        acc[t] = 0ull;
    }
    if (nans) atomicAdd(&lds[kWebNaN], (unsigned long long)nans);          // kept once, in row 0's slot
    nans = 0u;
}

// TC: the thresholds a lane keeps in registers (nthresholds <= TC); WIDE: four voxels a step
template <int TC, bool WIDE>
__global__ __launch_bounds__(kWebThreads) void classify_kernel(ClassifyArgs A) {
    __shared__ unsigned long long lds[kMaxThresholds * kSlots];
    const int tid = threadIdx.x;
    for (int i = tid; i < kMaxThresholds * kSlots; i += kWebThreads) lds[i] = 0ull;
    __syncthreads();

    unsigned long long acc[TC];
#pragma unroll
    for (int t = 0; t < TC; ++t) acc[t] = 0ull;
    unsigned nans = 0u;
    const float thw = A.th[A.which];

    auto voxel = [&](float e0, float e1, float e2) -> unsigned char {
        if (nbe::web_type(e0, e1, e2, thw) == kWebNaN) {
            ++nans;
            return kWebNaNType;
        }
#pragma unroll
        for (int t = 0; t < TC; ++t) acc[t] += 1ull << (16 * nbe::web_type(e0, e1, e2, A.th[t]));
        return (unsigned char)nbe::web_type(e0, e1, e2, thw);
    };

    const long long items = WIDE ? A.cells / 4 : A.cells;
    const long long step = (long long)gridDim.x * kWebThreads;
    int since = 0;
    for (long long i = blockIdx.x * (long long)kWebThreads + tid; i < items; i += step) {
        if (WIDE) {
            const float4* e = (const float4*)A.eig;
            const float4 a = e[i], b = e[items + i], c = e[2 * items + i];
            uchar4 ty;
            ty.x = voxel(a.x, b.x, c.x); ty.y = voxel(a.y, b.y, c.y); ty.z = voxel(a.z, b.z, c.z); ty.w = voxel(a.w, b.w, c.w);
            if (A.types) ((uchar4*)A.types)[i] = ty;
            since += 4;
        } else {
            const unsigned char ty = voxel(A.eig[i], A.eig[items + i], A.eig[2 * items + i]);
            if (A.types) A.types[i] = ty;
            since += 1;
        }
        if (since >= kFlushEvery) {
            flush<TC>(acc, nans, lds, A.nthresholds);
            since = 0;
        }
    }
    flush<TC>(acc, nans, lds, A.nthresholds);
    __syncthreads();
    // the voxels without a type are the same under every threshold
    const unsigned long long nn = lds[kWebNaN];
    for (int i = tid; i < A.nthresholds * kSlots; i += kWebThreads) {
        const unsigned long long v = i % kSlots == kWebNaN ? nn : lds[i];
        if (v) atomicAdd(&A.counts[i], v);
    }
}

bool size_ok(int64_t n) { return n >= NBE_LPT_MIN_N && n <= NBE_LPT_MAX_N; }

bool overlap(const void* a, long long abytes, const void* b, long long bbytes) {
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)bbytes && b0 < a0 + (uintptr_t)abytes;
}

dim3 voxel_grid(long long items, int max_blocks) {
    long long blocks = (items + kWebThreads - 1) / kWebThreads;
    if (blocks > kWebBlocks) blocks = kWebBlocks;
    if (max_blocks > 0 && blocks > max_blocks) blocks = max_blocks;
    return dim3((unsigned)blocks);
}

template <int TC>
void launch_classify(const ClassifyArgs& A, bool wide, dim3 grid, hipStream_t s) {
    if (wide) hipLaunchKernelGGL((classify_kernel<TC, true>), grid, dim3(kWebThreads), 0, s, A);
    else hipLaunchKernelGGL((classify_kernel<TC, false>), grid, dim3(kWebThreads), 0, s, A);
}

}  // namespace

extern "C" {

int nbe_tensor_eigenvalues(const void* tensor, int64_t n, void* eig, int max_blocks, void* stream) {
    if (!tensor || !eig) return fail("nbe_tensor_eigenvalues: NULL argument");
    if (!size_ok(n)) return fail("nbe_tensor_eigenvalues: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    const long long cells = n * n * n;
    if (overlap(tensor, 6 * 4 * cells, eig, 3 * 4 * cells)) return fail("nbe_tensor_eigenvalues: eig aliases tensor");
    const bool wide = cells % 4 == 0 && ((uintptr_t)tensor | (uintptr_t)eig) % 16 == 0;
    const long long items = wide ? cells / 4 : cells;
    const dim3 grid = voxel_grid(items, max_blocks);
    if (wide)
        hipLaunchKernelGGL(eigenvalues4_kernel, grid, dim3(kWebThreads), 0, (hipStream_t)stream, (const float4*)tensor,
                           (float4*)eig, items);
    else
        hipLaunchKernelGGL(eigenvalues_kernel, grid, dim3(kWebThreads), 0, (hipStream_t)stream, (const float*)tensor,
                           (float*)eig, items);
    return launched("nbe_tensor_eigenvalues");
}

int nbe_web_classify(const void* eig, int64_t n, const float* thresholds, int nthresholds, int which, void* types,
                     void* counts, int max_blocks, void* stream) {
    if (!eig || !thresholds || !counts) return fail("nbe_web_classify: NULL argument");
    if (!size_ok(n)) return fail("nbe_web_classify: n %lld not in %d .. %d", (long long)n, NBE_LPT_MIN_N, NBE_LPT_MAX_N);
    if (nthresholds < 1 || nthresholds > kMaxThresholds)
        return fail("nbe_web_classify: %d thresholds unsupported (1 .. %d)", nthresholds, kMaxThresholds);
    if (which < 0 || which >= nthresholds) return fail("nbe_web_classify: threshold %d not in 0 .. %d", which, nthresholds - 1);
    ClassifyArgs A;
    for (int t = 0; t < kMaxThresholds; ++t) {
        A.th[t] = t < nthresholds ? thresholds[t] : __builtin_nanf("");
        if (t < nthresholds && !std::isfinite(thresholds[t])) return fail("nbe_web_classify: threshold %d is not finite", t);
    }
    A.eig = (const float*)eig;
    A.types = (unsigned char*)types;
    A.counts = (unsigned long long*)counts;
    A.cells = n * n * n;
    A.nthresholds = nthresholds;
    A.which = which;
    const bool wide = A.cells % 4 == 0 && (uintptr_t)eig % 16 == 0 && (uintptr_t)types % 4 == 0;
    const dim3 grid = voxel_grid(wide ? A.cells / 4 : A.cells, max_blocks);
    hipStream_t s = (hipStream_t)stream;
    if (nthresholds == 1) launch_classify<1>(A, wide, grid, s);
    else if (nthresholds <= 8) launch_classify<8>(A, wide, grid, s);
    else launch_classify<kMaxThresholds>(A, wide, grid, s);
    return launched("nbe_web_classify");
}

}  // extern "C"
