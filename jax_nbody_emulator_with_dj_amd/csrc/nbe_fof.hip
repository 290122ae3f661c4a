// Friends-of-friends halos of an emulated box (include/nbe.h, "Halos").  Replaces the particle
// positions, the nbodykit FoF run and the halo sums of the reference's scripts/halos.py (:359-404, :407-450).  No context:
// these entry points need no weights.
//
// Everything that decides a link is an integer, and the integers, the adjacency of cells and the union-find are written
// once in nbe_catalog.h, with the arguments that they are sound; tools/catalog_host_walk.hip walks those bodies serially on
// the host.  Here are the kernels, which are grid-stride loops around them, the wave reduction and the entry points.

#include "../../include/nbe.h"
#include "nbe_catalog.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <cstdint>

using namespace nbe;

namespace {

constexpr int kFofThreads = 256;

struct FofExps { int q[3]; };

__global__ __launch_bounds__(kFofThreads) void fof_cells_kernel(const void* disp, int half, long long n, double L, int ncell,
                                                                int* __restrict__ X, long long* __restrict__ keys,
                                                                int* __restrict__ parent, int* __restrict__ stats) {
    const long long count = n * n * n;
    int bad = 0;
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < count; x += (long long)gridDim.x * blockDim.x)
        fof_lattice_row(disp, half, n, count, L, ncell, x, X, keys, parent, &bad);
    if (bad) atomicAdd(&stats[0], bad);
}

__global__ __launch_bounds__(kFofThreads) void fof_gather_kernel(const int* __restrict__ X, const long long* __restrict__ order,
                                                                 long long count, FofParticle* __restrict__ P) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < count; j += (long long)gridDim.x * blockDim.x)
        P[j] = fof_gather_record(X, order, count, j);
}

__global__ __launch_bounds__(kFofThreads) void fof_link_kernel(const FofParticle* __restrict__ P, const long long* __restrict__ sk,
                                                               long long count, int ncell, long long R2, int* parent) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x)
        fof_link_particle(P, sk, count, i, ncell, R2, parent);
}

// Sum v[0 .. NV) over the runs of equal key among the 64 lanes of a wave (every lane takes part; key < 0 marks a lane
// without a term); true in the last lane of each run, which then holds the run's sums.  A key may come back later in the
// wave, so a run is known by the lane it starts at, not by its key.
template <int NV>
__device__ inline bool wave_run_sums(int key, long long (&v)[NV]) {
    const int lane = (int)(threadIdx.x & 63);
    const int prev = __shfl_up(key, 1, 64);
    const unsigned long long heads = __ballot(lane == 0 || prev != key);
    const int start = 63 - __clzll((long long)(heads & (~0ull >> (63 - lane))));   // bit 0 is set: lane 0 heads a run
    for (int off = 1; off < 64; off <<= 1) {
        const bool take = lane - off >= start;
#pragma unroll
        for (int c = 0; c < NV; ++c) {
            const long long u = __shfl_up(v[c], off, 64);
            if (take) v[c] += u;
        }
    }
    return key >= 0 && (lane == 63 || ((heads >> (lane + 1)) & 1ull));
}

// every particle to its root, and the sizes of the groups at their roots (runs of one root inside a wave add once)
__global__ __launch_bounds__(kFofThreads) void fof_labels_kernel(int* parent, long long count, int* __restrict__ sizes) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = blockIdx.x * (long long)blockDim.x; base < count; base += stride) {
        const long long x = base + threadIdx.x;
        int r = -1;
        if (x < count) {
            r = fof_root(parent, (int)x);
            parent[x] = r;                                 // a racing reader sees x's old pointer or its root: both lead to r
        }
        long long one[1] = {1};
        if (wave_run_sums<1>(r, one)) atomicAdd(&sizes[r], (int)one[0]);
    }
}

template <bool REDUCE, int NV>
__global__ __launch_bounds__(kFofThreads) void fof_catalog_kernel(const int* __restrict__ X, const int* __restrict__ parent,
                                                                  const int* __restrict__ slot, const void* vel, int vel_half,
                                                                  FofExps E, long long count,
                                                                  unsigned long long* __restrict__ sums, int* __restrict__ labels) {
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long base = blockIdx.x * (long long)blockDim.x; base < count; base += stride) {
        const long long x = base + threadIdx.x;
        int s = -1;
        long long t[6] = {0, 0, 0, 0, 0, 0};
        if (x < count) {
            const int r = parent[x];
            s = slot[r];
            if (labels) labels[x] = s;
            if (s >= 0) fof_terms(X, count, x, r, NV == 6 ? vel : nullptr, vel_half, E.q, t);
        }
        long long v[NV];
#pragma unroll
        for (int c = 0; c < NV; ++c) v[c] = t[c];
        if (REDUCE) {
            if (wave_run_sums<NV>(s, v)) {
#pragma unroll
                for (int c = 0; c < NV; ++c) atomicAdd(&sums[(long long)s * NV + c], (unsigned long long)v[c]);
            }
        } else if (s >= 0) {
#pragma unroll
            for (int c = 0; c < NV; ++c) atomicAdd(&sums[(long long)s * NV + c], (unsigned long long)v[c]);
        }
    }
}

}  // namespace

extern "C" {

int nbe_fof_cells(const void* disp, int disp_dtype, int64_t n, double boxsize, int ncell, int max_blocks, void* coords,
                  void* keys, void* parent, void* stats, void* stream) {
    if (!disp || !coords || !keys || !parent || !stats) return fail("nbe_fof_cells: NULL argument");
    if (disp_dtype != NBE_F32 && disp_dtype != NBE_F16) return fail("nbe_fof_cells: dtype %d unsupported", disp_dtype);
    if (n < NBE_FOF_MIN_N || n > NBE_FOF_MAX_N)
        return fail("nbe_fof_cells: lattice size %lld unsupported (%d .. %d)", (long long)n, NBE_FOF_MIN_N, NBE_FOF_MAX_N);
    if (int rc = check_boxsize("nbe_fof_cells", boxsize)) return rc;
    if (int rc = check_ncell("nbe_fof_cells", ncell)) return rc;
    const long long count = (long long)n * n * n;
    hipLaunchKernelGGL(fof_cells_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream, disp,
                       disp_dtype == NBE_F16, (long long)n, boxsize, ncell, (int*)coords, (long long*)keys, (int*)parent,
                       (int*)stats);
    return launched("nbe_fof_cells");
}

int nbe_fof_gather(const void* coords, const void* order, int64_t count, int max_blocks, void* sorted, void* stream) {
    if (!coords || !order || !sorted) return fail("nbe_fof_gather: NULL argument");
    if (int rc = check_count("nbe_fof_gather", count)) return rc;
    hipLaunchKernelGGL(fof_gather_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream,
                       (const int*)coords, (const long long*)order, (long long)count, (FofParticle*)sorted);
    return launched("nbe_fof_gather");
}

int nbe_fof_link(const void* sorted, const void* sorted_keys, int64_t count, int ncell, int64_t r2, int max_blocks,
                 void* parent, void* stream) {
    if (!sorted || !sorted_keys || !parent) return fail("nbe_fof_link: NULL argument");
    if (int rc = check_count("nbe_fof_link", count)) return rc;
    if (int rc = check_ncell("nbe_fof_link", ncell)) return rc;
    // the cells must be at least isqrt(r2) + 1 units wide (the adjacency argument): ncell (s + 1) <= 2^30
    const long long room = (1LL << kCoordBits) / ncell - 1;
    if (r2 < 0 || r2 >= (room + 1) * (room + 1))
        return fail("nbe_fof_link: r2 %lld needs cells wider than 2^30 / %d", (long long)r2, ncell);
    hipLaunchKernelGGL(fof_link_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream,
                       (const FofParticle*)sorted, (const long long*)sorted_keys, (long long)count, ncell, (long long)r2,
                       (int*)parent);
    return launched("nbe_fof_link");
}

int nbe_fof_labels(void* parent, int64_t count, int max_blocks, void* sizes, void* stream) {
    if (!parent || !sizes) return fail("nbe_fof_labels: NULL argument");
    if (int rc = check_count("nbe_fof_labels", count)) return rc;
    hipLaunchKernelGGL(fof_labels_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream,
                       (int*)parent, (long long)count, (int*)sizes);
    return launched("nbe_fof_labels");
}

int nbe_fof_catalog(const void* coords, const void* parent, const void* slot, const void* velocity, int velocity_dtype,
                    const int exponents[3], int64_t count, int wave_reduce, int max_blocks, void* sums, void* labels,
                    void* stream) {
    if (!coords || !parent || !slot || !sums) return fail("nbe_fof_catalog: NULL argument");
    if (int rc = check_count("nbe_fof_catalog", count)) return rc;
    FofExps E = {{0, 0, 0}};
    if (velocity) {
        if (velocity_dtype != NBE_F32 && velocity_dtype != NBE_F16)
            return fail("nbe_fof_catalog: dtype %d unsupported", velocity_dtype);
        if (!exponents) return fail("nbe_fof_catalog: a velocity needs its exponents");
        for (int c = 0; c < 3; ++c) {
            if (exponents[c] < -200 || exponents[c] > 200) return fail("nbe_fof_catalog: exponent %d out of range", exponents[c]);
            E.q[c] = 24 - exponents[c];
        }
    }
    const dim3 grid(fof_grid(count, max_blocks)), block(kFofThreads);
    hipStream_t s = (hipStream_t)stream;
    const int half = velocity_dtype == NBE_F16;
#define NBE_FOF_LAUNCH(R, NV)                                                                                              \
    hipLaunchKernelGGL((fof_catalog_kernel<R, NV>), grid, block, 0, s, (const int*)coords, (const int*)parent,            \
                       (const int*)slot, velocity, half, E, (long long)count, (unsigned long long*)sums, (int*)labels)
    if (velocity) { if (wave_reduce) NBE_FOF_LAUNCH(true, 6); else NBE_FOF_LAUNCH(false, 6); }
    else { if (wave_reduce) NBE_FOF_LAUNCH(true, 3); else NBE_FOF_LAUNCH(false, 3); }
#undef NBE_FOF_LAUNCH
    return launched("nbe_fof_catalog");
}

}  // extern "C"
