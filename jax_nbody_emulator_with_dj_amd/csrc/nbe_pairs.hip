// Pair counts of periodic catalogues (include/nbe.h, "Pairs"): the histogram of Corrfunc's
// theory.DD / theory.DDsmu and of nbodykit's SimulationBox2PCF ('1d' and '2d' modes).  No context: these entry points need
// no weights.
//
// Everything that decides a bin is an integer: FoF's coordinates, minimum-image differences, cells and keys, the bin rule
// T_b < q <= T_{b+1}, the exact mu bin, the adjacency of cells and the at most 18 ranges of sorted records that a particle
// meets (pair_range) are written once in nbe_catalog.h, and tools/catalog_host_walk.hip walks those bodies serially on the
// host.  A count is a sum of ones, so every grouping of the adds gives the same bits.
//
// Two decompositions of the same work.  "Particles": FoF's form, one thread per sorted particle of A reading its own ranges
// from memory; the threads of a wave that share a cell read the same record at the same time, so the loads are as good as
// uniform.  "Cells": a workgroup takes 256 consecutive sorted particles of A and goes through the runs of one cell among
// them; for each run the ranges of B are streamed through one LDS tile after another and every particle of the run, held in
// registers by its thread, meets every record of the tile.  Both add into a per-workgroup LDS image of 64-bit counters that
// is flushed once with 64-bit global atomics, with one LDS atomic per lane or with the equal bins of a wave added once.
// nbe_pair_count takes "particles" with one atomic per lane, which measured fastest from 0.02 to 460 particles in a cell
// (DESIGN.md section 12.7); nbe_pair_count_form reaches the other three for the timing tool and the tests.

#include "../../include/nbe.h"
#include "nbe_catalog.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <cstdint>

using namespace nbe;

namespace {

constexpr int kPairThreads = 256;

__global__ __launch_bounds__(kPairThreads) void pair_coords_kernel(const void* pos, int wide, long long count, double L, int ncell,
                                                                   int* __restrict__ X, long long* __restrict__ keys,
                                                                   int* __restrict__ stats) {
    int bad = 0;
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < count; x += (long long)gridDim.x * blockDim.x)
        pair_position_row(pos, wide, count, L, ncell, x, X, keys, &bad);
    if (bad) atomicAdd(&stats[0], bad);
}

// image[entry] += 1 for every lane of the wave that calls it with entry >= 0.  COMBINE: the lanes that hold one entry add
// once, their number (most pairs fall into the outermost bins, so a wave's adds hit few addresses); else one LDS atomic a
// lane.  Every active lane of the wave must call it together.
template <bool COMBINE>
__device__ inline void pair_add(unsigned long long* image, int entry) {
    if (!COMBINE) {
        if (entry >= 0) atomicAdd(&image[entry], 1ull);
        return;
    }
    unsigned long long pending = __ballot(entry >= 0);
    const int lane = (int)(threadIdx.x & 63);
    while (pending) {
        const int lead = __ffsll((long long)pending) - 1;
        const int e = __shfl(entry, lead, 64);
        const unsigned long long same = __ballot(entry == e);
        if (lane == lead) atomicAdd(&image[e], (unsigned long long)__popcll(same));
        pending &= ~same;
    }
}

__device__ inline void pair_image_begin(unsigned long long* image, int entries, long long* T, const PairBins& bins, int nb) {
    for (int e = threadIdx.x; e < entries; e += kPairThreads) image[e] = 0;
    for (int b = threadIdx.x; b <= nb; b += kPairThreads) T[b] = bins.T[b];
    __syncthreads();
}

__device__ inline void pair_image_flush(const unsigned long long* image, int entries, unsigned long long* counts) {
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += kPairThreads)
        if (image[e]) atomicAdd(&counts[e], image[e]);
}

// "Cells": see the head of the file.  All loop bounds are the same in every thread of the workgroup.
template <bool COMBINE>
__global__ __launch_bounds__(kPairThreads) void pair_cells_kernel(const FofParticle* __restrict__ A, const long long* __restrict__ skA,
                                                                  long long countA, const FofParticle* __restrict__ B,
                                                                  const long long* __restrict__ skB, long long countB, int ncell,
                                                                  int half, PairBins bins, int nb, int s, int nmu, int los,
                                                                  unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long image[];
    __shared__ FofParticle tile[kPairThreads];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    __shared__ long long rlo[kPairRanges], rlen[kPairRanges];
    const int entries = nb * nmu, tid = (int)threadIdx.x;
    pair_image_begin(image, entries, T, bins, nb);
    for (long long base = blockIdx.x * (long long)kPairThreads; base < countA; base += (long long)gridDim.x * kPairThreads) {
        const long long end = base + kPairThreads < countA ? base + kPairThreads : countA;
        const long long i = base + tid;
        const FofParticle me = A[i < countA ? i : countA - 1];
        long long seg = base;
        while (seg < end) {                                                    // the run of one cell inside this chunk
            const long long key = skA[seg];
            const long long segend = fof_lower_bound(skA, end, seg, key + 1);
            const FofParticle first = A[seg];
            if (tid < kPairRanges) {
                long long lo, hi;
                pair_range(skB, countB, fof_cell(first.x0, ncell), fof_cell(first.x1, ncell), fof_cell(first.x2, ncell), ncell,
                           half != 0, tid, &lo, &hi);
                if (half && tid == 0) lo = seg;                                // earlier runs of this cell met this one already
                rlo[tid] = lo; rlen[tid] = hi - lo;
            }
            __syncthreads();
            const long long total = pair_ranges_total(rlen);
            const bool active = i >= seg && i < segend;
            const bool wave_on = __ballot(active) != 0;
            for (long long tb = 0; tb < total; tb += kPairThreads) {           // the ranges, end to end, a tile at a time
                if (tb) __syncthreads();
                long long q = tb + tid;
                if (q < total) {
                    const int t = pair_ranges_locate(rlen, &q);
                    FofParticle o = B[rlo[t] + q];
                    o.p = half && t == 0 ? (int)(rlo[0] + q) : kPairNoOrder;   // the own row: only the records behind i
                    tile[tid] = o;
                }
                __syncthreads();
                const int m = (int)(total - tb < kPairThreads ? total - tb : kPairThreads);
                if (wave_on)
                    for (int k = 0; k < m; ++k) {
                        const FofParticle o = tile[k];
                        pair_add<COMBINE>(image, active && o.p > (int)i ? pair_bin(me, o, T, nb, s, nmu, los) : -1);
                    }
            }
            __syncthreads();
            seg = segend;
        }
    }
    pair_image_flush(image, entries, counts);
}

// "Particles": FoF's decomposition, for catalogues with a few particles in a cell
template <bool COMBINE>
__global__ __launch_bounds__(kPairThreads) void pair_particles_kernel(const FofParticle* __restrict__ A, long long countA,
                                                                      const FofParticle* __restrict__ B,
                                                                      const long long* __restrict__ skB, long long countB, int ncell,
                                                                      int half, PairBins bins, int nb, int s, int nmu, int los,
                                                                      unsigned long long* __restrict__ counts) {
    extern __shared__ __attribute__((aligned(16))) unsigned long long image[];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    const int entries = nb * nmu;
    pair_image_begin(image, entries, T, bins, nb);
    for (long long i = blockIdx.x * (long long)kPairThreads + threadIdx.x; i < countA; i += (long long)gridDim.x * kPairThreads)
        pair_count_particle(A, i, B, skB, countB, ncell, half != 0, T, nb, s, nmu, los,
                            [&](int entry) { pair_add<COMBINE>(image, entry); });
    pair_image_flush(image, entries, counts);
}

int pair_count_launch(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                      int64_t countB, int ncell, const int64_t* thresholds, int nbins, int nmu, int los, int max_blocks, int form,
                      void* counts, void* stream) {
    if (!sortedA || !keysA || !thresholds || !counts) return fail("nbe_pair_count: NULL argument");
    if ((sortedB == nullptr) != (keysB == nullptr)) return fail("nbe_pair_count: sortedB and keysB go together");
    const bool half = sortedB == nullptr;
    if (half) { sortedB = sortedA; keysB = keysA; countB = countA; }
    if (!count_ok(countA) || !count_ok(countB))
        return fail("nbe_pair_count: bad particle counts %lld, %lld", (long long)countA, (long long)countB);
    if (int rc = check_ncell("nbe_pair_count", ncell)) return rc;
    if (nbins < 1 || nbins > NBE_PAIR_MAX_BINS) return fail("nbe_pair_count: nbins %d not in 1 .. %d", nbins, NBE_PAIR_MAX_BINS);
    if (nmu < 1 || nmu > NBE_PAIR_MAX_MU) return fail("nbe_pair_count: nmu %d not in 1 .. %d", nmu, NBE_PAIR_MAX_MU);
    if (nbins * nmu > NBE_PAIR_MAX_IMAGE) return fail("nbe_pair_count: %d x %d bins exceed %d", nbins, nmu, NBE_PAIR_MAX_IMAGE);
    if (los < 0 || los > 2) return fail("nbe_pair_count: los %d not in 0 .. 2", los);
    if (form < 0 || form > 3) return fail("nbe_pair_count_form: form %d not in 0 .. 3", form);
    PairBins bins;
    int s;
    if (int rc = check_thresholds("nbe_pair_count", thresholds, nbins, ncell, &bins, &s)) return rc;
    const bool cells = (form & 2) == 0, combine = (form & 1) != 0;
    const dim3 grid(fof_grid(countA, max_blocks)), block(kPairThreads);
    const size_t lds = (size_t)nbins * nmu * sizeof(unsigned long long);
    hipStream_t st = (hipStream_t)stream;
#define NBE_PAIR_LAUNCH(C)                                                                                                 \
    do {                                                                                                                   \
        if (cells)                                                                                                         \
            hipLaunchKernelGGL((pair_cells_kernel<C>), grid, block, lds, st, (const FofParticle*)sortedA,                  \
                               (const long long*)keysA, (long long)countA, (const FofParticle*)sortedB,                    \
                               (const long long*)keysB, (long long)countB, ncell, (int)half, bins, nbins, s, nmu, los,     \
                               (unsigned long long*)counts);                                                               \
        else                                                                                                               \
            hipLaunchKernelGGL((pair_particles_kernel<C>), grid, block, lds, st, (const FofParticle*)sortedA,              \
                               (long long)countA, (const FofParticle*)sortedB, (const long long*)keysB, (long long)countB, \
                               ncell, (int)half, bins, nbins, s, nmu, los, (unsigned long long*)counts);                   \
    } while (0)
    if (combine) NBE_PAIR_LAUNCH(true); else NBE_PAIR_LAUNCH(false);
#undef NBE_PAIR_LAUNCH
    return launched("nbe_pair_count");
}

}  // namespace

extern "C" {

int nbe_pair_coords(const void* pos, int pos_dtype, int64_t count, double boxsize, int ncell, int max_blocks, void* coords,
                    void* keys, void* stats, void* stream) {
    if (!pos || !coords || !keys || !stats) return fail("nbe_pair_coords: NULL argument");
    if (pos_dtype != NBE_F32 && pos_dtype != NBE_F64) return fail("nbe_pair_coords: dtype %d unsupported", pos_dtype);
    if (int rc = check_count("nbe_pair_coords", count)) return rc;
    if (int rc = check_boxsize("nbe_pair_coords", boxsize)) return rc;
    if (int rc = check_ncell("nbe_pair_coords", ncell)) return rc;
    hipLaunchKernelGGL(pair_coords_kernel, dim3(fof_grid(count, max_blocks)), dim3(kPairThreads), 0, (hipStream_t)stream, pos,
                       pos_dtype == NBE_F64, (long long)count, boxsize, ncell, (int*)coords, (long long*)keys, (int*)stats);
    return launched("nbe_pair_coords");
}

int nbe_pair_count(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                   int64_t countB, int ncell, const int64_t* thresholds, int nbins, int nmu, int los, int max_blocks,
                   void* counts, void* stream) {
    return pair_count_launch(sortedA, keysA, countA, sortedB, keysB, countB, ncell, thresholds, nbins, nmu, los, max_blocks,
                             NBE_PAIR_FORM, counts, stream);
}

int nbe_pair_count_form(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                        int64_t countB, int ncell, const int64_t* thresholds, int nbins, int nmu, int los, int max_blocks,
                        int form, void* counts, void* stream) {
    return pair_count_launch(sortedA, keysA, countA, sortedB, keysB, countB, ncell, thresholds, nbins, nmu, los, max_blocks,
                             form, counts, stream);
}

}  // extern "C"
