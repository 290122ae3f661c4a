// Radial count profiles around centres (include/nbe.h, "Profiles"): for every row of a catalogue
// of centres the histogram of its separations to a catalogue of matter -- the profile and spherical-overdensity step of
// a halo finder such as Rockstar or AHF, which the reference does not have.  No context: these entry points need no
// weights.
//
// Everything that decides a bin is the pair count's, from nbe_catalog.h: the records, pair_range with half = false (the 27
// cells around a centre as at most 18 ranges of the sorted matter), the ranges laid end to end and pair_bin with nmu = 1
// (the 32-bit rejection, q in 64 bits, T_b < q <= T_{b+1}).  Nothing about coordinates, the minimum image, the threshold
// rule or the adjacency of cells is restated here; tools/catalog_host_walk.hip walks the per-centre bodies on the host.
//
// What differs is the decomposition.  nbe_pair_count adds every row of A into one histogram with one thread per row;
// a halo catalogue has 10^3 .. 10^4 rows, a few dozen workgroups, and wants one histogram per row.  Here a centre is the
// unit of work.  "Group": a workgroup of 256 threads per centre, grid-strided; threads 0 .. 17 find the ranges, then all
// threads stream the ranges end to end, 256 records a step, each lane binning its record against the centre it holds in
// registers and adding into an LDS image of nbins 32-bit counters (a bin of one centre never exceeds countB <= 2^30).  The
// image is widened and written to the centre's row with plain vector stores: one workgroup owns a row, so there is no
// global atomic and the caller need not zero the output.  "Wave": the same with one wave per centre, four centres a
// workgroup and no workgroup barrier inside the loop, for catalogues whose 27 cells hold a few dozen records.  A count is a
// sum of ones: both forms and every launch geometry give the same bits.  nbe_halo_profiles takes the wave form from
// NBE_PROFILE_WAVE_CENTRES centres on where 27 countB / ncell^3 < NBE_PROFILE_WAVE_BELOW, as measured (section 12.8); a
// 64-bit image measured the same as the 32-bit one, which is half the LDS.

#include "../../include/nbe.h"
#include "nbe_catalog.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <cstdint>

using namespace nbe;

namespace {

constexpr int kProfileThreads = 256;
constexpr int kProfileWave = 64;
constexpr int kProfileWaves = kProfileThreads / kProfileWave;
constexpr int kProfileMaxGrid = 1 << 16;
#if defined(NBE_PROFILE_IMAGE64)                           // timing-probe builds only (tools/time_profiles.py --image64_lib)
using ProfileCounter = unsigned long long;
#else
using ProfileCounter = unsigned int;
#endif

// what one wave wrote to LDS becomes visible to its other lanes (no workgroup barrier: the waves run apart)
__device__ inline void profile_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

// "Group": a workgroup per centre.  Every loop bound is the same in all threads of the workgroup.
__global__ __launch_bounds__(kProfileThreads) void profile_group_kernel(const FofParticle* __restrict__ A, long long countA,
                                                                        const FofParticle* __restrict__ B,
                                                                        const long long* __restrict__ skB, long long countB,
                                                                        int ncell, PairBins bins, int nb, int s,
                                                                        unsigned long long* __restrict__ counts) {
    __shared__ ProfileCounter image[NBE_PAIR_MAX_BINS];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    __shared__ long long rlo[kPairRanges], rlen[kPairRanges];
    const int tid = (int)threadIdx.x;
    for (int b = tid; b <= nb; b += kProfileThreads) T[b] = bins.T[b];
    for (long long h = blockIdx.x; h < countA; h += gridDim.x) {
        const FofParticle me = A[h];
        if (tid < kPairRanges) profile_range(me, skB, countB, ncell, tid, rlo, rlen);
        for (int b = tid; b < nb; b += kProfileThreads) image[b] = 0;
        __syncthreads();
        profile_stream(me, B, rlo, rlen, pair_ranges_total(rlen), tid, kProfileThreads, T, nb, s,
                       [&](int b) { if (b >= 0) atomicAdd(&image[b], (ProfileCounter)1); });
        __syncthreads();
        unsigned long long* row = counts + (long long)me.p * nb;
        for (int b = tid; b < nb; b += kProfileThreads) row[b] = image[b];
        __syncthreads();                                   // the image and the ranges are free for the next centre
    }
}

// "Wave": a wave per centre, four centres a workgroup.  After the thresholds are in LDS no wave waits for another.
__global__ __launch_bounds__(kProfileThreads) void profile_wave_kernel(const FofParticle* __restrict__ A, long long countA,
                                                                       const FofParticle* __restrict__ B,
                                                                       const long long* __restrict__ skB, long long countB,
                                                                       int ncell, PairBins bins, int nb, int s,
                                                                       unsigned long long* __restrict__ counts) {
    __shared__ ProfileCounter images[kProfileWaves][NBE_PAIR_MAX_BINS];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    __shared__ long long los[kProfileWaves][kPairRanges], lens[kProfileWaves][kPairRanges];
    const int tid = (int)threadIdx.x, wave = tid / kProfileWave, lane = tid % kProfileWave;
    for (int b = tid; b <= nb; b += kProfileThreads) T[b] = bins.T[b];
    __syncthreads();
    ProfileCounter* image = images[wave];
    long long *rlo = los[wave], *rlen = lens[wave];
    for (long long h = blockIdx.x * (long long)kProfileWaves + wave; h < countA; h += (long long)gridDim.x * kProfileWaves) {
        const FofParticle me = A[h];
        if (lane < kPairRanges) profile_range(me, skB, countB, ncell, lane, rlo, rlen);
        for (int b = lane; b < nb; b += kProfileWave) image[b] = 0;
        profile_wave_sync();
        profile_stream(me, B, rlo, rlen, pair_ranges_total(rlen), lane, kProfileWave, T, nb, s,
                       [&](int b) { if (b >= 0) atomicAdd(&image[b], (ProfileCounter)1); });
        profile_wave_sync();
        unsigned long long* row = counts + (long long)me.p * nb;
        for (int b = lane; b < nb; b += kProfileWave) row[b] = image[b];
        profile_wave_sync();
    }
}

int halo_profiles_launch(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                         int64_t countB, int ncell, const int64_t* thresholds, int nbins, int max_blocks, int form,
                         void* counts, void* stream) {
    if (!sortedA || !keysA || !sortedB || !keysB || !thresholds || !counts) return fail("nbe_halo_profiles: NULL argument");
    if (!count_ok(countA) || !count_ok(countB))
        return fail("nbe_halo_profiles: bad row counts %lld, %lld", (long long)countA, (long long)countB);
    if (int rc = check_ncell("nbe_halo_profiles", ncell)) return rc;
    if (nbins < 1 || nbins > NBE_PAIR_MAX_BINS) return fail("nbe_halo_profiles: nbins %d not in 1 .. %d", nbins, NBE_PAIR_MAX_BINS);
    if (form < -1 || form > 1) return fail("nbe_halo_profiles_form: form %d not in 0 .. 1", form);
    // the library's choice: a wave per centre where there are centres enough to fill the card with waves and the 27 cells
    // of a centre hold few rows of B on average
    if (form < 0)
        form = countA >= NBE_PROFILE_WAVE_CENTRES &&
               27.0 * (double)countB < (double)NBE_PROFILE_WAVE_BELOW * ncell * ncell * ncell ? 1 : 0;
    PairBins bins;
    int s;
    if (int rc = check_thresholds("nbe_halo_profiles", thresholds, nbins, ncell, &bins, &s)) return rc;
    long long g = form ? (countA + kProfileWaves - 1) / kProfileWaves : countA;
    if (g > kProfileMaxGrid) g = kProfileMaxGrid;
    if (max_blocks > 0 && max_blocks < g) g = max_blocks;
    const dim3 grid((unsigned)g), block(kProfileThreads);
    hipStream_t st = (hipStream_t)stream;
    if (form)
        hipLaunchKernelGGL(profile_wave_kernel, grid, block, 0, st, (const FofParticle*)sortedA, (long long)countA,
                           (const FofParticle*)sortedB, (const long long*)keysB, (long long)countB, ncell, bins, nbins, s,
                           (unsigned long long*)counts);
    else
        hipLaunchKernelGGL(profile_group_kernel, grid, block, 0, st, (const FofParticle*)sortedA, (long long)countA,
                           (const FofParticle*)sortedB, (const long long*)keysB, (long long)countB, ncell, bins, nbins, s,
                           (unsigned long long*)counts);
    return launched("nbe_halo_profiles");
}

}  // namespace

extern "C" {

int nbe_halo_profiles(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                      int64_t countB, int ncell, const int64_t* thresholds, int nbins, int max_blocks, void* counts,
                      void* stream) {
    return halo_profiles_launch(sortedA, keysA, countA, sortedB, keysB, countB, ncell, thresholds, nbins, max_blocks,
                                -1, counts, stream);
}

int nbe_halo_profiles_form(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                           int64_t countB, int ncell, const int64_t* thresholds, int nbins, int max_blocks, int form,
                           void* counts, void* stream) {
    if (form < 0) return fail("nbe_halo_profiles_form: form %d not in 0 .. 1", form);
    return halo_profiles_launch(sortedA, keysA, countA, sortedB, keysB, countB, ncell, thresholds, nbins, max_blocks, form,
                                counts, stream);
}

}  // extern "C"
