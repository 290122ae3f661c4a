// Pairwise velocity moments of periodic catalogues and about centres (include/nbe.h, "Pairwise velocities"; DESIGN.md section
// 12.9): per bin of separation the number of pairs, the sum of their radial velocities and the sums of the squares of the
// radial and of the full velocity difference -- the mean streaming velocity v12(r) and the dispersions sigma_r(r), sigma_t(r) of
// the streaming model (Peebles 1980; Fisher 1995; Scoccimarro 2004; Reid & White 2011), the pairwise-velocity statistics that
// go with the configuration-space counts of Corrfunc's theory module (theory.DD, theory.vpf), and the infall and dispersion
// profile of matter about halos.  The reference has no such step.  No context: these entry points need no weights.
//
// Everything that decides a bin is the pair count's, and every term of a pair is an integer fixed by the pair alone
// (pair_velocity_terms in nbe_catalog.h: the exact rounding of the radial word by 128-bit comparisons), so each sum is the
// same bits for every launch geometry, form, row order and stream.  tools/catalog_host_walk.hip walks the same bodies on the
// host.  The velocity records lie parallel to the sorted FofParticle records and are read only for a pair that is in a bin.
//
// nbe_pair_velocity is nbe_pair_count's "particles" form: a thread per sorted row of A, a per-workgroup LDS image of
// 6 nbins 64-bit words, flushed once with 64-bit global atomics; the signed sum is added as its two's-complement word.  Form 1
// adds every term to the global table directly (the comparison for the image).  nbe_halo_velocity_profiles carries both
// decompositions of nbe_halo_profiles over: a workgroup per centre, or a wave per centre with four centres a workgroup; the
// per-centre image is nbins x 6 words, and the owner of a row writes it with plain stores.

#include "../../include/nbe.h"
#include "nbe_catalog.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <cstdint>

using namespace nbe;

namespace {

constexpr int kVelThreads = 256;
constexpr int kVelWave = 64;
constexpr int kVelWaves = kVelThreads / kVelWave;
constexpr int kVelMaxGrid = 1 << 16;
constexpr int kVelImage = kVelSums * NBE_PAIR_MAX_BINS;

__global__ __launch_bounds__(kVelThreads) void velocity_words_kernel(const void* vel, int dtype, int lattice, long long count,
                                                                     int e, const FofParticle* __restrict__ P,
                                                                     VelWord* __restrict__ out) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < count; j += (long long)gridDim.x * blockDim.x)
        out[j] = velocity_gather_record(vel, dtype, lattice, count, e, P, j);
}

// LOCAL: the terms go into the workgroup's LDS image, flushed once; else straight into the global table
template <bool LOCAL>
__global__ __launch_bounds__(kVelThreads) void pair_velocity_kernel(const FofParticle* __restrict__ A, const VelWord* __restrict__ VA,
                                                                    long long countA, const FofParticle* __restrict__ B,
                                                                    const VelWord* __restrict__ VB,
                                                                    const long long* __restrict__ skB, long long countB, int ncell,
                                                                    int half, PairBins bins, int nb, int s,
                                                                    unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long image[kVelImage];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    const int entries = kVelSums * nb;
    for (int e = threadIdx.x; e < entries; e += kVelThreads) image[e] = 0;
    for (int b = threadIdx.x; b <= nb; b += kVelThreads) T[b] = bins.T[b];
    __syncthreads();
    unsigned long long* into = LOCAL ? image : sums;
    for (long long i = blockIdx.x * (long long)kVelThreads + threadIdx.x; i < countA; i += (long long)gridDim.x * kVelThreads)
        pair_velocity_particle(A, VA, i, B, VB, skB, countB, ncell, half != 0, T, nb, s,
                               [&](int at, unsigned long long v) { if (v) atomicAdd(&into[at], v); });
    if (!LOCAL) return;
    __syncthreads();
    for (int e = threadIdx.x; e < entries; e += kVelThreads)
        if (image[e]) atomicAdd(&sums[e], image[e]);
}

// what one wave wrote to LDS becomes visible to its other lanes (no workgroup barrier: the waves run apart)
__device__ inline void velocity_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

__device__ inline VelWord centre_word(const VelWord* VA, long long h) {
    VelWord w;
    w.w0 = w.w1 = w.w2 = w.pad = 0;
    return VA ? VA[h] : w;
}

// "Group": a workgroup per centre.  Every loop bound is the same in all threads of the workgroup.
__global__ __launch_bounds__(kVelThreads) void profile_velocity_group_kernel(const FofParticle* __restrict__ A,
                                                                             const VelWord* __restrict__ VA, long long countA,
                                                                             const FofParticle* __restrict__ B,
                                                                             const VelWord* __restrict__ VB,
                                                                             const long long* __restrict__ skB, long long countB,
                                                                             int ncell, PairBins bins, int nb, int s,
                                                                             unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long image[kVelImage];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    __shared__ long long rlo[kPairRanges], rlen[kPairRanges];
    const int tid = (int)threadIdx.x, entries = kVelSums * nb;
    for (int b = tid; b <= nb; b += kVelThreads) T[b] = bins.T[b];
    for (long long h = blockIdx.x; h < countA; h += gridDim.x) {
        const FofParticle me = A[h];
        const VelWord mine = centre_word(VA, h);
        if (tid < kPairRanges) profile_range(me, skB, countB, ncell, tid, rlo, rlen);
        for (int e = tid; e < entries; e += kVelThreads) image[e] = 0;
        __syncthreads();
        profile_velocity_stream(me, mine, B, VB, rlo, rlen, pair_ranges_total(rlen), tid, kVelThreads, T, nb, s,
                                [&](int at, unsigned long long v) { if (v) atomicAdd(&image[at], v); });
        __syncthreads();
        unsigned long long* row = sums + (long long)me.p * entries;
        for (int e = tid; e < entries; e += kVelThreads) row[e] = image[e];
        __syncthreads();                                   // the image and the ranges are free for the next centre
    }
}

// "Wave": a wave per centre, four centres a workgroup.  After the thresholds are in LDS no wave waits for another.
__global__ __launch_bounds__(kVelThreads) void profile_velocity_wave_kernel(const FofParticle* __restrict__ A,
                                                                            const VelWord* __restrict__ VA, long long countA,
                                                                            const FofParticle* __restrict__ B,
                                                                            const VelWord* __restrict__ VB,
                                                                            const long long* __restrict__ skB, long long countB,
                                                                            int ncell, PairBins bins, int nb, int s,
                                                                            unsigned long long* __restrict__ sums) {
    __shared__ unsigned long long images[kVelWaves][kVelImage];
    __shared__ long long T[NBE_PAIR_MAX_BINS + 1];
    __shared__ long long los[kVelWaves][kPairRanges], lens[kVelWaves][kPairRanges];
    const int tid = (int)threadIdx.x, wave = tid / kVelWave, lane = tid % kVelWave, entries = kVelSums * nb;
    for (int b = tid; b <= nb; b += kVelThreads) T[b] = bins.T[b];
    __syncthreads();
    unsigned long long* image = images[wave];
    long long *rlo = los[wave], *rlen = lens[wave];
    for (long long h = blockIdx.x * (long long)kVelWaves + wave; h < countA; h += (long long)gridDim.x * kVelWaves) {
        const FofParticle me = A[h];
        const VelWord mine = centre_word(VA, h);
        if (lane < kPairRanges) profile_range(me, skB, countB, ncell, lane, rlo, rlen);
        for (int e = lane; e < entries; e += kVelWave) image[e] = 0;
        velocity_wave_sync();
        profile_velocity_stream(me, mine, B, VB, rlo, rlen, pair_ranges_total(rlen), lane, kVelWave, T, nb, s,
                                [&](int at, unsigned long long v) { if (v) atomicAdd(&image[at], v); });
        velocity_wave_sync();
        unsigned long long* row = sums + (long long)me.p * entries;
        for (int e = lane; e < entries; e += kVelWave) row[e] = image[e];
        velocity_wave_sync();
    }
}

int pair_velocity_launch(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                         const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds, int nbins,
                         int max_blocks, int form, void* sums, void* stream) {
    if (!sortedA || !keysA || !wordsA || !thresholds || !sums) return fail("nbe_pair_velocity: NULL argument");
    if ((sortedB == nullptr) != (keysB == nullptr) || (sortedB == nullptr) != (wordsB == nullptr))
        return fail("nbe_pair_velocity: sortedB, keysB and wordsB go together");
    const bool half = sortedB == nullptr;
    if (half) { sortedB = sortedA; keysB = keysA; wordsB = wordsA; countB = countA; }
    if (!count_ok(countA) || !count_ok(countB))
        return fail("nbe_pair_velocity: bad particle counts %lld, %lld", (long long)countA, (long long)countB);
    if (int rc = check_ncell("nbe_pair_velocity", ncell)) return rc;
    if (nbins < 1 || nbins > NBE_PAIR_MAX_BINS) return fail("nbe_pair_velocity: nbins %d not in 1 .. %d", nbins, NBE_PAIR_MAX_BINS);
    if (form < 0 || form > 1) return fail("nbe_pair_velocity_form: form %d not in 0 .. 1", form);
    PairBins bins;
    int s;
    if (int rc = check_thresholds("nbe_pair_velocity", thresholds, nbins, ncell, &bins, &s)) return rc;
    const dim3 grid(fof_grid(countA, max_blocks)), block(kVelThreads);
    hipStream_t st = (hipStream_t)stream;
    if (form == 0)
        hipLaunchKernelGGL((pair_velocity_kernel<true>), grid, block, 0, st, (const FofParticle*)sortedA, (const VelWord*)wordsA,
                           (long long)countA, (const FofParticle*)sortedB, (const VelWord*)wordsB, (const long long*)keysB,
                           (long long)countB, ncell, (int)half, bins, nbins, s, (unsigned long long*)sums);
    else
        hipLaunchKernelGGL((pair_velocity_kernel<false>), grid, block, 0, st, (const FofParticle*)sortedA, (const VelWord*)wordsA,
                           (long long)countA, (const FofParticle*)sortedB, (const VelWord*)wordsB, (const long long*)keysB,
                           (long long)countB, ncell, (int)half, bins, nbins, s, (unsigned long long*)sums);
    return launched("nbe_pair_velocity");
}

int halo_velocity_launch(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                         const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds, int nbins,
                         int max_blocks, int form, void* sums, void* stream) {
    if (!sortedA || !keysA || !sortedB || !keysB || !wordsB || !thresholds || !sums)
        return fail("nbe_halo_velocity_profiles: NULL argument");
    if (!count_ok(countA) || !count_ok(countB))
        return fail("nbe_halo_velocity_profiles: bad row counts %lld, %lld", (long long)countA, (long long)countB);
    if (int rc = check_ncell("nbe_halo_velocity_profiles", ncell)) return rc;
    if (nbins < 1 || nbins > NBE_PAIR_MAX_BINS)
        return fail("nbe_halo_velocity_profiles: nbins %d not in 1 .. %d", nbins, NBE_PAIR_MAX_BINS);
    if (form < -1 || form > 1) return fail("nbe_halo_velocity_profiles_form: form %d not in 0 .. 1", form);
    if (form < 0)                                          // nbe_halo_profiles's choice
        form = countA >= NBE_PROFILE_WAVE_CENTRES &&
               27.0 * (double)countB < (double)NBE_PROFILE_WAVE_BELOW * ncell * ncell * ncell ? 1 : 0;
    PairBins bins;
    int s;
    if (int rc = check_thresholds("nbe_halo_velocity_profiles", thresholds, nbins, ncell, &bins, &s)) return rc;
    long long g = form ? (countA + kVelWaves - 1) / kVelWaves : countA;
    if (g > kVelMaxGrid) g = kVelMaxGrid;
    if (max_blocks > 0 && max_blocks < g) g = max_blocks;
    const dim3 grid((unsigned)g), block(kVelThreads);
    hipStream_t st = (hipStream_t)stream;
    if (form)
        hipLaunchKernelGGL(profile_velocity_wave_kernel, grid, block, 0, st, (const FofParticle*)sortedA, (const VelWord*)wordsA,
                           (long long)countA, (const FofParticle*)sortedB, (const VelWord*)wordsB, (const long long*)keysB,
                           (long long)countB, ncell, bins, nbins, s, (unsigned long long*)sums);
    else
        hipLaunchKernelGGL(profile_velocity_group_kernel, grid, block, 0, st, (const FofParticle*)sortedA, (const VelWord*)wordsA,
                           (long long)countA, (const FofParticle*)sortedB, (const VelWord*)wordsB, (const long long*)keysB,
                           (long long)countB, ncell, bins, nbins, s, (unsigned long long*)sums);
    return launched("nbe_halo_velocity_profiles");
}

}  // namespace

extern "C" {

int nbe_velocity_words(const void* velocity, int dtype, int lattice, int64_t count, int exponent, const void* sorted,
                       int max_blocks, void* words, void* stream) {
    if (!velocity || !sorted || !words) return fail("nbe_velocity_words: NULL argument");
    if (lattice ? dtype != NBE_F32 && dtype != NBE_F16 : dtype != NBE_F32 && dtype != NBE_F64)
        return fail("nbe_velocity_words: dtype %d unsupported for a %s", dtype, lattice ? "(3, count) field" : "(count, 3) table");
    if (int rc = check_count("nbe_velocity_words", count)) return rc;
    if (exponent < -1000 || exponent > 1024) return fail("nbe_velocity_words: exponent %d out of range", exponent);
    hipLaunchKernelGGL(velocity_words_kernel, dim3(fof_grid(count, max_blocks)), dim3(kVelThreads), 0, (hipStream_t)stream,
                       velocity, dtype, lattice != 0, (long long)count, exponent, (const FofParticle*)sorted, (VelWord*)words);
    return launched("nbe_velocity_words");
}

int nbe_pair_velocity(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                      const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds, int nbins,
                      int max_blocks, void* sums, void* stream) {
    return pair_velocity_launch(sortedA, keysA, wordsA, countA, sortedB, keysB, wordsB, countB, ncell, thresholds, nbins,
                                max_blocks, 0, sums, stream);
}

int nbe_pair_velocity_form(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                           const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds,
                           int nbins, int max_blocks, int form, void* sums, void* stream) {
    return pair_velocity_launch(sortedA, keysA, wordsA, countA, sortedB, keysB, wordsB, countB, ncell, thresholds, nbins,
                                max_blocks, form, sums, stream);
}

int nbe_halo_velocity_profiles(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA, const void* sortedB,
                               const void* keysB, const void* wordsB, int64_t countB, int ncell, const int64_t* thresholds,
                               int nbins, int max_blocks, void* sums, void* stream) {
    return halo_velocity_launch(sortedA, keysA, wordsA, countA, sortedB, keysB, wordsB, countB, ncell, thresholds, nbins,
                                max_blocks, -1, sums, stream);
}

int nbe_halo_velocity_profiles_form(const void* sortedA, const void* keysA, const void* wordsA, int64_t countA,
                                    const void* sortedB, const void* keysB, const void* wordsB, int64_t countB, int ncell,
                                    const int64_t* thresholds, int nbins, int max_blocks, int form, void* sums, void* stream) {
    if (form < 0) return fail("nbe_halo_velocity_profiles_form: form %d not in 0 .. 1", form);
    return halo_velocity_launch(sortedA, keysA, wordsA, countA, sortedB, keysB, wordsB, countB, ncell, thresholds, nbins,
                                max_blocks, form, sums, stream);
}

}  // extern "C"
