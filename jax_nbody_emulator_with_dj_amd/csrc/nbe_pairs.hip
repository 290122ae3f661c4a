// Pair counts of periodic catalogues (include/nbe.h, "Pairs"): the histogram of Corrfunc's
// theory.DD / theory.DDsmu and of nbodykit's SimulationBox2PCF ('1d' and '2d' modes).  No context: these entry points need
// no weights.
//
// Everything that decides a bin is an integer, and the integers are FoF's (csrc/nbe_fof.hip, whose inline bodies this file
// includes): coordinates X_c in units of L / 2^30, the minimum-image difference d_c = fof_diff, q = d_0^2 + d_1^2 + d_2^2 in
// 64 bits (below 2^60), cells (X_c ncell) >> 30 and their keys.  With the thresholds T_0 < ... < T_nb a pair is in radial bin
// b iff T_b < q <= T_{b+1} ("<= T" is the FoF link rule), and with nmu > 1 in mu bin m = #{ j in 1 .. nmu - 1 :
// d_los^2 nmu^2 >= j^2 q } for q > 0, the two sides compared as 128-bit products, and m = 0 for q = 0.  A count is a sum of
// ones, so every grouping of the adds gives the same bits.
//
// Adjacency is FoF's argument with s = isqrt(T_nb): ncell (s + 1) <= 2^30, so two particles with q <= T_nb sit in the same
// cell or in cells adjacent with wrap-around, and ncell >= 3 keeps the offsets -1, 0, +1 distinct.  A cross count visits the
// 27 cells around a particle of A in the sorted B; an auto count visits the later particles of the own cell and FoF's half
// set of 13 cells, so that each unordered pair is met once.  Cells of one (c0, c1) row that are consecutive in c2 are
// consecutive in the sorted keys and form one range; a row that crosses the periodic face in c2 adds a second one: at most
// 18 ranges (pair_range), found by binary search in the sorted keys.
//
// Two decompositions of the same work.  "Particles": FoF's form, one thread per sorted particle of A reading its own ranges
// from memory; the threads of a wave that share a cell read the same record at the same time, so the loads are as good as
// uniform.  "Cells": a workgroup takes 256 consecutive sorted particles of A and goes through the runs of one cell among
// them; for each run the ranges of B are streamed through one LDS tile after another and every particle of the run, held in
// registers by its thread, meets every record of the tile.  Both add into a per-workgroup LDS image of 64-bit counters that
// is flushed once with 64-bit global atomics, with one LDS atomic per lane or with the equal bins of a wave added once.
// nbe_pair_count takes "particles" with one atomic per lane, which measured fastest from 0.02 to 460 particles in a cell
// (DESIGN.md section 12.7); nbe_pair_count_form reaches the other three for the timing tool and the tests.
//
// The per-pair and per-particle bodies are __host__ __device__ so that a stand-alone program can walk them serially on the
// host (tools/pairs_host_walk.hip); only the tiles, the wave-level combining and the launches are device code.

#ifndef NBE_FOF_BODIES_ONLY
#define NBE_FOF_BODIES_ONLY 1                              // FoF's inline bodies without its entry points
#endif
#include "nbe_fof.hip"

namespace {

constexpr int kPairThreads = 256;
constexpr int kPairRanges = 18;                            // 9 rows of cells, each with its part across the periodic face
constexpr int kPairNoOrder = 0x7fffffff;                   // the sorted position of a record that any particle may meet

struct PairBins { long long T[NBE_PAIR_MAX_BINS + 1]; };   // the thresholds, passed by value

// X = rint((x / L) 2^30) mod 2^30; false for a non-finite position or one 2^20 boxes or more away.  |t| < 2^50, and the
// two's-complement AND is the mathematical modulus.
__host__ __device__ inline bool pair_coordinate(double x, double L, int* X) {
    const double r = x / L;
    if (!(fabs(r) < kMaxShift)) return false;
    *X = (int)((long long)rint(r * kCoordUnit) & kCoordMask);
    return true;
}

__host__ __device__ inline double pair_load_real(const void* p, int wide, long long i) {
    return wide ? ((const double*)p)[i] : (double)((const float*)p)[i];
}

// isqrt of 0 <= v < 2^62
[[maybe_unused]] inline long long pair_isqrt(long long v) {
    long long s = (long long)std::sqrt((double)v);
    while (s * s > v) --s;
    while ((s + 1) * (s + 1) <= v) ++s;
    return s;
}

// Range t of 0 .. 17 of the sorted keys sk[0 .. count) that a particle of cell (c0, c1, c2) meets: row r = t >> 1 of cells,
// and for odd t that row's cell across the periodic face in c2 (empty where the row does not cross it).  Cross counts
// (half = false): the 9 rows (o0, o1) in -1 .. 1, cells c2 - 1 .. c2 + 1.  Auto counts (half = true): row 0 is the own
// cell and the cell at c2 + 1 -- the caller keeps to the records behind its own --, rows 1 .. 4 are FoF's (0, 1), (1, -1),
// (1, 0), (1, 1) with c2 - 1 .. c2 + 1, rows 5 .. 8 are empty.
__host__ __device__ inline void pair_range(const long long* sk, long long count, int c0, int c1, int c2, int ncell, bool half,
                                           int t, long long* lo, long long* hi) {
    const int r = t >> 1, wrap = t & 1;
    *lo = *hi = 0;
    int o0, o1;
    if (half) {
        if (r > 4) return;
        const int o0s[5] = {0, 0, 1, 1, 1}, o1s[5] = {0, 1, -1, 0, 1};
        o0 = o0s[r]; o1 = o1s[r];
    } else {
        o0 = r / 3 - 1; o1 = r % 3 - 1;
    }
    int b0 = c0 + o0, b1 = c1 + o1;
    b0 = b0 < 0 ? b0 + ncell : b0 >= ncell ? b0 - ncell : b0;
    b1 = b1 < 0 ? b1 + ncell : b1 >= ncell ? b1 - ncell : b1;
    const long long base = fof_key(b0, b1, 0, ncell);
    const bool own = half && r == 0;
    long long k0, k1;                                      // keys k0 .. k1 - 1
    if (!wrap) {
        k0 = base + (own ? c2 : c2 > 0 ? c2 - 1 : 0);
        k1 = base + (c2 + 1 < ncell ? c2 + 1 : ncell - 1) + 1;
    } else {                                               // ncell >= 3 keeps the cell across the face out of the range above
        if (c2 + 1 == ncell) k0 = base;
        else if (c2 == 0 && !own) k0 = base + ncell - 1;
        else return;
        k1 = k0 + 1;
    }
    *lo = fof_lower_bound(sk, count, 0, k0);
    *hi = fof_lower_bound(sk, count, *lo, k1);
}

// d_los^2 nmu^2 >= j^2 q, exactly
__host__ __device__ inline bool pair_mu_ge(unsigned long long l2, unsigned long long q, int nmu, int j) {
    return (unsigned __int128)l2 * (unsigned)(nmu * nmu) >= (unsigned __int128)q * (unsigned)(j * j);
}

// The image entry b nmu + m of the pair (a, o), or -1 where it is in no bin.  T[0 .. nb] are the thresholds, s = isqrt(T[nb]):
// |d_c| <= s is necessary for q <= T[nb] and is tested in 32 bits before any 64-bit product.  The float estimate of m only
// says where the exact comparisons start.
__host__ __device__ inline int pair_bin(const FofParticle& a, const FofParticle& o, const long long* T, int nb, int s, int nmu,
                                        int los) {
    const int d0 = (int)fof_diff(a.x0, o.x0), d1 = (int)fof_diff(a.x1, o.x1), d2 = (int)fof_diff(a.x2, o.x2);
    if ((d0 < 0 ? -d0 : d0) > s || (d1 < 0 ? -d1 : d1) > s || (d2 < 0 ? -d2 : d2) > s) return -1;
    const long long q = (long long)d0 * d0 + (long long)d1 * d1 + (long long)d2 * d2;
    if (q <= T[0] || q > T[nb]) return -1;
    int lo = 0, hi = nb;                                   // T[lo] < q <= T[hi]
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (T[mid] < q) lo = mid; else hi = mid;
    }
    int m = 0;
    if (nmu > 1 && q > 0) {
        const long long dl = los == 0 ? d0 : los == 1 ? d1 : d2;
        const unsigned long long l2 = (unsigned long long)(dl * dl);
        m = (int)((float)nmu * sqrtf((float)l2 / (float)q));
        m = m < 0 ? 0 : m > nmu - 1 ? nmu - 1 : m;
        while (m < nmu - 1 && pair_mu_ge(l2, (unsigned long long)q, nmu, m + 1)) ++m;
        while (m > 0 && !pair_mu_ge(l2, (unsigned long long)q, nmu, m)) --m;
    }
    return lo * nmu + m;
}

// The particle at sorted position i of A against its ranges of B, one pair at a time ("particles" form, and the host
// walk): image[entry] += 1 through `add`.
template <typename Add>
__host__ __device__ inline void pair_count_particle(const FofParticle* A, long long i, const FofParticle* B, const long long* skB,
                                                    long long countB, int ncell, bool half, const long long* T, int nb, int s,
                                                    int nmu, int los, Add add) {
    const FofParticle me = A[i];
    const int c0 = fof_cell(me.x0, ncell), c1 = fof_cell(me.x1, ncell), c2 = fof_cell(me.x2, ncell);
    for (int t = 0; t < (half ? 10 : kPairRanges); ++t) {
        long long lo, hi;
        pair_range(skB, countB, c0, c1, c2, ncell, half, t, &lo, &hi);
        if (half && t == 0) lo = i + 1;                    // the rest of the own cell: i lies inside this range
        for (long long j = lo; j < hi; ++j) add(pair_bin(me, B[j], T, nb, s, nmu, los));
    }
}

#if defined(__HIPCC__)

__global__ __launch_bounds__(kPairThreads) void pair_coords_kernel(const void* pos, int wide, long long count, double L, int ncell,
                                                                   int* __restrict__ X, long long* __restrict__ keys,
                                                                   int* __restrict__ stats) {
    int bad = 0;
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < count; x += (long long)gridDim.x * blockDim.x) {
        int X0 = 0, X1 = 0, X2 = 0;
        const bool ok = pair_coordinate(pair_load_real(pos, wide, 3 * x), L, &X0) &
                        pair_coordinate(pair_load_real(pos, wide, 3 * x + 1), L, &X1) &
                        pair_coordinate(pair_load_real(pos, wide, 3 * x + 2), L, &X2);
        if (!ok) { ++bad; X0 = X1 = X2 = 0; }
        X[x] = X0; X[count + x] = X1; X[2 * count + x] = X2;
        keys[x] = fof_key(fof_cell(X0, ncell), fof_cell(X1, ncell), fof_cell(X2, ncell), ncell);
    }
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
            long long total = 0;
            for (int t = 0; t < kPairRanges; ++t) total += rlen[t];
            const bool active = i >= seg && i < segend;
            const bool wave_on = __ballot(active) != 0;
            for (long long tb = 0; tb < total; tb += kPairThreads) {           // the ranges, end to end, a tile at a time
                if (tb) __syncthreads();
                long long q = tb + tid;
                if (q < total) {
                    int t = 0;
                    for (long long len = rlen[0]; q >= len; len = rlen[++t]) q -= len;
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

#endif  // __HIPCC__

}  // namespace

#if defined(__HIPCC__) && !defined(NBE_PAIRS_BODIES_ONLY)

namespace {

int pair_count_launch(const void* sortedA, const void* keysA, int64_t countA, const void* sortedB, const void* keysB,
                      int64_t countB, int ncell, const int64_t* thresholds, int nbins, int nmu, int los, int max_blocks, int form,
                      void* counts, void* stream) {
    if (!sortedA || !keysA || !thresholds || !counts) return fail("nbe_pair_count: NULL argument");
    if ((sortedB == nullptr) != (keysB == nullptr)) return fail("nbe_pair_count: sortedB and keysB go together");
    const bool half = sortedB == nullptr;
    if (half) { sortedB = sortedA; keysB = keysA; countB = countA; }
    if (countA < 1 || countA > (1LL << 30) || countB < 1 || countB > (1LL << 30))
        return fail("nbe_pair_count: bad particle counts %lld, %lld", (long long)countA, (long long)countB);
    if (ncell < 3 || ncell > NBE_FOF_MAX_CELLS) return fail("nbe_pair_count: ncell %d not in 3 .. %d", ncell, NBE_FOF_MAX_CELLS);
    if (nbins < 1 || nbins > NBE_PAIR_MAX_BINS) return fail("nbe_pair_count: nbins %d not in 1 .. %d", nbins, NBE_PAIR_MAX_BINS);
    if (nmu < 1 || nmu > NBE_PAIR_MAX_MU) return fail("nbe_pair_count: nmu %d not in 1 .. %d", nmu, NBE_PAIR_MAX_MU);
    if (nbins * nmu > NBE_PAIR_MAX_IMAGE) return fail("nbe_pair_count: %d x %d bins exceed %d", nbins, nmu, NBE_PAIR_MAX_IMAGE);
    if (los < 0 || los > 2) return fail("nbe_pair_count: los %d not in 0 .. 2", los);
    if (form < 0 || form > 3) return fail("nbe_pair_count_form: form %d not in 0 .. 3", form);
    PairBins bins;
    for (int b = 0; b <= nbins; ++b) {
        bins.T[b] = thresholds[b];
        if (b ? thresholds[b] <= thresholds[b - 1] : thresholds[0] < -1)
            return fail("nbe_pair_count: the thresholds must increase strictly from -1 or more");
    }
    // the cells must be at least isqrt(T_nb) + 1 units wide (the adjacency argument): ncell (s + 1) <= 2^30
    const long long room = (1LL << kCoordBits) / ncell - 1, top = bins.T[nbins];
    if (top < 0 || top >= (room + 1) * (room + 1))
        return fail("nbe_pair_count: threshold %lld needs cells wider than 2^30 / %d", top, ncell);
    const int s = (int)pair_isqrt(top);
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
    if (count < 1 || count > (1LL << 30)) return fail("nbe_pair_coords: bad particle count %lld", (long long)count);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize)) return fail("nbe_pair_coords: bad boxsize %g", boxsize);
    if (ncell < 3 || ncell > NBE_FOF_MAX_CELLS) return fail("nbe_pair_coords: ncell %d not in 3 .. %d", ncell, NBE_FOF_MAX_CELLS);
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

#endif
