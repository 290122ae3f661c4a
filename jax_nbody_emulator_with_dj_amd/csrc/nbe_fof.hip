// Friends-of-friends halos of an emulated box (include/nbe.h, "Halos").  Replaces the particle
// positions, the nbodykit FoF run and the halo sums of the reference's scripts/halos.py (:359-404, :407-450).  No context:
// these entry points need no weights.
//
// Everything that decides a link is an integer.  A particle's coordinates are X_c = rint((i_c / n + psi_c / L) 2^30) mod
// 2^30 (float64, exact product); the minimum-image difference d_c is (X_c(p) - X_c(q)) mod 2^30 mapped to [-2^29, 2^29);
// p and q are linked iff d_0^2 + d_1^2 + d_2^2 <= R2 in 64-bit integers.  Particles are sorted (by the caller, with
// torch.sort) by the key of their cell, (X_c ncell) >> 30 per axis; the occupied cells are found by binary search in the
// sorted keys, so memory is O(particles) however fine the cell grid is.
//
// Adjacency.  ncell <= 2^30 / (s + 1) with s = isqrt(R2), so a cell is at least s + 1 coordinate units wide.  A linked
// pair has |d_c| <= s on every axis, so x_c ncell / 2^30 of the two particles differ by less than 1 (modulo ncell across
// the periodic face) and their floors by at most 1: linked particles sit in the same cell or in cells adjacent with
// wrap-around.  ncell >= 3 makes the offsets -1, 0, +1 distinct modulo ncell, so of the two directions between a pair of
// adjacent cells exactly one is in the half set of 13 offsets that a thread visits, and every candidate pair is tested once.
//
// Union (fof_unite).  parent[] is a forest over particle indices with parent[x] <= x at all times: it starts as the
// identity and every write is an atomicMin with a value below x.  find follows the pointers with path halving; every step
// moves to a strictly smaller index, so it ends after at most x steps whatever other threads do.  To unite roots a > b a
// thread does old = atomicMin(&parent[a], b).  old == a: a was still a root and now hangs under b.  Otherwise a had
// already been hooked under old < a by someone else: whether or not the atomicMin lowered parent[a] to b, the sets of
// {a, old, b} are joined once old and b are, so the thread goes on with the pair (find(old), find(b)), whose larger
// member is below a.  The larger index of the pair falls strictly with every retry and stops at the latest when both are
// equal: no thread waits for another, and the bound does not depend on scheduling.  (This is the asynchronous union-find
// with min-hooking and path halving of Jayanti & Tarjan 2016 / ConnectIt, Dhulipala, Hong & Shun 2020.)  Section 12.5 has
// the argument that no link is lost.
//
// The per-particle bodies below are __host__ __device__ so that a stand-alone program can walk them serially on the host
// (tools/fof_host_walk.hip); only the wave reduction and the launches are device code.

#include "../../include/nbe.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace {

constexpr int kFofThreads = 256;
constexpr int kCoordBits = 30;
constexpr int kCoordMask = (1 << kCoordBits) - 1;
constexpr double kCoordUnit = 1073741824.0;               // 2^30
constexpr double kMaxShift = 1048576.0;                   // |psi / L| at or beyond 2^20 boxes is rejected

struct FofParticle { int x0, x1, x2, p; };                // sorted order: coordinates and particle index, one 16-byte load

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline int parent_min(int* a, int v) { return atomicMin(a, v); }
__device__ inline int parent_load(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
inline int parent_min(int* a, int v) { const int o = *a; if (v < o) *a = v; return o; }     // the serial host walk
inline int parent_load(const int* a) { return *a; }
#endif

// X = rint((q + psi / L) 2^30) mod 2^30 with q = i / n; false for a non-finite or out-of-range displacement.  The product
// by 2^30 is exact, so no contraction can change the integer.
__host__ __device__ inline bool fof_coordinate(long long i, long long n, float psi, double L, int* X) {
    const double r = (double)psi / L;
    if (!(fabs(r) < kMaxShift)) return false;
    const double t = ((double)i / (double)n + r) * kCoordUnit;
    *X = (int)((long long)rint(t) & kCoordMask);
    return true;
}

__host__ __device__ inline int fof_cell(int X, int ncell) { return (int)(((long long)X * ncell) >> kCoordBits); }

__host__ __device__ inline long long fof_key(int c0, int c1, int c2, int ncell) {
    return ((long long)c0 * ncell + c1) * ncell + c2;
}

// (a - b) mod 2^30 mapped to [-2^29, 2^29): a, b in [0, 2^30), so a - b + 2^29 stays inside an int
__host__ __device__ inline long long fof_diff(int a, int b) {
    return (long long)(((a - b + (1 << (kCoordBits - 1))) & kCoordMask) - (1 << (kCoordBits - 1)));
}

// first position in [from, n) whose key is >= key, given that every position before `from` holds a smaller key: gallops
// from `from`, then bisects
__host__ __device__ inline long long fof_lower_bound(const long long* sk, long long n, long long from, long long key) {
    if (from >= n || sk[from] >= key) return from;
    long long lo = from, step = 1;                         // sk[lo] < key
    while (lo + step < n && sk[lo + step] < key) { lo += step; step <<= 1; }
    long long hi = lo + step < n ? lo + step : n;          // the answer is in (lo, hi]
    while (hi - lo > 1) {
        const long long mid = lo + ((hi - lo) >> 1);
        if (sk[mid] < key) lo = mid; else hi = mid;
    }
    return hi;
}

// root of x with path halving.  Every value ever stored in parent[y] is <= y, so x falls strictly: at most x steps.
__host__ __device__ inline int fof_find(int* parent, int x) {
    for (;;) {
        const int p = parent_load(parent + x);
        if (p == x) return x;
        const int g = parent_load(parent + p);
        if (g == p) return p;
        parent_min(parent + x, g);                         // halving: x skips its parent
        x = g;
    }
}

// join the sets of p and q (see the head of the file): max(a, b) falls strictly with every retry
__host__ __device__ inline void fof_unite(int* parent, int p, int q) {
    int a = fof_find(parent, p), b = fof_find(parent, q);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = parent_min(parent + a, b);
        if (old == a) return;
        a = fof_find(parent, old);                         // old < a, and find never rises
        b = fof_find(parent, b);
    }
}

__host__ __device__ inline void fof_scan(const FofParticle* P, long long lo, long long hi, const FofParticle& me,
                                         long long R2, int* parent) {
    for (long long j = lo; j < hi; ++j) {
        const FofParticle o = P[j];
        const long long d0 = fof_diff(me.x0, o.x0), d1 = fof_diff(me.x1, o.x1), d2 = fof_diff(me.x2, o.x2);
        if (d0 * d0 + d1 * d1 + d2 * d2 <= R2) fof_unite(parent, me.p, o.p);
    }
}

// The particle at sorted position i against the later particles of its own cell and the particles of 13 of its 26
// neighbour cells: rows (o0, o1) = (0, 0) with o2 = +1, and (0, 1), (1, -1), (1, 0), (1, 1) with o2 = -1, 0, +1.  Cells
// of one row that are consecutive in c2 are consecutive in the sorted keys and are scanned as one range; a row that
// crosses the periodic face in c2 splits into two.
__host__ __device__ inline void fof_link_particle(const FofParticle* P, const long long* sk, long long count, long long i,
                                                  int ncell, long long R2, int* parent) {
    const FofParticle me = P[i];
    const int c0 = fof_cell(me.x0, ncell), c1 = fof_cell(me.x1, ncell), c2 = fof_cell(me.x2, ncell);
    const long long mine = fof_key(c0, c1, c2, ncell);
    {   // own row: the rest of the own cell, then the cell at c2 + 1
        const long long base = mine - c2;
        if (c2 + 1 < ncell) {
            fof_scan(P, i + 1, fof_lower_bound(sk, count, i + 1, mine + 2), me, R2, parent);
        } else {
            fof_scan(P, i + 1, fof_lower_bound(sk, count, i + 1, mine + 1), me, R2, parent);
            const long long lo = fof_lower_bound(sk, count, 0, base);
            fof_scan(P, lo, fof_lower_bound(sk, count, lo, base + 1), me, R2, parent);
        }
    }
    const int o0s[4] = {0, 1, 1, 1}, o1s[4] = {1, -1, 0, 1};
    for (int r = 0; r < 4; ++r) {
        int b0 = c0 + o0s[r], b1 = c1 + o1s[r];
        b0 = b0 >= ncell ? b0 - ncell : b0;
        b1 = b1 < 0 ? b1 + ncell : b1 >= ncell ? b1 - ncell : b1;
        const long long base = fof_key(b0, b1, 0, ncell);
        const long long from = base > mine ? i + 1 : 0;   // a row ahead in key order starts after i
        const int zlo = c2 > 0 ? c2 - 1 : 0, zhi = c2 + 1 < ncell ? c2 + 1 : ncell - 1;
        const long long lo = fof_lower_bound(sk, count, from, base + zlo);
        fof_scan(P, lo, fof_lower_bound(sk, count, lo, base + zhi + 1), me, R2, parent);
        if (c2 == 0 || c2 + 1 == ncell) {                  // the cell across the face: ncell >= 3 keeps it out of zlo .. zhi
            const long long w = base + (c2 == 0 ? ncell - 1 : 0);
            const long long wl = fof_lower_bound(sk, count, from, w);
            fof_scan(P, wl, fof_lower_bound(sk, count, wl, w + 1), me, R2, parent);
        }
    }
}

// after the link kernel has ended: the root of x, read-only (the caller stores it)
__host__ __device__ inline int fof_root(const int* parent, int x) {
    for (;;) {
        const int p = parent_load(parent + x);
        if (p == x) return x;
        x = p;
    }
}

__host__ __device__ inline float fof_load_real(const void* p, int half, long long i) {
    return half ? (float)((const _Float16*)p)[i] : ((const float*)p)[i];
}

// the integers a member x of the halo rooted at r adds to its sums: d_c(x, r), then rint(v_c 2^(24 - e_c))
__host__ __device__ inline void fof_terms(const int* X, long long count, long long x, int r, const void* vel, int vel_half,
                                          const int qexp[3], long long out[6]) {
    for (int c = 0; c < 3; ++c) out[c] = fof_diff(X[c * count + x], X[c * count + r]);
    for (int c = 0; c < 3; ++c)
        out[3 + c] = vel ? (long long)rint(ldexp((double)fof_load_real(vel, vel_half, c * count + x), qexp[c])) : 0;
}

#if defined(__HIPCC__)

struct FofExps { int q[3]; };

__global__ __launch_bounds__(kFofThreads) void fof_cells_kernel(const void* disp, int half, long long n, double L, int ncell,
                                                                int* __restrict__ X, long long* __restrict__ keys,
                                                                int* __restrict__ parent, int* __restrict__ stats) {
    const long long count = n * n * n;
    int bad = 0;
    for (long long x = blockIdx.x * (long long)blockDim.x + threadIdx.x; x < count; x += (long long)gridDim.x * blockDim.x) {
        const long long i2 = x % n, rest = x / n, i1 = rest % n, i0 = rest / n;
        int X0 = 0, X1 = 0, X2 = 0;
        const bool ok = fof_coordinate(i0, n, fof_load_real(disp, half, x), L, &X0) &
                        fof_coordinate(i1, n, fof_load_real(disp, half, count + x), L, &X1) &
                        fof_coordinate(i2, n, fof_load_real(disp, half, 2 * count + x), L, &X2);
        if (!ok) { ++bad; X0 = X1 = X2 = 0; }
        X[x] = X0; X[count + x] = X1; X[2 * count + x] = X2;
        keys[x] = fof_key(fof_cell(X0, ncell), fof_cell(X1, ncell), fof_cell(X2, ncell), ncell);
        parent[x] = (int)x;
    }
    if (bad) atomicAdd(&stats[0], bad);
}

__global__ __launch_bounds__(kFofThreads) void fof_gather_kernel(const int* __restrict__ X, const long long* __restrict__ order,
                                                                 long long count, FofParticle* __restrict__ P) {
    for (long long j = blockIdx.x * (long long)blockDim.x + threadIdx.x; j < count; j += (long long)gridDim.x * blockDim.x) {
        const long long p = order[j];
        FofParticle o;
        o.x0 = X[p]; o.x1 = X[count + p]; o.x2 = X[2 * count + p]; o.p = (int)p;
        P[j] = o;
    }
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

int fof_grid(long long count, int max_blocks) {
    const int g = grid_for(count, kFofThreads);
    return max_blocks > 0 && max_blocks < g ? max_blocks : g;
}

#endif  // __HIPCC__

}  // namespace

#if defined(__HIPCC__) && !defined(NBE_FOF_BODIES_ONLY)

extern "C" {

int nbe_fof_cells(const void* disp, int disp_dtype, int64_t n, double boxsize, int ncell, int max_blocks, void* coords,
                  void* keys, void* parent, void* stats, void* stream) {
    if (!disp || !coords || !keys || !parent || !stats) return fail("nbe_fof_cells: NULL argument");
    if (disp_dtype != NBE_F32 && disp_dtype != NBE_F16) return fail("nbe_fof_cells: dtype %d unsupported", disp_dtype);
    if (n < NBE_FOF_MIN_N || n > NBE_FOF_MAX_N)
        return fail("nbe_fof_cells: lattice size %lld unsupported (%d .. %d)", (long long)n, NBE_FOF_MIN_N, NBE_FOF_MAX_N);
    if (!(boxsize > 0.0) || !std::isfinite(boxsize)) return fail("nbe_fof_cells: bad boxsize %g", boxsize);
    if (ncell < 3 || ncell > NBE_FOF_MAX_CELLS) return fail("nbe_fof_cells: ncell %d not in 3 .. %d", ncell, NBE_FOF_MAX_CELLS);
    const long long count = (long long)n * n * n;
    hipLaunchKernelGGL(fof_cells_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream, disp,
                       disp_dtype == NBE_F16, (long long)n, boxsize, ncell, (int*)coords, (long long*)keys, (int*)parent,
                       (int*)stats);
    return launched("nbe_fof_cells");
}

int nbe_fof_gather(const void* coords, const void* order, int64_t count, int max_blocks, void* sorted, void* stream) {
    if (!coords || !order || !sorted) return fail("nbe_fof_gather: NULL argument");
    if (count < 1 || count > (1LL << 30)) return fail("nbe_fof_gather: bad particle count %lld", (long long)count);
    hipLaunchKernelGGL(fof_gather_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream,
                       (const int*)coords, (const long long*)order, (long long)count, (FofParticle*)sorted);
    return launched("nbe_fof_gather");
}

int nbe_fof_link(const void* sorted, const void* sorted_keys, int64_t count, int ncell, int64_t r2, int max_blocks,
                 void* parent, void* stream) {
    if (!sorted || !sorted_keys || !parent) return fail("nbe_fof_link: NULL argument");
    if (count < 1 || count > (1LL << 30)) return fail("nbe_fof_link: bad particle count %lld", (long long)count);
    if (ncell < 3 || ncell > NBE_FOF_MAX_CELLS) return fail("nbe_fof_link: ncell %d not in 3 .. %d", ncell, NBE_FOF_MAX_CELLS);
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
    if (count < 1 || count > (1LL << 30)) return fail("nbe_fof_labels: bad particle count %lld", (long long)count);
    hipLaunchKernelGGL(fof_labels_kernel, dim3(fof_grid(count, max_blocks)), dim3(kFofThreads), 0, (hipStream_t)stream,
                       (int*)parent, (long long)count, (int*)sizes);
    return launched("nbe_fof_labels");
}

int nbe_fof_catalog(const void* coords, const void* parent, const void* slot, const void* velocity, int velocity_dtype,
                    const int exponents[3], int64_t count, int wave_reduce, int max_blocks, void* sums, void* labels,
                    void* stream) {
    if (!coords || !parent || !slot || !sums) return fail("nbe_fof_catalog: NULL argument");
    if (count < 1 || count > (1LL << 30)) return fail("nbe_fof_catalog: bad particle count %lld", (long long)count);
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

#endif
