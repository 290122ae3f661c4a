// The integer layer of the catalogue kernels (nbe_fof.hip, nbe_pairs.hip, nbe_profiles.hip, nbe_pairvel.hip; DESIGN.md
// sections 12.5, 12.7, 12.8, 12.9): coordinates, cells and keys, the union-find, the bin of a pair, the ranges of sorted
// records that a particle meets, the velocity moments of a pair and the per-row bodies of the coordinate and gather kernels.  Every function is inline and __host__ __device__ (or host
// only): no kernel, no entry point, no LDS, no wave intrinsic.  The kernels are loops around these bodies, and
// tools/catalog_host_walk.hip walks the same bodies serially on the host.
//
// Everything that decides a link or a bin is an integer.  A particle's coordinates are X_c = rint((i_c / n + psi_c / L) 2^30)
// mod 2^30 (float64, exact product), or rint((x_c / L) 2^30) mod 2^30 for a row of positions; the minimum-image difference
// d_c is (X_c(p) - X_c(q)) mod 2^30 mapped to [-2^29, 2^29); q = d_0^2 + d_1^2 + d_2^2 in 64-bit integers (below 2^60).  p
// and q are linked iff q <= R2.  With the thresholds T_0 < ... < T_nb a pair is in radial bin b iff T_b < q <= T_{b+1}
// ("<= T" is the FoF link rule), and with nmu > 1 in mu bin m = #{ j in 1 .. nmu - 1 : d_los^2 nmu^2 >= j^2 q } for q > 0,
// the two sides compared as 128-bit products, and m = 0 for q = 0.  A count is a sum of ones, so every grouping of the adds
// gives the same bits.  Particles are sorted (by the caller, with torch.sort) by the key of their cell, (X_c ncell) >> 30 per
// axis; the occupied cells are found by binary search in the sorted keys, so memory is O(particles) however fine the cell
// grid is.
//
// Adjacency.  ncell <= 2^30 / (s + 1) with s = isqrt(R2) or isqrt(T_nb), so a cell is at least s + 1 coordinate units wide.
// A pair with q <= s^2 + 2 s has |d_c| <= s on every axis, so x_c ncell / 2^30 of the two particles differ by less than 1
// (modulo ncell across the periodic face) and their floors by at most 1: such particles sit in the same cell or in cells
// adjacent with wrap-around.  ncell >= 3 makes the offsets -1, 0, +1 distinct modulo ncell, so of the two directions between
// a pair of adjacent cells exactly one is in the half set of 13 offsets that FoF and an auto count visit, and every
// candidate pair is tested once.  A cross count visits the 27 cells around a particle of A in the sorted B.  Cells of one
// (c0, c1) row that are consecutive in c2 are consecutive in the sorted keys and form one range; a row that crosses the
// periodic face in c2 adds a second one: at most 18 ranges (pair_range).
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
#pragma once

#include "../../include/nbe.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

namespace nbe {

// ---- coordinates, cells and keys ------------------------------------------------------------------------------------

constexpr int kCoordBits = 30;
constexpr int kCoordMask = (1 << kCoordBits) - 1;
constexpr double kCoordUnit = 1073741824.0;               // 2^30
constexpr double kMaxShift = 1048576.0;                   // |psi / L| at or beyond 2^20 boxes is rejected

struct FofParticle { int x0, x1, x2, p; };                // sorted order: coordinates and particle index, one 16-byte load

// X = rint((q + psi / L) 2^30) mod 2^30 with q = i / n; false for a non-finite or out-of-range displacement.  The product
// by 2^30 is exact, so no contraction can change the integer.
__host__ __device__ inline bool fof_coordinate(long long i, long long n, float psi, double L, int* X) {
    const double r = (double)psi / L;
    if (!(fabs(r) < kMaxShift)) return false;
    const double t = ((double)i / (double)n + r) * kCoordUnit;
    *X = (int)((long long)rint(t) & kCoordMask);
    return true;
}

// X = rint((x / L) 2^30) mod 2^30; false for a non-finite position or one 2^20 boxes or more away.  |t| < 2^50, and the
// two's-complement AND is the mathematical modulus.
__host__ __device__ inline bool pair_coordinate(double x, double L, int* X) {
    const double r = x / L;
    if (!(fabs(r) < kMaxShift)) return false;
    *X = (int)((long long)rint(r * kCoordUnit) & kCoordMask);
    return true;
}

__host__ __device__ inline float fof_load_real(const void* p, int half, long long i) {
    return half ? (float)((const _Float16*)p)[i] : ((const float*)p)[i];
}

__host__ __device__ inline double pair_load_real(const void* p, int wide, long long i) {
    return wide ? ((const double*)p)[i] : (double)((const float*)p)[i];
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

// ---- one row of a catalogue: what the coordinate and gather kernels do for their index ------------------------------

// row x of a catalogue of `count` rows gets its coordinates and the key of its cell; a bad row (ok = false) becomes 0, 0, 0
// and is counted in *bad, the caller's own counter
__host__ __device__ inline void catalog_store_row(bool ok, int X0, int X1, int X2, long long count, int ncell, long long x,
                                                  int* X, long long* keys, int* bad) {
    if (!ok) { ++*bad; X0 = X1 = X2 = 0; }
    X[x] = X0; X[count + x] = X1; X[2 * count + x] = X2;
    keys[x] = fof_key(fof_cell(X0, ncell), fof_cell(X1, ncell), fof_cell(X2, ncell), ncell);
}

// particle x of the n^3 lattice (count = n^3) with the displacement disp (3, n, n, n); also parent[x] = x
__host__ __device__ inline void fof_lattice_row(const void* disp, int half, long long n, long long count, double L, int ncell,
                                                long long x, int* X, long long* keys, int* parent, int* bad) {
    const long long i2 = x % n, rest = x / n, i1 = rest % n, i0 = rest / n;
    int X0 = 0, X1 = 0, X2 = 0;
    const bool ok = fof_coordinate(i0, n, fof_load_real(disp, half, x), L, &X0) &
                    fof_coordinate(i1, n, fof_load_real(disp, half, count + x), L, &X1) &
                    fof_coordinate(i2, n, fof_load_real(disp, half, 2 * count + x), L, &X2);
    catalog_store_row(ok, X0, X1, X2, count, ncell, x, X, keys, bad);
    parent[x] = (int)x;
}

// row x of the positions pos (count, 3)
__host__ __device__ inline void pair_position_row(const void* pos, int wide, long long count, double L, int ncell, long long x,
                                                  int* X, long long* keys, int* bad) {
    int X0 = 0, X1 = 0, X2 = 0;
    const bool ok = pair_coordinate(pair_load_real(pos, wide, 3 * x), L, &X0) &
                    pair_coordinate(pair_load_real(pos, wide, 3 * x + 1), L, &X1) &
                    pair_coordinate(pair_load_real(pos, wide, 3 * x + 2), L, &X2);
    catalog_store_row(ok, X0, X1, X2, count, ncell, x, X, keys, bad);
}

// the record at sorted position j: row order[j] with its coordinates
__host__ __device__ inline FofParticle fof_gather_record(const int* X, const long long* order, long long count, long long j) {
    const long long p = order[j];
    FofParticle o;
    o.x0 = X[p]; o.x1 = X[count + p]; o.x2 = X[2 * count + p]; o.p = (int)p;
    return o;
}

// ---- union-find ------------------------------------------------------------------------------------------------------

#if defined(__HIP_DEVICE_COMPILE__)
__device__ inline int parent_min(int* a, int v) { return atomicMin(a, v); }
__device__ inline int parent_load(const int* a) { return __hip_atomic_load(a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
#else
inline int parent_min(int* a, int v) { const int o = *a; if (v < o) *a = v; return o; }     // the serial host walk
inline int parent_load(const int* a) { return *a; }
#endif

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

// the integers a member x of the halo rooted at r adds to its sums: d_c(x, r), then rint(v_c 2^(24 - e_c))
__host__ __device__ inline void fof_terms(const int* X, long long count, long long x, int r, const void* vel, int vel_half,
                                          const int qexp[3], long long out[6]) {
    for (int c = 0; c < 3; ++c) out[c] = fof_diff(X[c * count + x], X[c * count + r]);
    for (int c = 0; c < 3; ++c)
        out[3 + c] = vel ? (long long)rint(ldexp((double)fof_load_real(vel, vel_half, c * count + x), qexp[c])) : 0;
}

// ---- the bin of a pair and the ranges of a particle -----------------------------------------------------------------

constexpr int kPairRanges = 18;                            // 9 rows of cells, each with its part across the periodic face
constexpr int kPairNoOrder = 0x7fffffff;                   // the sorted position of a record that any particle may meet

struct PairBins { long long T[NBE_PAIR_MAX_BINS + 1]; };   // the thresholds, passed by value

// isqrt of 0 <= v < 2^62
inline long long pair_isqrt(long long v) {
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

// range t of the 27 cells around the centre `me` in the sorted matter: rlo[t], rlen[t]
__host__ __device__ inline void profile_range(const FofParticle& me, const long long* skB, long long countB, int ncell, int t,
                                              long long* rlo, long long* rlen) {
    long long lo, hi;
    pair_range(skB, countB, fof_cell(me.x0, ncell), fof_cell(me.x1, ncell), fof_cell(me.x2, ncell), ncell, false, t, &lo, &hi);
    rlo[t] = lo; rlen[t] = hi - lo;
}

// The 18 ranges rlo[t], rlen[t] laid end to end: their total, and for record *q of 0 .. total - 1 the range t it lies in,
// with *q made its offset in that range: its sorted position is rlo[t] + *q.
__host__ __device__ inline long long pair_ranges_total(const long long* rlen) {
    long long total = 0;
    for (int t = 0; t < kPairRanges; ++t) total += rlen[t];
    return total;
}

__host__ __device__ inline int pair_ranges_locate(const long long* rlen, long long* q) {
    int t = 0;
    for (long long len = rlen[0]; *q >= len; len = rlen[++t]) *q -= len;
    return t;
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

// The particle at sorted position i of A against its ranges of B, one pair at a time (the "particles" form of the pair
// count, and the host walk): image[entry] += 1 through `add`.
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

// records first, first + step, ... of a centre's ranges laid end to end (the profile kernels): add(bin or -1) for each
template <typename Add>
__host__ __device__ inline void profile_stream(const FofParticle& me, const FofParticle* B, const long long* rlo,
                                               const long long* rlen, long long total, long long first, long long step,
                                               const long long* T, int nb, int s, Add add) {
    for (long long q = first; q < total; q += step) {
        long long at = q;
        const int t = pair_ranges_locate(rlen, &at);
        add(pair_bin(me, B[rlo[t] + at], T, nb, s, 1, 0));
    }
}

// ---- velocity moments of a pair (nbe_pairvel.hip) -------------------------------------------------
//
// One exponent e per call with max |v_c| < 2^e over every component of every catalogue of the call; W_c = rint(v_c 2^(20 - e)),
// |W_c| <= 2^20.  For a pair (a, o) with d_c = fof_diff(X_c(o), X_c(a)), q = sum d_c^2 > 0 and dW_c = W_c(o) - W_c(a)
// (|dW_c| <= 2^21): u = sum dW_c d_c, an exact 64-bit integer (|u| <= |dW| sqrt(q) < 2^52); the radial word is
// vr = sign(u) k with k = floor(|u| / sqrt(q) + 1/2), the k >= 0 with (2 k - 1)^2 q <= 4 u^2 < (2 k + 1)^2 q, decided by
// 128-bit products (k <= |dW| + 1/2 < 2^23, so both sides stay below 2^107); vr = 0 for q = 0.  |dW|^2 = sum dW_c^2 needs no
// rounding.  A tie 4 u^2 = (2 k + 1)^2 q cannot occur for u != 0 (section 12.9), and d -> -d, dW -> -dW leaves u alone: the
// terms of a pair do not depend on which of its rows is called a.

constexpr int kVelBits = NBE_VELOCITY_BITS;                // |W_c| <= 2^20
constexpr int kVelSplit = 24;                              // a square x < 2^44 is summed as x & (2^24 - 1) and x >> 24
constexpr int kVelSums = NBE_VELOCITY_SUMS;                              // per bin: N, S1, vr^2 lo, vr^2 hi, |dW|^2 lo, |dW|^2 hi

struct VelWord { int w0, w1, w2, pad; };                   // parallel to the sorted FofParticle records, one 16-byte load

// W = rint(v 2^(20 - e)); 0 for a value that is not finite or not below 2^e, which the caller has excluded
__host__ __device__ inline int velocity_word(double v, int e) {
    const double t = ldexp(v, kVelBits - e);
    return fabs(t) <= 1048576.0 ? (int)rint(t) : 0;
}

__host__ __device__ inline double velocity_load(const void* p, int dtype, long long i) {
    return dtype == NBE_F64 ? ((const double*)p)[i] : dtype == NBE_F16 ? (double)(float)((const _Float16*)p)[i]
                                                                       : (double)((const float*)p)[i];
}

// the velocity record at sorted position j: the words of row P[j].p of vel, which is (count, 3) row-major (lattice = 0) or
// (3, count) (lattice = 1)
__host__ __device__ inline VelWord velocity_gather_record(const void* vel, int dtype, int lattice, long long count, int e,
                                                          const FofParticle* P, long long j) {
    const long long p = P[j].p;
    VelWord w;
    w.w0 = velocity_word(velocity_load(vel, dtype, lattice ? p : 3 * p), e);
    w.w1 = velocity_word(velocity_load(vel, dtype, lattice ? count + p : 3 * p + 1), e);
    w.w2 = velocity_word(velocity_load(vel, dtype, lattice ? 2 * count + p : 3 * p + 2), e);
    w.pad = 0;
    return w;
}

struct PairVelocity { long long vr, vr2, dw2; };

// (2 k + j)^2 q <= 4 u^2 for j = -1 or +1 and 2 k + j >= 0, exactly
__host__ __device__ inline bool pair_vr_le(unsigned long long k, int j, unsigned long long q, unsigned long long au) {
    const unsigned long long m = 2 * k + j;
    return (unsigned __int128)(m * m) * q <= (unsigned __int128)(2 * au) * (2 * au);
}

// the terms of the pair (a, o) with the velocity records wa, wo (see above).  The float estimate of k only says where the
// exact comparisons start.
__host__ __device__ inline PairVelocity pair_velocity_terms(const FofParticle& a, const VelWord& wa, const FofParticle& o,
                                                            const VelWord& wo) {
    const long long d0 = fof_diff(o.x0, a.x0), d1 = fof_diff(o.x1, a.x1), d2 = fof_diff(o.x2, a.x2);
    const long long e0 = (long long)wo.w0 - wa.w0, e1 = (long long)wo.w1 - wa.w1, e2 = (long long)wo.w2 - wa.w2;
    PairVelocity r;
    r.dw2 = e0 * e0 + e1 * e1 + e2 * e2;
    r.vr = r.vr2 = 0;
    const unsigned long long q = (unsigned long long)(d0 * d0 + d1 * d1 + d2 * d2);
    const long long u = e0 * d0 + e1 * d1 + e2 * d2;
    if (q == 0 || u == 0) return r;
    const unsigned long long au = (unsigned long long)(u < 0 ? -u : u);
    unsigned long long k = (unsigned long long)((double)au / sqrt((double)q) + 0.5);
    while (k > 0 && !pair_vr_le(k, -1, q, au)) --k;       // (2 k - 1)^2 q <= 4 u^2
    while (pair_vr_le(k, 1, q, au)) ++k;                   // 4 u^2 < (2 k + 1)^2 q
    r.vr = u < 0 ? -(long long)k : (long long)k;
    r.vr2 = (long long)(k * k);
    return r;
}

// image[6 b ..] += (1, vr, vr^2 lo, vr^2 hi, |dW|^2 lo, |dW|^2 hi) through add(index, unsigned 64-bit word); the signed vr
// is added as its two's-complement word
template <typename Add>
__host__ __device__ inline void pair_velocity_add(int b, const PairVelocity& t, Add add) {
    const unsigned long long mask = (1ull << kVelSplit) - 1;
    add(kVelSums * b, 1ull);
    add(kVelSums * b + 1, (unsigned long long)t.vr);
    add(kVelSums * b + 2, (unsigned long long)t.vr2 & mask);
    add(kVelSums * b + 3, (unsigned long long)t.vr2 >> kVelSplit);
    add(kVelSums * b + 4, (unsigned long long)t.dw2 & mask);
    add(kVelSums * b + 5, (unsigned long long)t.dw2 >> kVelSplit);
}

// pair_count_particle with nmu = 1 and the velocity records VA, VB beside A, B: the record of B is read only for a pair
// that is in a bin
template <typename Add>
__host__ __device__ inline void pair_velocity_particle(const FofParticle* A, const VelWord* VA, long long i, const FofParticle* B,
                                                       const VelWord* VB, const long long* skB, long long countB, int ncell,
                                                       bool half, const long long* T, int nb, int s, Add add) {
    const FofParticle me = A[i];
    const VelWord mine = VA[i];
    const int c0 = fof_cell(me.x0, ncell), c1 = fof_cell(me.x1, ncell), c2 = fof_cell(me.x2, ncell);
    for (int t = 0; t < (half ? 10 : kPairRanges); ++t) {
        long long lo, hi;
        pair_range(skB, countB, c0, c1, c2, ncell, half, t, &lo, &hi);
        if (half && t == 0) lo = i + 1;                    // the rest of the own cell: i lies inside this range
        for (long long j = lo; j < hi; ++j) {
            const FofParticle o = B[j];
            const int b = pair_bin(me, o, T, nb, s, 1, 0);
            if (b >= 0) pair_velocity_add(b, pair_velocity_terms(me, mine, o, VB[j]), add);
        }
    }
}

// profile_stream with the velocity record `mine` of the centre (zero: the box frame) and VB beside B
template <typename Add>
__host__ __device__ inline void profile_velocity_stream(const FofParticle& me, const VelWord& mine, const FofParticle* B,
                                                        const VelWord* VB, const long long* rlo, const long long* rlen,
                                                        long long total, long long first, long long step, const long long* T,
                                                        int nb, int s, Add add) {
    for (long long q = first; q < total; q += step) {
        long long at = q;
        const int t = pair_ranges_locate(rlen, &at);
        const long long j = rlo[t] + at;
        const FofParticle o = B[j];
        const int b = pair_bin(me, o, T, nb, s, 1, 0);
        if (b >= 0) pair_velocity_add(b, pair_velocity_terms(me, mine, o, VB[j]), add);
    }
}

}  // namespace nbe
