// Density fields from emulated displacements (include/nbe.h, "Density"): mass assignment of the displaced lattice onto
// a periodic mesh (NGP / CIC / TSC / PCS), the inverse assignment window on the rfft of the mesh, shell-binned power
// spectra with their multipoles and (k, mu) wedges, Minkowski functionals, the shell filter and triple sums of the
// bispectrum estimator and one-point statistics.
// Replaces the DISCO-DJ / Pylians step of the reference's pipeline (scripts/core.py:447-458, scripts/utils.py:136-148,
// :652-763, :1083-1085, :1164-1187, :1248-1274, :1314-1399, :1447-1449).  No context: these entry points need no weights.
//
// Paint.  One workgroup per Lagrangian tile of 8^3 particles.  Pass 1 reads the tile's
// displacements once and bounds its Eulerian footprint (the nodes its particles touch, from the tile's own positions).
// Pass 2 splits every particle's unit mass into fixed-point weights of 2^-22 (cumulative rounding: every weight is within
// one unit of the exact product of the 1-D B-splines and the weights of a particle sum to exactly 2^22) and adds them
// with 32-bit integer LDS atomics into an image of the footprint (512 particles * 2^22 = 2^31 fits an unsigned cell).
// Pass 3 flushes the non-zero cells with 64-bit integer atomics into the int64 mesh, row-major so that the lanes of a
// wave-instruction cover contiguous runs of a mesh row.  Integer adds commute: the mesh is bitwise independent of the
// order in which workgroups and lanes arrive.  A tile whose footprint exceeds the LDS image adds its weights straight
// into the global mesh (the same integers, so the same bits) and is counted in stats[0].
//
// Shared pieces, each written once.  Both moment entry points and the triple sums reduce with moments_pass_kernel<CENTRED,
// ORDER> / triple_sums_kernel, block_sum and sum_finish_kernel.  The spectral kernels decode a mode with half_mode
// (nbe_spectral.h, with fail, launched and grid_for, which nbe_lpt.hip shares) and
// the shell sums of the power spectrum and of the shell filter share power_exponent and shell_add.  upper_bound bins
// the Minkowski thresholds and the triangle counts; with_worder turns worder into a template argument.  The two
// painters (paint_kernel, paint_field_kernel) still carry their own copies of the tile pass: their positions are
// i a + psi s as the compiler contracts it, and moving that expression changes which product is fused.

#include "../../include/nbe.h"
#include "nbe_spectral.h"

#include <hip/hip_runtime.h>

#include <climits>
#include <cstdarg>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <type_traits>

namespace {

constexpr int kTile = 8;                                  // tile edge in particles
constexpr int kPaintThreads = 256;
constexpr int kPerThread = kTile * kTile * kTile / kPaintThreads;
constexpr int kLdsCells = 16384;                          // 64 KiB image: 2 workgroups per CU
constexpr double kUnit = 4194304.0;                       // 2^22 fixed-point units per particle mass
constexpr double kUMax = 1073741824.0;                    // |position| beyond 2^30 mesh cells is rejected

struct PaintArgs {
    const void* disp;
    long long n0, n1, n2;       // particle lattice
    double s0, s1, s2;          // mesh cells per unit of length (res_i / L_i)
    double a0, a1, a2;          // mesh cells per lattice step (res_i / N_i)
    int r0, r1, r2;             // mesh
    int tiles1, tiles2;
    unsigned long long* mesh;   // (r0, r1, r2) int64, zeroed by the caller
    int* stats;                 // [0] tiles on the direct path, [1] particles with a non-finite or huge position,
                                // [2:4] (int64) global 64-bit atomic adds when `count` is set (measurement only)
    int count;
};

__device__ inline int wrap(int j, int r) {
    int m = j % r;
    return m < 0 ? m + r : m;
}

// 1-D B-spline of order P in units of the mesh spacing: first node j0, weights of nodes j0 .. j0+P-1
template <int P>
__device__ inline int bspline(double u, double* w) {
    const double fl = floor(u + 1.0 - 0.5 * P);
    if (P == 1) {
        w[0] = 1.0;
    } else if (P == 2) {
        const double f = u - fl;
        w[0] = 1.0 - f; w[1] = f;
    } else if (P == 3) {
        const double d = u - fl - 1.0;                     // [-0.5, 0.5): offset from the middle node
        w[0] = 0.5 * (0.5 - d) * (0.5 - d); w[1] = 0.75 - d * d; w[2] = 0.5 * (0.5 + d) * (0.5 + d);
    } else {
        const double f = u - fl - 1.0, g = 1.0 - f;        // [0, 1): offset from the second node
        const double f2 = f * f, f3 = f2 * f;
        w[0] = g * g * g * (1.0 / 6.0);
        w[1] = (4.0 - 6.0 * f2 + 3.0 * f3) * (1.0 / 6.0);
        w[2] = (1.0 + 3.0 * f + 3.0 * f2 - 3.0 * f3) * (1.0 / 6.0);
        w[3] = f3 * (1.0 / 6.0);
    }
    return (int)fl;
}

// the P^3 fixed-point weights of one particle in (a, b, c) order; fn(a, b, c, q)
template <int P, typename F>
__device__ inline void particle_weights(const double* u, int* j0, F fn) {
    double wx[P], wy[P], wz[P];
    j0[0] = bspline<P>(u[0], wx);
    j0[1] = bspline<P>(u[1], wy);
    j0[2] = bspline<P>(u[2], wz);
    double S = 0.0;
    long long Qp = 0;
#pragma unroll
    for (int a = 0; a < P; ++a)
#pragma unroll
        for (int b = 0; b < P; ++b) {
            const double wab = wx[a] * wy[b];
#pragma unroll
            for (int c = 0; c < P; ++c) {
                S += wab * wz[c];
                const long long Q = (long long)rint(S * kUnit);     // the weights sum to round(2^22 * 1) = 2^22
                const unsigned q = (unsigned)(Q - Qp);
                Qp = Q;
                if (q) fn(a, b, c, q);
            }
        }
}

// true for a footprint of e0 x e1 x e2 nodes that does not fit an image of `cells` cells: the one place the painters
// decide the path.  (Each extent is tested first: the product of three extents of up to 2^31 cells does not fit 64 bits.)
__device__ inline bool beyond_image(long long e0, long long e1, long long e2, int cells) {
    return e0 > cells || e1 > cells || e2 > cells || e0 * e1 * e2 > cells;
}

// measurement builds of a call (count_atomics != 0): the workgroup's global atomic adds into stats[2:4]
__device__ inline void count_atomics(const PaintArgs& A, unsigned na, unsigned* shared) {
    atomicAdd(shared, na);
    __syncthreads();
    if (threadIdx.x == 0) atomicAdd((unsigned long long*)(A.stats + 2), (unsigned long long)*shared);
}

template <int P, bool HALF>
__global__ __launch_bounds__(kPaintThreads) void paint_kernel(PaintArgs A) {
    __shared__ unsigned img[kLdsCells];
    __shared__ int lo[3], hi[3];
    __shared__ unsigned natomic;
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x;
    const int t2 = (int)(tile % A.tiles2);
    const long long rest = tile / A.tiles2;
    const int t1 = (int)(rest % A.tiles1), t0 = (int)(rest / A.tiles1);
    if (tid < 3) { lo[tid] = INT_MAX; hi[tid] = INT_MIN; }
    if (tid == 0) natomic = 0u;
    __syncthreads();

    const long long ncell = A.n0 * A.n1 * A.n2;
    double u[kPerThread][3];
    bool live[kPerThread];
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int l = tid + k * kPaintThreads;
        const long long i0 = t0 * kTile + (l >> 6), i1 = t1 * kTile + ((l >> 3) & 7), i2 = t2 * kTile + (l & 7);
        live[k] = i0 < A.n0 && i1 < A.n1 && i2 < A.n2;
        if (!live[k]) continue;
        const long long idx = (i0 * A.n1 + i1) * A.n2 + i2;
        float p0, p1, p2;
        if (HALF) {
            const _Float16* d = (const _Float16*)A.disp;
            p0 = (float)d[idx]; p1 = (float)d[ncell + idx]; p2 = (float)d[2 * ncell + idx];
        } else {
            const float* d = (const float*)A.disp;
            p0 = d[idx]; p1 = d[ncell + idx]; p2 = d[2 * ncell + idx];
        }
        // lattice q = i L / N, position q + psi, in mesh units (periodic wrap applied per node)
        u[k][0] = (double)i0 * A.a0 + (double)p0 * A.s0;
        u[k][1] = (double)i1 * A.a1 + (double)p1 * A.s1;
        u[k][2] = (double)i2 * A.a2 + (double)p2 * A.s2;
        if (!(fabs(u[k][0]) < kUMax && fabs(u[k][1]) < kUMax && fabs(u[k][2]) < kUMax)) {
            live[k] = false;
            atomicAdd(&A.stats[1], 1);
            continue;
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int j = (int)floor(u[k][c] + 1.0 - 0.5 * P);
            mn[c] = min(mn[c], j);
            mx[c] = max(mx[c], j + P - 1);
        }
    }
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (mn[c] != INT_MAX) { atomicMin(&lo[c], mn[c]); atomicMax(&hi[c], mx[c]); }
    }
    __syncthreads();
    if (hi[0] < lo[0]) return;                             // no live particle in this tile (uniform)

    const long long e0 = (long long)hi[0] - lo[0] + 1, e1 = (long long)hi[1] - lo[1] + 1,
                    e2 = (long long)hi[2] - lo[2] + 1;
    const int r0 = A.r0, r1 = A.r1, r2 = A.r2;
    if (beyond_image(e0, e1, e2, kLdsCells)) {
        // footprint larger than the image: the same integer weights straight into the mesh
        if (tid == 0) atomicAdd(&A.stats[0], 1);
        unsigned na = 0;
#pragma unroll
        for (int k = 0; k < kPerThread; ++k) {
            if (!live[k]) continue;
            int j0[3];
            particle_weights<P>(u[k], j0, [&](int a, int b, int c, unsigned q) {
                const long long g = ((long long)wrap(j0[0] + a, r0) * r1 + wrap(j0[1] + b, r1)) * r2 + wrap(j0[2] + c, r2);
                atomicAdd(&A.mesh[g], (unsigned long long)q);
                ++na;
            });
        }
        if (A.count) count_atomics(A, na, &natomic);
        return;
    }

    const int E1 = (int)e1, E2 = (int)e2, vol = (int)(e0 * e1 * e2);
    const int l0 = lo[0], l1 = lo[1], l2 = lo[2];
    for (int i = tid; i < vol; i += kPaintThreads) img[i] = 0u;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        if (!live[k]) continue;
        int j0[3];
        particle_weights<P>(u[k], j0, [&](int a, int b, int c, unsigned q) {
            atomicAdd(&img[((j0[0] + a - l0) * E1 + (j0[1] + b - l1)) * E2 + (j0[2] + c - l2)], q);
        });
    }
    __syncthreads();
    unsigned na = 0;
    for (int i = tid; i < vol; i += kPaintThreads) {
        const unsigned v = img[i];
        if (!v) continue;
        const int c2 = i % E2, r = i / E2, c1 = r % E1, c0 = r / E1;
        const long long g = ((long long)wrap(l0 + c0, r0) * r1 + wrap(l1 + c1, r1)) * r2 + wrap(l2 + c2, r2);
        atomicAdd(&A.mesh[g], (unsigned long long)v);
        ++na;
    }
    if (A.count) count_atomics(A, na, &natomic);
}

__global__ void mesh_to_delta_kernel(const long long* __restrict__ mesh, float* __restrict__ out, long long n,
                                     double scale) {
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = (float)((double)mesh[i] * scale - 1.0);
}

// ---- Per-particle fields --------------------------------------------------------------------
// Weighted mass assignment: besides its unit mass every particle carries up to NBE_PAINT_MAX_CHANNELS quantities, each as
// an integer V = rint(q 2^(24 - e_c)) with |V| <= 2^24 (e_c: the channel's binary exponent, max |q_c| < 2^e_c, from
// quantity_range_kernel).  A cell sums w V over its particles in 64-bit integers with the weights w of particle_weights
// (two's complement: unsigned adds wrap correctly), so the sums are bitwise independent of scheduling, of the path a tile
// takes and of the other channels.  Positions may be shifted along one axis by a second field (redshift space), and
// disp == NULL paints the undisplaced lattice.
//
// LDS: a tile adds up to 512 * 2^22 * 2^24 = 2^55 to a cell, so the image has 64-bit cells; 8192 of them keep the 64 KiB
// and the two workgroups per CU of paint_kernel.  The one image is reused pass by pass (the mass, then each channel);
// positions and the V stay in registers and the weights are recomputed per pass.  A footprint beyond 8192 cells takes the
// direct path: the same integers into the global meshes, all channels in one sweep over the weights.
constexpr int kFieldCells = 8192;
constexpr long long kMassLimit = 1LL << 39;               // a cell at or above it could overflow |S| <= M 2^24 < 2^63

struct FieldArgs {
    const void* disp;           // (3, N0, N1, N2), or NULL: the undisplaced lattice
    const void* qty;            // (nchan, N0, N1, N2)
    const void* shift;          // (N0, N1, N2) added along axis `los` after scaling by vs, or NULL
    int disp_half, qty_half, shift_half, nchan, los;
    double vs;                  // mesh cells per unit of the shift field
    long long n0, n1, n2;
    double s0, s1, s2;
    double a0, a1, a2;
    int r0, r1, r2;
    int tiles1, tiles2;
    int qexp[NBE_PAINT_MAX_CHANNELS];   // 24 - e_c
    unsigned long long* mesh;   // (r0, r1, r2) int64 masses, zeroed by the caller
    unsigned long long* qmesh;  // (nchan, r0, r1, r2) int64 sums of w V, zeroed by the caller
    int* stats;                 // [0] tiles on the direct path, [1] particles with a non-finite or huge position
};

__device__ inline float load_real(const void* p, int half, long long i) {
    return half ? (float)((const _Float16*)p)[i] : ((const float*)p)[i];
}

// What paint_field_kernel and paint_particles_kernel do once the positions u, the integers V and the footprint of a
// workgroup's 512 particles are known (two per thread): the meshes, and the two ways into them.
struct FieldMeshes {
    unsigned long long* mesh;
    unsigned long long* qmesh;
    long long cells;
    int r0, r1, r2, nchan;
};

// a thread's node bounds mn, mx (INT_MAX: no live particle) into the workgroup's lo, hi; false if nothing is live (uniform)
__device__ inline bool merge_footprint(const int* mn, const int* mx, int* lo, int* hi) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        if (mn[c] != INT_MAX) { atomicMin(&lo[c], mn[c]); atomicMax(&hi[c], mx[c]); }
    }
    __syncthreads();
    return hi[0] >= lo[0];
}

// footprint larger than the image: one particle's integers straight into the meshes
template <int P>
__device__ inline void direct_add(const FieldMeshes& M, const double* uk, const int* Vk) {
    const int r0 = M.r0, r1 = M.r1, r2 = M.r2, nchan = M.nchan;
    const long long cells = M.cells;
    int j0[3];
    particle_weights<P>(uk, j0, [&](int a, int b, int c, unsigned q) {
        const long long g = ((long long)wrap(j0[0] + a, r0) * r1 + wrap(j0[1] + b, r1)) * r2 + wrap(j0[2] + c, r2);
        atomicAdd(&M.mesh[g], (unsigned long long)q);
        if (0 < nchan && Vk[0]) atomicAdd(&M.qmesh[g], (unsigned long long)((long long)q * Vk[0]));
        if (1 < nchan && Vk[1]) atomicAdd(&M.qmesh[cells + g], (unsigned long long)((long long)q * Vk[1]));
        if (2 < nchan && Vk[2]) atomicAdd(&M.qmesh[2 * cells + g], (unsigned long long)((long long)q * Vk[2]));
        if (3 < nchan && Vk[3]) atomicAdd(&M.qmesh[3 * cells + g], (unsigned long long)((long long)q * Vk[3]));
    });
}

// the mass, then one channel per pass through the one image of the footprint lo .. hi (at most kFieldCells cells), each
// flushed row-major with 64-bit atomics
template <int P>
__device__ inline void image_passes(const FieldMeshes& M, unsigned long long* img, const int* lo, const int* hi,
                                    double (*u)[3], const int (*V)[NBE_PAINT_MAX_CHANNELS], const bool* live) {
    static_assert(kPerThread == 2, "the scatter steps below name both particles of a thread");
    const int tid = threadIdx.x;
    const int r0 = M.r0, r1 = M.r1, r2 = M.r2;
    const int l0 = lo[0], l1 = lo[1], l2 = lo[2];
    const int E1 = hi[1] - l1 + 1, E2 = hi[2] - l2 + 1, vol = (hi[0] - l0 + 1) * E1 * E2;
    for (int pass = 0; pass <= M.nchan; ++pass) {
        for (int i = tid; i < vol; i += kPaintThreads) img[i] = 0ull;
        __syncthreads();
        auto scatter = [&](double* uk, const int* Vk) {
            const int v = pass == 0 ? 1 : pass == 1 ? Vk[0] : pass == 2 ? Vk[1] : pass == 3 ? Vk[2] : Vk[3];
            if (!v) return;
            // keeps the weights from being computed ahead of the pass loop and held in ~2 P^3 registers
            asm volatile("" : "+v"(uk[0]), "+v"(uk[1]), "+v"(uk[2]));
            int j0[3];
            particle_weights<P>(uk, j0, [&](int a, int b, int c, unsigned q) {
                atomicAdd(&img[((j0[0] + a - l0) * E1 + (j0[1] + b - l1)) * E2 + (j0[2] + c - l2)],
                          (unsigned long long)((long long)q * v));
            });
        };
        if (live[0]) scatter(u[0], V[0]);
        if (live[1]) scatter(u[1], V[1]);
        __syncthreads();
        unsigned long long* dst = pass == 0 ? M.mesh : M.qmesh + (pass - 1) * M.cells;
        for (int i = tid; i < vol; i += kPaintThreads) {
            const unsigned long long v = img[i];
            if (!v) continue;
            const int c2 = i % E2, r = i / E2, c1 = r % E1, c0 = r / E1;
            const long long g = ((long long)wrap(l0 + c0, r0) * r1 + wrap(l1 + c1, r1)) * r2 + wrap(l2 + c2, r2);
            atomicAdd(&dst[g], v);
        }
        __syncthreads();
    }
}

template <int P>
__global__ __launch_bounds__(kPaintThreads) void paint_field_kernel(FieldArgs A) {
    __shared__ unsigned long long img[kFieldCells];
    __shared__ int lo[3], hi[3];
    const int tid = threadIdx.x;
    const long long tile = blockIdx.x;
    const int t2 = (int)(tile % A.tiles2);
    const long long rest = tile / A.tiles2;
    const int t1 = (int)(rest % A.tiles1), t0 = (int)(rest / A.tiles1);
    if (tid < 3) { lo[tid] = INT_MAX; hi[tid] = INT_MIN; }
    __syncthreads();

    const long long ncell = A.n0 * A.n1 * A.n2;
    const int nchan = A.nchan;
    double u[kPerThread][3];
    int V[kPerThread][NBE_PAINT_MAX_CHANNELS];
    bool live[kPerThread];
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const int l = tid + k * kPaintThreads;
        const long long i0 = t0 * kTile + (l >> 6), i1 = t1 * kTile + ((l >> 3) & 7), i2 = t2 * kTile + (l & 7);
        live[k] = i0 < A.n0 && i1 < A.n1 && i2 < A.n2;
#pragma unroll
        for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c) V[k][c] = 0;
        if (!live[k]) continue;
        const long long idx = (i0 * A.n1 + i1) * A.n2 + i2;
        float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
        if (A.disp) {
            p0 = load_real(A.disp, A.disp_half, idx);
            p1 = load_real(A.disp, A.disp_half, ncell + idx);
            p2 = load_real(A.disp, A.disp_half, 2 * ncell + idx);
        }
        // as paint_kernel; along the line of sight i a + psi s + v vs, all in float64
        u[k][0] = (double)i0 * A.a0 + (double)p0 * A.s0;
        u[k][1] = (double)i1 * A.a1 + (double)p1 * A.s1;
        u[k][2] = (double)i2 * A.a2 + (double)p2 * A.s2;
        if (A.shift) {
            const double d = (double)load_real(A.shift, A.shift_half, idx) * A.vs;
            if (A.los == 0) u[k][0] += d;
            else if (A.los == 1) u[k][1] += d;
            else u[k][2] += d;
        }
        if (!(fabs(u[k][0]) < kUMax && fabs(u[k][1]) < kUMax && fabs(u[k][2]) < kUMax)) {
            live[k] = false;
            atomicAdd(&A.stats[1], 1);
            continue;
        }
#pragma unroll
        for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c)
            if (c < nchan)
                V[k][c] = (int)rint(ldexp((double)load_real(A.qty, A.qty_half, c * ncell + idx), A.qexp[c]));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int j = (int)floor(u[k][c] + 1.0 - 0.5 * P);
            mn[c] = min(mn[c], j);
            mx[c] = max(mx[c], j + P - 1);
        }
    }
    if (!merge_footprint(mn, mx, lo, hi)) return;          // no live particle in this tile

    const FieldMeshes M = {A.mesh, A.qmesh, (long long)A.r0 * A.r1 * A.r2, A.r0, A.r1, A.r2, nchan};
    if (beyond_image((long long)hi[0] - lo[0] + 1, (long long)hi[1] - lo[1] + 1, (long long)hi[2] - lo[2] + 1,
                     kFieldCells)) {
        if (tid == 0) atomicAdd(&A.stats[0], 1);
        if (live[0]) direct_add<P>(M, u[0], V[0]);
        if (live[1]) direct_add<P>(M, u[1], V[1]);
        return;
    }
    image_passes<P>(M, img, lo, hi, u, V, live);
}

// ---- Particle catalogues --------------------------------------------------------------------
// The integer scheme of paint_field_kernel for explicit positions: halos, a subsample, an N-body snapshot.  A workgroup
// takes a chunk of kChunk consecutive entries of `order` (the last chunk is ragged) and follows the three passes above:
// its footprint from its own particles, the LDS image where that fits, the direct path where it does not.  Which chunk a
// particle falls into changes the path only, never an integer that is added: the meshes are the same bits for every
// order.  particle_keys_kernel gives the order that keeps consecutive chunks compact.
constexpr int kChunk = kPaintThreads * kPerThread;

struct PositionArgs {
    const void* pos;            // (count, 3) float32 or float64
    const void* shift;          // (count,) added along axis `los` after scaling by vs, or NULL
    int pos_f64, shift_half, los;
    double vs;                  // mesh cells per unit of the shift
    double s0, s1, s2;          // mesh cells per unit of length (res_i / L_i)
    long long count;
};

struct ParticleArgs {
    PositionArgs pos;
    const long long* order;     // (count,) permutation, or NULL: the identity
    const void* qty;            // (nchan, count)
    int qty_half, nchan;
    int r0, r1, r2;
    int qexp[NBE_PAINT_MAX_CHANNELS];   // 24 - e_c
    unsigned long long* mesh;   // as FieldArgs
    unsigned long long* qmesh;
    int* stats;                 // [0] chunks on the direct path, [1] particles with a non-finite or huge position
};

// u = x (res / L) in float64, plus the shift along its axis; false for a position that is not painted
__device__ inline bool particle_position(const PositionArgs& A, long long idx, double* u) {
    if (A.pos_f64) {
        const double* x = (const double*)A.pos + 3 * idx;
        u[0] = x[0] * A.s0; u[1] = x[1] * A.s1; u[2] = x[2] * A.s2;
    } else {
        const float* x = (const float*)A.pos + 3 * idx;
        u[0] = (double)x[0] * A.s0; u[1] = (double)x[1] * A.s1; u[2] = (double)x[2] * A.s2;
    }
    if (A.shift) {
        const double d = (double)load_real(A.shift, A.shift_half, idx) * A.vs;
        if (A.los == 0) u[0] += d;
        else if (A.los == 1) u[1] += d;
        else u[2] += d;
    }
    return fabs(u[0]) < kUMax && fabs(u[1]) < kUMax && fabs(u[2]) < kUMax;
}

template <int P>
__global__ __launch_bounds__(kPaintThreads) void paint_particles_kernel(ParticleArgs A) {
    __shared__ unsigned long long img[kFieldCells];
    __shared__ int lo[3], hi[3];
    const int tid = threadIdx.x;
    if (tid < 3) { lo[tid] = INT_MAX; hi[tid] = INT_MIN; }
    __syncthreads();

    const long long count = A.pos.count;
    const int nchan = A.nchan;
    double u[kPerThread][3];
    int V[kPerThread][NBE_PAINT_MAX_CHANNELS];
    bool live[kPerThread];
    int mn[3] = {INT_MAX, INT_MAX, INT_MAX}, mx[3] = {INT_MIN, INT_MIN, INT_MIN};
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
        const long long e = (long long)blockIdx.x * kChunk + tid + k * kPaintThreads;
        live[k] = e < count;
#pragma unroll
        for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c) V[k][c] = 0;
        if (!live[k]) continue;
        const long long idx = A.order ? A.order[e] : e;
        // (an entry of `order` outside 0 .. count-1 reads nothing and is counted with the rejected particles)
        if (idx < 0 || idx >= count || !particle_position(A.pos, idx, u[k])) {
            live[k] = false;
            atomicAdd(&A.stats[1], 1);
            continue;
        }
#pragma unroll
        for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c)
            if (c < nchan)
                V[k][c] = (int)rint(ldexp((double)load_real(A.qty, A.qty_half, c * count + idx), A.qexp[c]));
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const int j = (int)floor(u[k][c] + 1.0 - 0.5 * P);
            mn[c] = min(mn[c], j);
            mx[c] = max(mx[c], j + P - 1);
        }
    }
    if (!merge_footprint(mn, mx, lo, hi)) return;          // no live particle in this chunk

    const FieldMeshes M = {A.mesh, A.qmesh, (long long)A.r0 * A.r1 * A.r2, A.r0, A.r1, A.r2, nchan};
    if (beyond_image((long long)hi[0] - lo[0] + 1, (long long)hi[1] - lo[1] + 1, (long long)hi[2] - lo[2] + 1,
                     kFieldCells)) {
        if (tid == 0) atomicAdd(&A.stats[0], 1);
        if (live[0]) direct_add<P>(M, u[0], V[0]);
        if (live[1]) direct_add<P>(M, u[1], V[1]);
        return;
    }
    image_passes<P>(M, img, lo, hi, u, V, live);
}

// bits of x spread to every third position (x < 2^20)
__device__ inline unsigned long long spread3(unsigned long long x) {
    x = (x | x << 32) & 0x1f00000000ffffull;
    x = (x | x << 16) & 0x1f0000ff0000ffull;
    x = (x | x << 8) & 0x100f00f00f00f00full;
    x = (x | x << 4) & 0x10c30c30c30c30c3ull;
    x = (x | x << 2) & 0x1249249249249249ull;
    return x;
}

// keys[p] = the index of the mesh tile (edge^3 cells) that holds the periodically reduced node floor(u) of particle p:
// row-major over the tiles, or with MORTON their interleaved bits; LLONG_MAX for a particle that would not be painted.
// (A template, so that it is emitted after the painters: a kernel emitted ahead of paint_kernel moves that kernel in the
// code object, and its PCS instance then measured 1 % slower with the same instructions)
template <bool MORTON>
__global__ __launch_bounds__(256) void particle_keys_kernel(PositionArgs A, int r0, int r1, int r2, int edge,
                                                            long long* __restrict__ keys) {
    const long long T1 = (r1 + edge - 1) / edge, T2 = (r2 + edge - 1) / edge;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < A.count; i += (long long)gridDim.x * blockDim.x) {
        double u[3];
        long long key = LLONG_MAX;
        if (particle_position(A, i, u)) {
            const long long t0 = wrap((int)floor(u[0]), r0) / edge, t1 = wrap((int)floor(u[1]), r1) / edge,
                            t2 = wrap((int)floor(u[2]), r2) / edge;
            key = MORTON ? (long long)(spread3(t0) << 2 | spread3(t1) << 1 | spread3(t2)) : (t0 * T1 + t1) * T2 + t2;
        }
        keys[i] = key;
    }
}

// ---- Mesh readout --------------------------------------------------------------------------
// The adjoint of the painters: out_c(p) = 2^-22 sum of q f_c[node] over the fixed-point weights q that the painters add for
// particle p (particle_weights, which sum to exactly 2^22), in float64 in that function's (a, b, c) order and rounded to
// float32 once.  q <= 2^22 times a float32 is exact in float64, so fusing the product into the add changes nothing.  A
// thread takes a row and reads its P^3 nodes, wrapped as the painters wrap them, for every channel; no atomics on the
// output, one writer per word: the same bits for every grid and order.  Rows are those of the painters: entry e of `order`
// (or e itself) of a catalogue through particle_position, or particle e of the lattice through paint_field_kernel's
// expression.  (A template like particle_keys_kernel, so that it is emitted after the painters.)
struct ReadArgs {
    PositionArgs pos;           // a catalogue (pos.pos != NULL), or
    const void* disp;           // the lattice n0 x n1 x n2 displaced by (3, N0, N1, N2), or bare (NULL)
    int disp_half;
    long long n0, n1, n2;
    double a0, a1, a2;          // mesh cells per lattice step
    const long long* order;     // catalogue only: (count,) or NULL
    const float* field;         // (nchan, r0, r1, r2)
    float* out;                 // (nchan, count)
    int nchan, r0, r1, r2;
    float fill;
    int* stats;                 // [1] rows that are not read
};

template <int P>
__global__ __launch_bounds__(256) void mesh_read_kernel(ReadArgs A) {
    const long long count = A.pos.count, cells = (long long)A.r0 * A.r1 * A.r2;
    const int r0 = A.r0, r1 = A.r1, r2 = A.r2, nchan = A.nchan;
    for (long long e = blockIdx.x * (long long)blockDim.x + threadIdx.x; e < count; e += (long long)gridDim.x * blockDim.x) {
        double u[3];
        long long idx = e;
        bool live;
        if (A.pos.pos) {
            if (A.order) idx = A.order[e];
            if (idx < 0 || idx >= count) {                 // nothing to read and no row to write
                atomicAdd(&A.stats[1], 1);
                continue;
            }
            live = particle_position(A.pos, idx, u);
        } else {
            const long long i2 = e % A.n2, rest = e / A.n2, i1 = rest % A.n1, i0 = rest / A.n1;
            float p0 = 0.0f, p1 = 0.0f, p2 = 0.0f;
            if (A.disp) {
                p0 = load_real(A.disp, A.disp_half, idx);
                p1 = load_real(A.disp, A.disp_half, count + idx);
                p2 = load_real(A.disp, A.disp_half, 2 * count + idx);
            }
            u[0] = (double)i0 * A.a0 + (double)p0 * A.pos.s0;
            u[1] = (double)i1 * A.a1 + (double)p1 * A.pos.s1;
            u[2] = (double)i2 * A.a2 + (double)p2 * A.pos.s2;
            live = fabs(u[0]) < kUMax && fabs(u[1]) < kUMax && fabs(u[2]) < kUMax;
        }
        if (!live) {
            atomicAdd(&A.stats[1], 1);
#pragma unroll
            for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c)
                if (c < nchan) A.out[c * count + idx] = A.fill;
            continue;
        }
        double acc[NBE_PAINT_MAX_CHANNELS] = {0.0, 0.0, 0.0, 0.0};
        int j0[3];
        particle_weights<P>(u, j0, [&](int a, int b, int c, unsigned q) {
            const long long g = ((long long)wrap(j0[0] + a, r0) * r1 + wrap(j0[1] + b, r1)) * r2 + wrap(j0[2] + c, r2);
            const double w = (double)q;
#pragma unroll
            for (int ch = 0; ch < NBE_PAINT_MAX_CHANNELS; ++ch)
                if (ch < nchan) acc[ch] += w * (double)A.field[ch * cells + g];
        });
#pragma unroll
        for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c)
            if (c < nchan) A.out[c * count + idx] = (float)(acc[c] * (1.0 / kUnit));
    }
}

// per channel: the largest |q| as float bits (unsigned order = float order for non-negative floats; atomicMax commutes)
// in range[c], and the number of non-finite values of all channels in range[nchan]
__global__ __launch_bounds__(256) void quantity_range_kernel(const void* q, int half, int nchan, long long count,
                                                             unsigned* __restrict__ range) {
    __shared__ unsigned smax[NBE_PAINT_MAX_CHANNELS], sbad;
    if (threadIdx.x < NBE_PAINT_MAX_CHANNELS) smax[threadIdx.x] = 0u;
    if (threadIdx.x == 0) sbad = 0u;
    __syncthreads();
    unsigned bad = 0;
    for (int c = 0; c < nchan; ++c) {
        unsigned m = 0u;
        for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < count; i += (long long)gridDim.x * blockDim.x) {
            const float v = load_real(q, half, c * count + i);
            if (!isfinite(v)) ++bad;
            else m = max(m, __float_as_uint(fabsf(v)));
        }
        if (m) atomicMax(&smax[c], m);
    }
    if (bad) atomicAdd(&sbad, bad);
    __syncthreads();
    if ((int)threadIdx.x < nchan && smax[threadIdx.x]) atomicMax(&range[threadIdx.x], smax[threadIdx.x]);
    if (threadIdx.x == 0 && sbad) atomicAdd(&range[nchan], sbad);
}

struct ToFieldArgs {
    const long long* mesh;
    const long long* qmesh;
    float* out;
    long long cells;
    int nchan, mode;
    int e[NBE_PAINT_MAX_CHANNELS];
    double ratio;               // n_cells / N_p
    float fill;
    int* stats;                 // [2] cells whose mass reaches kMassLimit
};

// float64 throughout, one rounding to float32: mean S 2^(e - 46) n_cells / N_p, density S 2^(e - 24) / M (fill at M = 0)
__global__ void mesh_to_field_kernel(ToFieldArgs A) {
    int over = 0;
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < A.cells; i += (long long)gridDim.x * blockDim.x) {
        const long long M = A.mesh[i];
        if (M >= kMassLimit) ++over;
        for (int c = 0; c < A.nchan; ++c) {
            const double S = (double)A.qmesh[c * A.cells + i];
            float v;
            if (A.mode == NBE_FIELD_MEAN) v = (float)(ldexp(S, A.e[c] - 46) * A.ratio);
            else v = M == 0 ? A.fill : (float)(ldexp(S, A.e[c] - 24) / (double)M);
            A.out[c * A.cells + i] = v;
        }
    }
    if (over) atomicAdd(&A.stats[2], over);
}

__device__ inline double sinc_pi(long long f, long long n) {            // sinc(pi f / n), sinc(x) = sin(x) / x
    if (f == 0) return 1.0;
    const double x = (double)f / (double)n;
    return sinpi(x) / (3.141592653589793 * x);
}

template <int P>
__global__ void deconvolve_kernel(float2* __restrict__ f, long long r0, long long r1, long long r2) {
    const long long n = r0 * r1 * (r2 / 2 + 1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const HalfMode m = half_mode(i, r0, r1, r2);
        const double w = sinc_pi(m.f0, r0) * sinc_pi(m.f1, r1) * sinc_pi(m.f2, r2);
        double wp = w;
#pragma unroll
        for (int p = 1; p < P; ++p) wp *= w;
        const double inv = 1.0 / wp;
        float2 v = f[i];
        v.x = (float)(v.x * inv);
        v.y = (float)(v.y * inv);
        f[i] = v;
    }
}

// Shell sums, shared by the power spectrum and the shell filter.  A first pass finds the largest |term| of each shell as
// float bits (unsigned order = float order for non-negative floats; atomicMax commutes): binmax = m 2^e, m in [0.5, 1).
// The second adds, per shell and in integers, the weights, w (|k| / k_F - offset) in the shell's k unit and w term in
// units of 2^(e - 32), so that every term is at most 2^32 units.
// the power exponent 32 - e of a binmax word; INT_MIN: non-finite shell, reported by the caller
__device__ inline int power_exponent(unsigned binmax) {
    const float m = __uint_as_float(binmax);
    int e = 0;
    if (isfinite(m) && m > 0.0f) frexp((double)m, &e);
    return isfinite(m) ? 32 - e : INT_MIN;
}

// a term in the shell's power unit 2^(e - 32); 0 in a non-finite shell
__device__ inline long long power_units(double p, int pexp) {
    return pexp == INT_MIN ? 0 : (long long)rint(ldexp(p, pexp));
}

// one mode into the LDS triple t[0], t[stride], t[2 stride] of its shell: weight, k, power
__device__ inline void shell_add(unsigned long long* t, int stride, int w, long long kq, double p, int pexp) {
    const long long pq = power_units(p, pexp);
    atomicAdd(t, (unsigned long long)w);
    atomicAdd(t + stride, (unsigned long long)(w * kq));
    atomicAdd(t + 2 * stride, (unsigned long long)(w * pq));
}

// One mode of the half spectrum of an n^3 mesh: shell b (0 = not binned), full-grid weight, |k| / k_F, Re(a b*)
struct Mode { int b; int w; double kk; double p; };

__device__ inline Mode mode_of(const HalfMode& h, const float2* a, const float2* bb, long long i, long long n) {
    Mode m;
    m.kk = sqrt((double)h.q);
    m.b = (int)floor(m.kk + 0.5);
    if (m.b < 1 || m.b > n / 2) { m.b = 0; return m; }
    m.w = h.w;
    const float2 x = a[i], y = bb ? bb[i] : x;
    m.p = (double)x.x * y.x + (double)x.y * y.y;
    return m;
}

__device__ inline Mode mode_at(const float2* a, const float2* bb, long long i, long long n) {
    return mode_of(half_mode(i, n, n, n), a, bb, i, n);
}

// pass 1: per-shell max |Re(a b*)|
__global__ void pk_max_kernel(const float2* __restrict__ a, const float2* __restrict__ b, long long n,
                              unsigned* __restrict__ binmax) {
    extern __shared__ unsigned smax[];
    const int nb = (int)(n / 2) + 1;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) smax[i] = 0u;
    __syncthreads();
    const long long total = n * n * (n / 2 + 1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Mode m = mode_at(a, b, i, n);
        if (m.b) atomicMax(&smax[m.b], __float_as_uint((float)fabs(m.p)));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += blockDim.x)
        if (smax[i]) atomicMax(&binmax[i], smax[i]);
}

// pass 2: every mode binned by rint(|k| / k_F); k in units of 2^-36 about the shell's index
constexpr double kKUnit = 68719476736.0;                  // 2^36
__global__ void pk_sum_kernel(const float2* __restrict__ a, const float2* __restrict__ b, long long n,
                              const unsigned* __restrict__ binmax, unsigned long long* __restrict__ sums) {
    extern __shared__ unsigned long long ssum[];           // [3][nb]: weight, k, power
    const int nb = (int)(n / 2) + 1;
    int* sexp = (int*)(ssum + 3 * nb);
    for (int i = threadIdx.x; i < 3 * nb; i += blockDim.x) ssum[i] = 0ull;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) sexp[i] = power_exponent(binmax[i]);
    __syncthreads();
    const long long total = n * n * (n / 2 + 1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const Mode m = mode_at(a, b, i, n);
        if (m.b) shell_add(ssum + m.b, nb, m.w, (long long)rint((m.kk - m.b) * kKUnit), m.p, sexp[m.b]);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * nb; i += blockDim.x)
        if (ssum[i]) atomicAdd(&sums[i], ssum[i]);
}

// ---- Anisotropic shell sums -----------------------------------------------------------------
// Multipoles and (k, mu) wedges about the array axis `los`: the shells, weights, terms and exponents of the two passes
// above (pass 1 is pk_max_kernel itself), with mu^2 = m_los^2 / |m|^2.  Only even powers of mu enter, so neither the sign
// of m_los nor the mirror modes the half spectrum leaves out along axis 2 matter.
__device__ inline long long los_freq(const HalfMode& h, int los) { return los == 0 ? h.f0 : los == 1 ? h.f1 : h.f2; }

// pass 2 of the multipoles: per shell the weights, k, and the terms times L_0 = 1, L_2 and L_4 in the shell's power unit
__global__ void pk_multipole_kernel(const float2* __restrict__ a, const float2* __restrict__ b, long long n, int los,
                                    const unsigned* __restrict__ binmax, unsigned long long* __restrict__ sums) {
    extern __shared__ unsigned long long ssum[];           // [5][nb]: weight, k, L0, L2, L4
    const int nb = (int)(n / 2) + 1;
    int* sexp = (int*)(ssum + 5 * nb);
    for (int i = threadIdx.x; i < 5 * nb; i += blockDim.x) ssum[i] = 0ull;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) sexp[i] = power_exponent(binmax[i]);
    __syncthreads();
    const long long total = n * n * (n / 2 + 1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const HalfMode h = half_mode(i, n, n, n);
        const Mode m = mode_of(h, a, b, i, n);
        if (!m.b) continue;
        const long long f = los_freq(h, los);
        const double mu2 = (double)(f * f) / (double)h.q;
        const double l2 = (3.0 * mu2 - 1.0) / 2.0, l4 = (35.0 * (mu2 * mu2) - 30.0 * mu2 + 3.0) / 8.0;
        unsigned long long* t = ssum + m.b;
        const int pexp = sexp[m.b];
        shell_add(t, nb, m.w, (long long)rint((m.kk - m.b) * kKUnit), m.p, pexp);
        atomicAdd(t + 3 * nb, (unsigned long long)(m.w * power_units(m.p * l2, pexp)));
        atomicAdd(t + 4 * nb, (unsigned long long)(m.w * power_units(m.p * l4, pexp)));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 5 * nb; i += blockDim.x)
        if (ssum[i]) atomicAdd(&sums[i], ssum[i]);
}

// The wedge of a mode: min(nmu - 1, #{ j in 1 .. nmu-1 : j^2 q <= nmu^2 f^2 }) = floor(nmu |mu|) with mu = 1 in the last
// bin.  The float64 quotient is a first guess only; the integers decide (nmu <= 64, q < 2^23: every product < 2^35).
__device__ inline int mu_bin(long long f, long long q, int nmu, double kk) {
    const long long af = f < 0 ? -f : f, t = (long long)nmu * nmu * af * af;
    int j = (int)((double)(nmu * af) / kk);
    j = j > nmu - 1 ? nmu - 1 : j;
    while (j > 0 && (long long)j * j * q > t) --j;
    while (j < nmu - 1 && (long long)(j + 1) * (j + 1) * q <= t) ++j;
    return j;
}

// pass 2 of the wedges, for the mu bins mu0 <= j < mu1 (an image of 4 (mu1 - mu0) nb words); a mode of another bin is
// skipped once its bin is known.  sums is [word][mu][s] over all nmu bins.
__global__ void pk_wedge_kernel(const float2* __restrict__ a, const float2* __restrict__ b, long long n, int los, int nmu,
                                int mu0, int mu1, const unsigned* __restrict__ binmax,
                                unsigned long long* __restrict__ sums) {
    extern __shared__ unsigned long long ssum[];           // [4][mu1 - mu0][nb]: weight, k, |mu|, power
    const int nb = (int)(n / 2) + 1, bins = (mu1 - mu0) * nb;
    int* sexp = (int*)(ssum + 4 * bins);
    for (int i = threadIdx.x; i < 4 * bins; i += blockDim.x) ssum[i] = 0ull;
    for (int i = threadIdx.x; i < nb; i += blockDim.x) sexp[i] = power_exponent(binmax[i]);
    __syncthreads();
    const long long total = n * n * (n / 2 + 1);
    for (long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const HalfMode h = half_mode(i, n, n, n);
        const Mode m = mode_of(h, a, b, i, n);
        if (!m.b) continue;
        const long long f = los_freq(h, los);
        const int j = mu_bin(f, h.q, nmu, m.kk);
        if (j < mu0 || j >= mu1) continue;
        const double mu = (double)(f < 0 ? -f : f) / m.kk;
        unsigned long long* t = ssum + (j - mu0) * nb + m.b;
        atomicAdd(t, (unsigned long long)m.w);
        atomicAdd(t + bins, (unsigned long long)(m.w * (long long)rint((m.kk - m.b) * kKUnit)));
        atomicAdd(t + 2 * bins, (unsigned long long)(m.w * (long long)rint(mu * kKUnit)));
        atomicAdd(t + 3 * bins, (unsigned long long)(m.w * power_units(m.p, sexp[m.b])));
    }
    __syncthreads();
    for (int i = threadIdx.x; i < 4 * bins; i += blockDim.x)
        if (ssum[i]) {
            const int word = i / bins, r = i - word * bins;
            atomicAdd(&sums[((long long)word * nmu + mu0) * nb + r], ssum[i]);
        }
}

// ---- Minkowski functionals ------------------------------------------------------------------
// Moments (nbe_field_moments, and to the fourth order nbe_field_moments4): two passes in float64 (the sum, then the sums
// of powers of the deviation from the mean), each over a fixed partition of the voxels into mom_blocks(total) *
// kMomThreads strided runs, reduced in a fixed order by one block.
constexpr int kMomThreads = 256;
constexpr int kMomMaxBlocks = NBE_MOMENTS_WORDS - 2;

int mom_blocks(long long total) {
    const long long b = (total + 8 * kMomThreads - 1) / (8 * kMomThreads);
    return (int)(b < kMomMaxBlocks ? b : kMomMaxBlocks);
}

// Fixed-step upper_bound: #{a[i] <= v} over the n sorted values of a (LDS); top = top_step(n).  A NaN v gives 0.
__device__ inline int top_step(int n) {
    int top = 1;
    while (2 * top <= n) top *= 2;
    return top;
}

template <typename T>
__device__ inline int upper_bound(const T* a, int n, int top, T v) {
    int pos = 0;
    for (int step = top; step > 0; step >>= 1)
        if (pos + step <= n && a[pos + step - 1] <= v) pos += step;
    return pos;
}

// the block's sum of v over its threads, in a fixed tree order; valid in thread 0
__device__ inline double block_sum(double v, double* red) {
    red[threadIdx.x] = v;
    __syncthreads();
    for (int s = kMomThreads / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) red[threadIdx.x] += red[threadIdx.x + s];
        __syncthreads();
    }
    return red[0];
}

// One pass over a field: block b's sums of x (CENTRED = false), or of the powers 2 .. ORDER of d = x - *mean, into
// partial[(p - 2) * kMomMaxBlocks + b].  Each ORDER keeps its own expression: the compiler contracts `a2 += d * d` and
// `d2 = d * d; a2 += d2` differently, and one ulp of the ORDER 2 std can move a voxel across a Minkowski threshold.
template <bool CENTRED, int ORDER>
__global__ __launch_bounds__(kMomThreads) void moments_pass_kernel(const float* __restrict__ x, long long total,
                                                                   const double* mean_at, double* partial) {
    static_assert(ORDER == 2 || ORDER == 4, "the variance alone, or the central moments to the fourth");
    __shared__ double red[kMomThreads];
    const double mean = CENTRED ? *mean_at : 0.0;
    const long long stride = (long long)gridDim.x * kMomThreads;
    double a2 = 0.0, a3 = 0.0, a4 = 0.0;
    auto add = [&](float v) {
        if (!CENTRED) {
            a2 += v;
        } else if (ORDER == 2) {
            const double d = v - mean;
            a2 += d * d;
        } else {
            const double d = v - mean, d2 = d * d;
            a2 += d2; a3 += d2 * d; a4 += d2 * d2;
        }
    };
    long long i = (long long)blockIdx.x * kMomThreads + threadIdx.x;
    for (; i + 3 * stride < total; i += 4 * stride) {        // four loads in flight, added in index order
        const float a = x[i], b = x[i + stride], c = x[i + 2 * stride], d = x[i + 3 * stride];
        add(a); add(b); add(c); add(d);
    }
    for (; i < total; i += stride) add(x[i]);
    const double s2 = block_sum(a2, red);
    if (threadIdx.x == 0) partial[blockIdx.x] = s2;
    if (!CENTRED || ORDER == 2) return;
    __syncthreads();
    const double s3 = block_sum(a3, red);
    if (threadIdx.x == 0) partial[kMomMaxBlocks + blockIdx.x] = s3;
    __syncthreads();
    const double s4 = block_sum(a4, red);
    if (threadIdx.x == 0) partial[2 * kMomMaxBlocks + blockIdx.x] = s4;
}

// block j: out[j] = the sum of the nb partials of row j (rows of `row` words) in a fixed order; with total != 0 divided
// by it, and with root its square root after that
__global__ __launch_bounds__(kMomThreads) void sum_finish_kernel(const double* partial, long long row, int nb, double* out,
                                                                 long long total, int root) {
    __shared__ double red[kMomThreads];
    double acc = 0.0;
    for (int b = threadIdx.x; b < nb; b += kMomThreads) acc += partial[blockIdx.x * row + b];
    double s = block_sum(acc, red);
    if (total) s = s / (double)total;
    if (threadIdx.x == 0) out[blockIdx.x] = root ? sqrt(s) : s;
}

// Counts: one pass.  Each voxel v owns the 8 elements at its low corner (1 cube, 3 faces, 3 edges, 1 vertex); an element
// is in the excursion set {w >= t} iff the largest w of its 1, 2, 4 or 8 voxels is >= t.  bin(w) = #{thresholds <= w}
// (upper_bound over the sorted thresholds) is monotone, so an element's bin is the largest bin of its voxels, and one
// histogram of element bins per functional holds the counts of every threshold: count(t_k) = sum of bins > k.
//
// A workgroup sweeps a column of kMfJ x kMfK voxels (j, k) along i, kMfI planes at a time.  Every plane is read once from
// HBM with a one-voxel low-side halo in j and k (wrapped), standardized and binned as it is loaded, and stored as 16-bit
// bins in LDS (double-buffered); the bins of the previous plane stay in registers.  A wave covers one row of 64 voxels
// along k, 4 rows of j per wave.
constexpr int kMfThreads = 256;
constexpr int kMfJ = 16, kMfK = 64, kMfI = 32;
constexpr int kMfRowLen = kMfK + 1, kMfPlane = (kMfJ + 1) * kMfRowLen;    // 17 x 65 bins with the halo
constexpr int kMfLoads = (kMfPlane + kMfThreads - 1) / kMfThreads;        // 5 plane positions per thread
constexpr int kMfBins = NBE_MF_MAX_THRESHOLDS + 1;
#ifndef NBE_MF_UNIFORM
#define NBE_MF_UNIFORM 1   // 0: every lane adds on its own (timing probes of the histogram layout only)
#endif

static_assert(kMfThreads == 4 * kMfK && kMfJ == 16, "a wave covers one row of k, four rows of j per wave");

// Add w (1 .. 3) to h[b] for every active lane.  When every active lane of the wave has the same bin, their weights are
// summed with two ballots into one LDS add; otherwise each lane adds its own.  A constant field, and the flat parts of a
// smooth one, put a whole row of 64 lanes on one bin: one add instead of 64 same-address LDS atomics, for one compare
// and one ballot on the other rows (DESIGN.md section 12.1 has the measurements).
__device__ inline void hist_add(unsigned* h, int b, unsigned w) {
#if NBE_MF_UNIFORM
    const int lead = __builtin_amdgcn_readfirstlane(b);
    if (__ballot(b != lead) == 0ull) {
        const unsigned long long m1 = __ballot(w & 1u), m2 = __ballot(w & 2u);
        if (__lane_id() == (unsigned)__builtin_amdgcn_readfirstlane((int)__lane_id()))
            atomicAdd(&h[lead], (unsigned)(__popcll(m1) + 2 * __popcll(m2)));
        return;
    }
#endif
    atomicAdd(&h[b], w);
}

// the three bins of one functional's elements of a voxel (faces or edges): equal bins of one lane go in one add
__device__ inline void hist_add3(unsigned* h, int a, int b, int c) {
    hist_add(h, a, 1u + (b == a) + (c == a));
    if (b != a) hist_add(h, b, 1u + (c == b));
    if (c != a && c != b) hist_add(h, c, 1u);
}

struct MfArgs {
    const float* x;
    long long n;
    const float* thr;              // sorted ascending, T values
    int T;
    const double* mom;             // NULL: w = x; else w = (x - float(mom[0])) / float(mom[1]) (0 where that std is 0)
    unsigned long long* counts;    // 4 (T+1) histograms (vertices, edges, faces, cubes) + non-finite voxels
    int nj, nk, ni;                // column / segment counts
    long long items;
};

__global__ __launch_bounds__(kMfThreads) void minkowski_counts_kernel(MfArgs A) {
    __shared__ float thr[NBE_MF_MAX_THRESHOLDS];
    __shared__ unsigned hist[4 * kMfBins];
    __shared__ unsigned short bins[2][kMfPlane];
    __shared__ unsigned nonfinite;
    const int tid = threadIdx.x, T = A.T, NB = 4 * (T + 1);
    const int n = (int)A.n;
    for (int i = tid; i < T; i += kMfThreads) thr[i] = A.thr[i];
    for (int i = tid; i < NB; i += kMfThreads) hist[i] = 0u;
    if (tid == 0) nonfinite = 0u;
    const int top = top_step(T);
    const bool stdz = A.mom != nullptr;
    float mf = 0.0f, sf = 0.0f;
    if (stdz) { mf = (float)A.mom[0]; sf = (float)A.mom[1]; }
    const long long plane = A.n * A.n;
    __syncthreads();

    // bin of one value: standardized with correctly rounded float32 subtraction and division (no reciprocal, nothing to
    // contract), then the number of thresholds <= w (NaN: 0; the caller rejects the field)
    auto bin_of = [&](float v) -> int {
        float w = v;
        if (stdz) w = sf == 0.0f ? 0.0f : __fdiv_rn(__fsub_rn(v, mf), sf);
        return upper_bound(thr, T, top, w);
    };

    const int wv = tid >> 6, kl = tid & 63;         // this thread's voxels: (j0 + 4 wv + r, k0 + kl), r = 0 .. 3
    unsigned bad = 0;
    int buf = 0;
    for (long long item = blockIdx.x; item < A.items; item += gridDim.x) {
        const int si = (int)(item % A.ni);
        const long long rest = item / A.ni;
        const int sk = (int)(rest % A.nk), sj = (int)(rest / A.nk);
        const int j0 = sj * kMfJ, k0 = sk * kMfK, i0 = si * kMfI, i1 = min(i0 + kMfI, n);
        // this thread's plane positions: in-plane offsets (< n^2 <= 2^22) and whether the position is a voxel of the column
        int off[kMfLoads];
        bool own[kMfLoads];
#pragma unroll
        for (int q = 0; q < kMfLoads; ++q) {
            const int p = tid + q * kMfThreads;
            const int jj = p / kMfRowLen, kk = p % kMfRowLen;
            const int j = ((j0 - 1 + jj) % n + n) % n, k = ((k0 - 1 + kk) % n + n) % n;
            off[q] = p < kMfPlane ? j * n + k : 0;
            own[q] = p < kMfPlane && jj >= 1 && kk >= 1 && j0 + jj - 1 < n && k0 + kk - 1 < n;
        }
        float raw[kMfLoads];
        auto load = [&](int i) {
            const float* src = A.x + (long long)i * plane;
#pragma unroll
            for (int q = 0; q < kMfLoads; ++q) raw[q] = (tid + q * kMfThreads < kMfPlane) ? src[off[q]] : 0.0f;
        };
        auto store = [&](bool count) {
#pragma unroll
            for (int q = 0; q < kMfLoads; ++q) {
                const int p = tid + q * kMfThreads;
                if (p < kMfPlane) {
                    bins[buf][p] = (unsigned short)bin_of(raw[q]);
                    if (count && own[q] && !isfinite(raw[q])) ++bad;
                }
            }
        };
        // rows 4 wv .. 4 wv + 4 of the halo'd plane at columns kl (c = 0) and kl + 1 (c = 1)
        int prev[5][2], cur[5][2];
        auto read = [&](int (*dst)[2]) {
#pragma unroll
            for (int r = 0; r < 5; ++r) {
                dst[r][0] = bins[buf][(4 * wv + r) * kMfRowLen + kl];
                dst[r][1] = bins[buf][(4 * wv + r) * kMfRowLen + kl + 1];
            }
        };
        load(i0 == 0 ? n - 1 : i0 - 1);               // the halo plane below the segment, wrapped
        store(false);
        __syncthreads();
        read(prev);
        buf ^= 1;
        load(i0);
        for (int i = i0; i < i1; ++i) {
            store(true);
            if (i + 1 < i1) load(i + 1);               // in flight while this plane is counted
            __syncthreads();
            read(cur);
            buf ^= 1;
            if (k0 + kl < n) {
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    if (j0 + 4 * wv + r >= n) break;
                    const int b000 = cur[r + 1][1], b001 = cur[r + 1][0], b010 = cur[r][1], b011 = cur[r][0];
                    const int b100 = prev[r + 1][1], b101 = prev[r + 1][0], b110 = prev[r][1], b111 = prev[r][0];
                    const int e0 = max(max(b000, b010), max(b001, b011));          // edge along i: v, v-e_j, v-e_k, v-e_j-e_k
                    const int e1 = max(max(b000, b100), max(b001, b101));          // edge along j
                    const int e2 = max(max(b000, b100), max(b010, b110));          // edge along k
                    const int vx = max(max(e0, max(b100, b101)), max(b110, b111));
                    hist_add(hist + 0 * (T + 1), vx, 1u);
                    hist_add3(hist + 1 * (T + 1), e0, e1, e2);
                    hist_add3(hist + 2 * (T + 1), max(b000, b100), max(b000, b010), max(b000, b001));
                    hist_add(hist + 3 * (T + 1), b000, 1u);
                }
            }
#pragma unroll
            for (int r = 0; r < 5; ++r) { prev[r][0] = cur[r][0]; prev[r][1] = cur[r][1]; }
        }
    }
    if (bad) atomicAdd(&nonfinite, bad);
    __syncthreads();
    for (int i = tid; i < NB; i += kMfThreads)
        if (hist[i]) atomicAdd(&A.counts[i], (unsigned long long)hist[i]);
    if (tid == 0 && nonfinite) atomicAdd(&A.counts[NB], (unsigned long long)nonfinite);
}

// ---- Bispectrum and one-point statistics ----------------------------------------------------
// Shell filter: one pass over the half spectrum of an n^3 mesh serves a batch of S spherical shells.  Every mode forms its
// integer |m|^2 once and tests it against the batch's [lo2, hi2) bounds (integers, prepared by the host); shell s receives
// the mode or 0 in its own filtered spectrum.  The bounds are symmetric under m -> -m, so the filtered half spectra stay
// Hermitian.  The per-shell sums use the shell-sum scheme above, with |m| - koff in units of 2^-kexp.
constexpr int kBkThreads = 256;

struct ShellArgs {
    const float2* spec;
    long long n;
    const long long* par;          // device, S x 4: lo2, hi2, koff, kexp
    int S;
    float2* out;                   // S filtered half spectra, or NULL
    unsigned* binmax;              // S, or NULL (no sums)
    unsigned long long* sums;      // S x 3: weight, k, power
};

__global__ __launch_bounds__(kBkThreads) void shell_max_kernel(ShellArgs A) {
    __shared__ long long lo2[NBE_BK_MAX_SHELLS], hi2[NBE_BK_MAX_SHELLS];
    __shared__ unsigned smax[NBE_BK_MAX_SHELLS];
    __shared__ long long qmin, qmax;
    const int S = A.S;
    for (int s = threadIdx.x; s < S; s += kBkThreads) { lo2[s] = A.par[4 * s]; hi2[s] = A.par[4 * s + 1]; smax[s] = 0u; }
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = LLONG_MAX, b = 0;
        for (int s = 0; s < S; ++s) { a = lo2[s] < a ? lo2[s] : a; b = hi2[s] > b ? hi2[s] : b; }
        qmin = a; qmax = b;
    }
    __syncthreads();
    const long long total = A.n * A.n * (A.n / 2 + 1), q0 = qmin, q1 = qmax;
    for (long long i = blockIdx.x * (long long)kBkThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kBkThreads) {
        const long long q = half_mode(i, A.n, A.n, A.n).q;
        if (q < q0 || q >= q1) continue;
        const float2 v = A.spec[i];
        const unsigned bits = __float_as_uint((float)fabs((double)v.x * v.x + (double)v.y * v.y));
        for (int s = 0; s < S; ++s)
            if (q >= lo2[s] && q < hi2[s]) atomicMax(&smax[s], bits);
    }
    __syncthreads();
    for (int s = threadIdx.x; s < S; s += kBkThreads)
        if (smax[s]) atomicMax(&A.binmax[s], smax[s]);
}

__global__ __launch_bounds__(kBkThreads) void shell_filter_kernel(ShellArgs A) {
    __shared__ long long lo2[NBE_BK_MAX_SHELLS], hi2[NBE_BK_MAX_SHELLS];
    __shared__ double koff[NBE_BK_MAX_SHELLS];
    __shared__ int kexp[NBE_BK_MAX_SHELLS], pexp[NBE_BK_MAX_SHELLS];
    __shared__ unsigned long long ssum[3 * NBE_BK_MAX_SHELLS];
    const int S = A.S;
    const bool sums = A.binmax != nullptr;
    for (int s = threadIdx.x; s < S; s += kBkThreads) {
        lo2[s] = A.par[4 * s]; hi2[s] = A.par[4 * s + 1];
        koff[s] = (double)A.par[4 * s + 2]; kexp[s] = (int)A.par[4 * s + 3];
        ssum[3 * s] = ssum[3 * s + 1] = ssum[3 * s + 2] = 0ull;
        pexp[s] = sums ? power_exponent(A.binmax[s]) : INT_MIN;
    }
    __syncthreads();
    const long long total = A.n * A.n * (A.n / 2 + 1);
    for (long long i = blockIdx.x * (long long)kBkThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kBkThreads) {
        const HalfMode m = half_mode(i, A.n, A.n, A.n);
        const long long q = m.q;
        const float2 v = A.spec[i];
        const float2 zero = make_float2(0.0f, 0.0f);
        for (int s = 0; s < S; ++s) {
            const bool in = q >= lo2[s] && q < hi2[s];
            if (A.out) A.out[(long long)s * total + i] = in ? v : zero;
            if (in && sums) {
                const double p = (double)v.x * v.x + (double)v.y * v.y;
                shell_add(ssum + 3 * s, 1, m.w, (long long)rint(ldexp(sqrt((double)q) - koff[s], kexp[s])), p, pexp[s]);
            }
        }
    }
    if (!sums) return;
    __syncthreads();
    for (int i = threadIdx.x; i < 3 * S; i += kBkThreads)
        if (ssum[i]) atomicAdd(&A.sums[i], ssum[i]);
}

// Triple sums: out[j] = sum over the voxels of f1 f2 f3_j in float64.  The voxels are cut into mom_blocks(total) *
// kMomThreads strided runs (a function of the mesh size only); every run is added in index order with one fused
// multiply-add per voxel, the runs of a block in block_sum's tree and the blocks by one workgroup of sum_finish_kernel.
// The result of field j therefore does not depend on which other fields share its launch.
constexpr int kTsFields = 8;

struct TripleArgs {
    const float* f1;
    const float* f2;
    const float* f3[kTsFields];
    int nj;
    long long total;
    double* partial;               // kTsFields rows of NBE_BK_PARTIALS
};

__global__ __launch_bounds__(kMomThreads) void triple_sums_kernel(TripleArgs A) {
    __shared__ double red[kMomThreads];
    double acc[kTsFields];
#pragma unroll
    for (int j = 0; j < kTsFields; ++j) acc[j] = 0.0;
    const long long stride = (long long)gridDim.x * kMomThreads;
    for (long long i = (long long)blockIdx.x * kMomThreads + threadIdx.x; i < A.total; i += stride) {
        const double p = (double)A.f1[i] * (double)A.f2[i];           // exact: 48 bits
#pragma unroll
        for (int j = 0; j < kTsFields; ++j)
            if (j < A.nj) acc[j] = fma(p, (double)A.f3[j][i], acc[j]);
    }
#pragma unroll
    for (int j = 0; j < kTsFields; ++j) {
        if (j >= A.nj) break;
        const double s = block_sum(acc[j], red);
        if (threadIdx.x == 0) A.partial[(long long)j * NBE_BK_PARTIALS + blockIdx.x] = s;
        __syncthreads();
    }
}

// Triangle counts: every pair (m1, m2) of the modes of shells 1 and 2 closes with m3 = -(m1 + m2); |m3|^2 is binned by
// upper_bound over the K sorted distinct bounds of the third shells, and the count of a shell [lo2, hi2) is the sum of
// the bins between its two bounds.  Integers throughout: exact at every mesh size.
constexpr int kPcChunk = 1024;

struct PairArgs {
    const int4* m1; long long c1;
    const int4* m2; long long c2;
    const int* edges; int K;
    unsigned long long* hist;      // K + 1
    long long tiles2;
};

__global__ __launch_bounds__(kBkThreads) void pair_count_kernel(PairArgs A) {
    __shared__ int4 chunk[kPcChunk];
    __shared__ int edges[NBE_BK_MAX_EDGES];
    __shared__ unsigned hist[NBE_BK_MAX_EDGES + 1];
    const int K = A.K, tid = threadIdx.x;
    const long long t2 = blockIdx.x % A.tiles2, t1 = blockIdx.x / A.tiles2;
    const long long j0 = t2 * kPcChunk;
    const int cn = (int)(A.c2 - j0 < kPcChunk ? A.c2 - j0 : kPcChunk);
    for (int i = tid; i < cn; i += kBkThreads) chunk[i] = A.m2[j0 + i];
    for (int i = tid; i < K; i += kBkThreads) edges[i] = A.edges[i];
    for (int i = tid; i <= K; i += kBkThreads) hist[i] = 0u;
    __syncthreads();
    const int top = top_step(K);
    const long long i1 = t1 * kBkThreads + tid;
    if (i1 < A.c1) {
        const int4 a = A.m1[i1];
        const int e0 = edges[0], e1 = edges[K - 1];
        for (int j = 0; j < cn; ++j) {
            const int4 b = chunk[j];
            const int x = a.x + b.x, y = a.y + b.y, z = a.z + b.z;
            const int q = x * x + y * y + z * z;
            if (q < e0 || q >= e1) continue;
            atomicAdd(&hist[upper_bound(edges, K, top, q)], 1u);
        }
    }
    __syncthreads();
    for (int i = tid; i <= K; i += kBkThreads)
        if (hist[i]) atomicAdd(&A.hist[i], (unsigned long long)hist[i]);
}

// One-point histogram over nbins uniform bins with float64 edges (np.linspace): voxel x, widened to float64, falls into
// bin searchsorted(edges, x, "right") - 1, and x == edges[nbins] into the last bin.  The bin is estimated from the uniform
// spacing and then moved against the edges themselves, so the rule is the edges' and not the estimate's.  LDS histograms
// per workgroup, flushed with 64-bit integer atomics; counts[nbins] = finite voxels outside, counts[nbins + 1] = non-finite.
// A density field puts half of its voxels into one or two bins, and lanes of one instruction that add to one LDS word
// are served one after the other: the workgroup keeps as many copies of the histogram as fit the space of 4096 bins (16
// at most), lane l adds to copy l mod copies, and the flush sums them (DESIGN.md section 12.2 has the measurements).
struct PdfArgs {
    const float* x;
    long long total;
    double lo, hi, scale;
    int nbins;
    const double* edges;
    unsigned long long* counts;
};

__global__ __launch_bounds__(kBkThreads) void field_histogram_kernel(PdfArgs A) {
    __shared__ double edges[NBE_PDF_MAX_BINS + 1];
    __shared__ unsigned hist[NBE_PDF_MAX_BINS + 2];
    const int nb = A.nbins;
    int copies = 1;
    while (copies < 16 && 2 * copies * (nb + 2) <= NBE_PDF_MAX_BINS + 2) copies *= 2;
    unsigned* mine = hist + (threadIdx.x & (copies - 1)) * (nb + 2);
    for (int i = threadIdx.x; i <= nb; i += kBkThreads) edges[i] = A.edges[i];
    for (int i = threadIdx.x; i < copies * (nb + 2); i += kBkThreads) hist[i] = 0u;
    __syncthreads();
    for (long long i = blockIdx.x * (long long)kBkThreads + threadIdx.x; i < A.total; i += (long long)gridDim.x * kBkThreads) {
        const float xf = A.x[i];
        const double x = (double)xf;
        int b;
        if (!isfinite(xf)) {
            b = nb + 1;
        } else if (x < A.lo || x > A.hi) {
            b = nb;
        } else {
            b = (int)((x - A.lo) * A.scale);
            b = b < 0 ? 0 : b > nb - 1 ? nb - 1 : b;
            while (b > 0 && x < edges[b]) --b;
            while (b < nb - 1 && x >= edges[b + 1]) ++b;
        }
        atomicAdd(&mine[b], 1u);
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nb + 2; i += kBkThreads) {
        unsigned v = 0u;                                  // a workgroup sees fewer than 2^32 voxels
        for (int c = 0; c < copies; ++c) v += hist[c * (nb + 2) + i];
        if (v) atomicAdd(&A.counts[i], (unsigned long long)v);
    }
}

// mom[0] = mean, mom[1] = std and for ORDER 4 mom[2], mom[3] = the third and fourth central moments; the partials start at
// mom[ORDER], ORDER - 1 rows of kMomMaxBlocks
template <int ORDER>
void field_moments(const float* x, long long total, double* mom, hipStream_t s) {
    const int nb = mom_blocks(total);
    const dim3 grid(nb), one(1), block(kMomThreads);
    double* partial = mom + ORDER;
    hipLaunchKernelGGL((moments_pass_kernel<false, 2>), grid, block, 0, s, x, total, mom, partial);
    hipLaunchKernelGGL(sum_finish_kernel, one, block, 0, s, partial, 0LL, nb, mom, total, 0);
    hipLaunchKernelGGL((moments_pass_kernel<true, ORDER>), grid, block, 0, s, x, total, mom, partial);
    for (int p = 2; p <= ORDER; ++p)
        hipLaunchKernelGGL(sum_finish_kernel, one, block, 0, s, partial + (p - 2) * kMomMaxBlocks, 0LL, nb, mom + p - 1,
                           total, p == 2);
}

// f(std::integral_constant<int, P>) for the assignment order P = worder (validated by the caller: 1 .. 4)
template <typename F>
void with_worder(int worder, F f) {
    switch (worder) {
        case 1: f(std::integral_constant<int, 1>{}); break;
        case 2: f(std::integral_constant<int, 2>{}); break;
        case 3: f(std::integral_constant<int, 3>{}); break;
        default: f(std::integral_constant<int, 4>{}); break;
    }
}

}  // namespace

extern "C" {

int nbe_paint_mesh(const void* disp, int disp_dtype, const int64_t n[3], const double boxsize[3], const int64_t res[3],
                   int worder, int count_atomics, void* mesh, void* stats, void* stream) {
    if (!disp || !mesh || !stats || !n || !boxsize || !res) return fail("nbe_paint_mesh: NULL argument");
    if (disp_dtype != NBE_F32 && disp_dtype != NBE_F16) return fail("nbe_paint_mesh: dtype %d unsupported", disp_dtype);
    if (worder < 1 || worder > 4) return fail("nbe_paint_mesh: worder %d not in 1..4", worder);
    for (int c = 0; c < 3; ++c) {
        if (n[c] < 1 || res[c] < 1 || res[c] > (1 << 20) || !(boxsize[c] > 0.0) || !std::isfinite(boxsize[c]))
            return fail("nbe_paint_mesh: bad geometry on axis %d (n %lld, res %lld, boxsize %g)", c, (long long)n[c],
                        (long long)res[c], boxsize[c]);
    }
    PaintArgs A;
    A.disp = disp;
    A.n0 = n[0]; A.n1 = n[1]; A.n2 = n[2];
    A.s0 = res[0] / boxsize[0]; A.s1 = res[1] / boxsize[1]; A.s2 = res[2] / boxsize[2];
    A.a0 = (double)res[0] / n[0]; A.a1 = (double)res[1] / n[1]; A.a2 = (double)res[2] / n[2];
    A.r0 = (int)res[0]; A.r1 = (int)res[1]; A.r2 = (int)res[2];
    const long long tl0 = (n[0] + kTile - 1) / kTile;
    A.tiles1 = (int)((n[1] + kTile - 1) / kTile);
    A.tiles2 = (int)((n[2] + kTile - 1) / kTile);
    A.mesh = (unsigned long long*)mesh;
    A.stats = (int*)stats;
    A.count = count_atomics != 0;
    const long long tiles = tl0 * A.tiles1 * A.tiles2;
    if (tiles > INT_MAX) return fail("nbe_paint_mesh: %lld tiles exceed one launch", tiles);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles), block(kPaintThreads);
    const bool half = disp_dtype == NBE_F16;
    with_worder(worder, [&](auto P) {
        if (half) hipLaunchKernelGGL((paint_kernel<decltype(P)::value, true>), grid, block, 0, s, A);
        else hipLaunchKernelGGL((paint_kernel<decltype(P)::value, false>), grid, block, 0, s, A);
    });
    return launched("nbe_paint_mesh");
}

int nbe_mesh_to_delta(const void* mesh, const int64_t res[3], int64_t nparticles, void* delta, void* stream) {
    if (!mesh || !delta || !res) return fail("nbe_mesh_to_delta: NULL argument");
    if (nparticles < 1 || res[0] < 1 || res[1] < 1 || res[2] < 1) return fail("nbe_mesh_to_delta: bad sizes");
    const long long cells = (long long)res[0] * res[1] * res[2];
    const double scale = (double)cells / ((double)nparticles * kUnit);
    hipLaunchKernelGGL(mesh_to_delta_kernel, dim3(grid_for(cells, 256)), dim3(256), 0, (hipStream_t)stream,
                       (const long long*)mesh, (float*)delta, cells, scale);
    return launched("nbe_mesh_to_delta");
}

int nbe_quantity_range(const void* quantity, int dtype, int nchan, int64_t count, void* range, void* stream) {
    if (!quantity || !range) return fail("nbe_quantity_range: NULL argument");
    if (dtype != NBE_F32 && dtype != NBE_F16) return fail("nbe_quantity_range: dtype %d unsupported", dtype);
    if (nchan < 1 || nchan > NBE_PAINT_MAX_CHANNELS)
        return fail("nbe_quantity_range: %d channels unsupported (1 .. %d)", nchan, NBE_PAINT_MAX_CHANNELS);
    if (count < 1) return fail("nbe_quantity_range: bad size");
    const int g = grid_for(count, 256 * 8);
    hipLaunchKernelGGL(quantity_range_kernel, dim3(g < 2048 ? g : 2048), dim3(256), 0, (hipStream_t)stream, quantity,
                       dtype == NBE_F16, nchan, (long long)count, (unsigned*)range);
    return launched("nbe_quantity_range");
}

int nbe_paint_fields(const void* disp, int disp_dtype, const void* quantity, int quantity_dtype, int nchan,
                     const int exponents[], const void* shift, int shift_dtype, int shift_axis, double shift_scale,
                     const int64_t n[3], const double boxsize[3], const int64_t res[3], int worder, void* mesh,
                     void* qmesh, void* stats, void* stream) {
    if (!mesh || !stats || !n || !boxsize || !res) return fail("nbe_paint_fields: NULL argument");
    if (nchan < 0 || nchan > NBE_PAINT_MAX_CHANNELS)
        return fail("nbe_paint_fields: %d channels unsupported (0 .. %d)", nchan, NBE_PAINT_MAX_CHANNELS);
    if (nchan && (!quantity || !qmesh || !exponents)) return fail("nbe_paint_fields: NULL quantity argument");
    if ((disp && disp_dtype != NBE_F32 && disp_dtype != NBE_F16) ||
        (nchan && quantity_dtype != NBE_F32 && quantity_dtype != NBE_F16) ||
        (shift && shift_dtype != NBE_F32 && shift_dtype != NBE_F16))
        return fail("nbe_paint_fields: dtype unsupported (disp %d, quantity %d, shift %d)", disp_dtype, quantity_dtype,
                    shift_dtype);
    if (shift && (shift_axis < 0 || shift_axis > 2 || !std::isfinite(shift_scale)))
        return fail("nbe_paint_fields: bad shift (axis %d, scale %g)", shift_axis, shift_scale);
    if (worder < 1 || worder > 4) return fail("nbe_paint_fields: worder %d not in 1..4", worder);
    for (int c = 0; c < 3; ++c) {
        if (n[c] < 1 || res[c] < 1 || res[c] > (1 << 20) || !(boxsize[c] > 0.0) || !std::isfinite(boxsize[c]))
            return fail("nbe_paint_fields: bad geometry on axis %d (n %lld, res %lld, boxsize %g)", c, (long long)n[c],
                        (long long)res[c], boxsize[c]);
    }
    FieldArgs A;
    A.disp = disp;
    A.qty = quantity;
    A.shift = shift;
    A.disp_half = disp_dtype == NBE_F16;
    A.qty_half = quantity_dtype == NBE_F16;
    A.shift_half = shift_dtype == NBE_F16;
    A.nchan = nchan;
    A.los = shift ? shift_axis : 0;
    A.n0 = n[0]; A.n1 = n[1]; A.n2 = n[2];
    A.s0 = res[0] / boxsize[0]; A.s1 = res[1] / boxsize[1]; A.s2 = res[2] / boxsize[2];
    A.a0 = (double)res[0] / n[0]; A.a1 = (double)res[1] / n[1]; A.a2 = (double)res[2] / n[2];
    A.vs = shift ? shift_scale * (res[A.los] / boxsize[A.los]) : 0.0;
    A.r0 = (int)res[0]; A.r1 = (int)res[1]; A.r2 = (int)res[2];
    for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c) {
        A.qexp[c] = 0;
        if (c < nchan) {
            if (exponents[c] < -200 || exponents[c] > 200)
                return fail("nbe_paint_fields: exponent %d of channel %d out of range", exponents[c], c);
            A.qexp[c] = 24 - exponents[c];
        }
    }
    const long long tl0 = (n[0] + kTile - 1) / kTile;
    A.tiles1 = (int)((n[1] + kTile - 1) / kTile);
    A.tiles2 = (int)((n[2] + kTile - 1) / kTile);
    A.mesh = (unsigned long long*)mesh;
    A.qmesh = (unsigned long long*)qmesh;
    A.stats = (int*)stats;
    const long long tiles = tl0 * A.tiles1 * A.tiles2;
    if (tiles > INT_MAX) return fail("nbe_paint_fields: %lld tiles exceed one launch", tiles);
    hipStream_t s = (hipStream_t)stream;
    const dim3 grid((unsigned)tiles), block(kPaintThreads);
    with_worder(worder, [&](auto P) { hipLaunchKernelGGL(paint_field_kernel<decltype(P)::value>, grid, block, 0, s, A); });
    return launched("nbe_paint_fields");
}

// the position arguments both particle entry points share; false (with the error set) when they are not valid
static bool position_args(const char* who, PositionArgs& P, const void* pos, int pos_dtype, const void* shift,
                          int shift_dtype, int shift_axis, double shift_scale, int64_t count, const double boxsize[3],
                          const int64_t res[3]) {
    if (!pos || !boxsize || !res) return fail("%s: NULL argument", who), false;
    if (pos_dtype != NBE_F32 && pos_dtype != NBE_F64) return fail("%s: position dtype %d unsupported", who, pos_dtype), false;
    if (shift && shift_dtype != NBE_F32 && shift_dtype != NBE_F16)
        return fail("%s: shift dtype %d unsupported", who, shift_dtype), false;
    if (shift && (shift_axis < 0 || shift_axis > 2 || !std::isfinite(shift_scale)))
        return fail("%s: bad shift (axis %d, scale %g)", who, shift_axis, shift_scale), false;
    if (count < 1 || count > INT_MAX) return fail("%s: %lld particles unsupported (1 .. 2^31 - 1)", who, (long long)count), false;
    for (int c = 0; c < 3; ++c) {
        if (res[c] < 1 || res[c] > (1 << 20) || !(boxsize[c] > 0.0) || !std::isfinite(boxsize[c]))
            return fail("%s: bad geometry on axis %d (res %lld, boxsize %g)", who, c, (long long)res[c], boxsize[c]), false;
    }
    P.pos = pos;
    P.shift = shift;
    P.pos_f64 = pos_dtype == NBE_F64;
    P.shift_half = shift_dtype == NBE_F16;
    P.los = shift ? shift_axis : 0;
    P.s0 = res[0] / boxsize[0]; P.s1 = res[1] / boxsize[1]; P.s2 = res[2] / boxsize[2];
    P.vs = shift ? shift_scale * (res[P.los] / boxsize[P.los]) : 0.0;
    P.count = count;
    return true;
}

int nbe_paint_particles(const void* pos, int pos_dtype, const void* order, const void* quantity, int quantity_dtype,
                        int nchan, const int exponents[], const void* shift, int shift_dtype, int shift_axis,
                        double shift_scale, int64_t count, const double boxsize[3], const int64_t res[3], int worder,
                        void* mesh, void* qmesh, void* stats, void* stream) {
    if (!mesh || !stats) return fail("nbe_paint_particles: NULL argument");
    if (nchan < 0 || nchan > NBE_PAINT_MAX_CHANNELS)
        return fail("nbe_paint_particles: %d channels unsupported (0 .. %d)", nchan, NBE_PAINT_MAX_CHANNELS);
    if (nchan && (!quantity || !qmesh || !exponents)) return fail("nbe_paint_particles: NULL quantity argument");
    if (nchan && quantity_dtype != NBE_F32 && quantity_dtype != NBE_F16)
        return fail("nbe_paint_particles: quantity dtype %d unsupported", quantity_dtype);
    if (worder < 1 || worder > 4) return fail("nbe_paint_particles: worder %d not in 1..4", worder);
    ParticleArgs A;
    if (!position_args("nbe_paint_particles", A.pos, pos, pos_dtype, shift, shift_dtype, shift_axis, shift_scale, count,
                       boxsize, res))
        return 1;
    A.order = (const long long*)order;
    A.qty = quantity;
    A.qty_half = quantity_dtype == NBE_F16;
    A.nchan = nchan;
    A.r0 = (int)res[0]; A.r1 = (int)res[1]; A.r2 = (int)res[2];
    for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c) {
        A.qexp[c] = 0;
        if (c < nchan) {
            if (exponents[c] < -200 || exponents[c] > 200)
                return fail("nbe_paint_particles: exponent %d of channel %d out of range", exponents[c], c);
            A.qexp[c] = 24 - exponents[c];
        }
    }
    A.mesh = (unsigned long long*)mesh;
    A.qmesh = (unsigned long long*)qmesh;
    A.stats = (int*)stats;
    const dim3 grid((unsigned)((count + kChunk - 1) / kChunk)), block(kPaintThreads);
    hipStream_t s = (hipStream_t)stream;
    with_worder(worder, [&](auto P) { hipLaunchKernelGGL(paint_particles_kernel<decltype(P)::value>, grid, block, 0, s, A); });
    return launched("nbe_paint_particles");
}

int nbe_particle_keys(const void* pos, int pos_dtype, const void* shift, int shift_dtype, int shift_axis,
                      double shift_scale, int64_t count, const double boxsize[3], const int64_t res[3], int tile_edge,
                      int morton, void* keys, void* stream) {
    if (!keys) return fail("nbe_particle_keys: NULL argument");
    if (tile_edge < 1 || tile_edge > (1 << 20)) return fail("nbe_particle_keys: tile edge %d unsupported", tile_edge);
    PositionArgs P;
    if (!position_args("nbe_particle_keys", P, pos, pos_dtype, shift, shift_dtype, shift_axis, shift_scale, count, boxsize,
                       res))
        return 1;
    const int g = grid_for(count, 256);
    const dim3 grid(g < 4096 ? g : 4096), block(256);
    hipStream_t s = (hipStream_t)stream;
    const int r0 = (int)res[0], r1 = (int)res[1], r2 = (int)res[2];
    if (morton) hipLaunchKernelGGL(particle_keys_kernel<true>, grid, block, 0, s, P, r0, r1, r2, tile_edge, (long long*)keys);
    else hipLaunchKernelGGL(particle_keys_kernel<false>, grid, block, 0, s, P, r0, r1, r2, tile_edge, (long long*)keys);
    return launched("nbe_particle_keys");
}

int nbe_mesh_read(const void* field, int nchan, const int64_t res[3], const void* disp, int disp_dtype, const int64_t n[3],
                  const void* pos, int pos_dtype, const void* order, int64_t count, const double boxsize[3], int worder,
                  double fill, void* out, void* stats, void* stream) {
    if (!field || !out || !stats || !res || !boxsize) return fail("nbe_mesh_read: NULL argument");
    if (nchan < 1 || nchan > NBE_PAINT_MAX_CHANNELS)
        return fail("nbe_mesh_read: %d channels unsupported (1 .. %d)", nchan, NBE_PAINT_MAX_CHANNELS);
    if (worder < 1 || worder > 4) return fail("nbe_mesh_read: worder %d not in 1..4", worder);
    ReadArgs A;
    if (pos) {
        if (disp) return fail("nbe_mesh_read: positions together with a displacement");
        if (!position_args("nbe_mesh_read", A.pos, pos, pos_dtype, nullptr, NBE_F32, 0, 0.0, count, boxsize, res)) return 1;
        A.n0 = A.n1 = A.n2 = 0;
        A.a0 = A.a1 = A.a2 = 0.0;
    } else {
        if (!n || order) return fail("nbe_mesh_read: the lattice form needs n and takes no order");
        if (disp && disp_dtype != NBE_F32 && disp_dtype != NBE_F16) return fail("nbe_mesh_read: dtype %d unsupported", disp_dtype);
        for (int c = 0; c < 3; ++c) {
            if (n[c] < 1 || n[c] > INT_MAX || res[c] < 1 || res[c] > (1 << 20) || !(boxsize[c] > 0.0) || !std::isfinite(boxsize[c]))
                return fail("nbe_mesh_read: bad geometry on axis %d (n %lld, res %lld, boxsize %g)", c, (long long)n[c],
                            (long long)res[c], boxsize[c]);
        }
        if ((double)n[0] * (double)n[1] * (double)n[2] > (double)INT_MAX || count != n[0] * n[1] * n[2])
            return fail("nbe_mesh_read: count %lld is not the lattice %lld x %lld x %lld (up to 2^31 - 1 rows)",
                        (long long)count, (long long)n[0], (long long)n[1], (long long)n[2]);
        A.pos.pos = nullptr; A.pos.shift = nullptr;
        A.pos.pos_f64 = A.pos.shift_half = A.pos.los = 0;
        A.pos.vs = 0.0;
        A.pos.s0 = res[0] / boxsize[0]; A.pos.s1 = res[1] / boxsize[1]; A.pos.s2 = res[2] / boxsize[2];
        A.pos.count = count;
        A.n0 = n[0]; A.n1 = n[1]; A.n2 = n[2];
        A.a0 = (double)res[0] / n[0]; A.a1 = (double)res[1] / n[1]; A.a2 = (double)res[2] / n[2];
    }
    A.disp = pos ? nullptr : disp;
    A.disp_half = disp_dtype == NBE_F16;
    A.order = (const long long*)order;
    A.field = (const float*)field;
    A.out = (float*)out;
    A.nchan = nchan;
    A.r0 = (int)res[0]; A.r1 = (int)res[1]; A.r2 = (int)res[2];
    A.fill = (float)fill;
    A.stats = (int*)stats;
    const dim3 grid(grid_for(count, 256)), block(256);
    hipStream_t s = (hipStream_t)stream;
    with_worder(worder, [&](auto P) { hipLaunchKernelGGL(mesh_read_kernel<decltype(P)::value>, grid, block, 0, s, A); });
    return launched("nbe_mesh_read");
}

int nbe_mesh_to_field(const void* mesh, const void* qmesh, int nchan, const int exponents[], const int64_t res[3],
                      int64_t nparticles, int mode, double fill, void* field, void* stats, void* stream) {
    if (!mesh || !qmesh || !exponents || !res || !field || !stats) return fail("nbe_mesh_to_field: NULL argument");
    if (nchan < 1 || nchan > NBE_PAINT_MAX_CHANNELS)
        return fail("nbe_mesh_to_field: %d channels unsupported (1 .. %d)", nchan, NBE_PAINT_MAX_CHANNELS);
    if (mode != NBE_FIELD_DENSITY && mode != NBE_FIELD_MEAN) return fail("nbe_mesh_to_field: mode %d unknown", mode);
    if (nparticles < 1 || res[0] < 1 || res[1] < 1 || res[2] < 1) return fail("nbe_mesh_to_field: bad sizes");
    if (!std::isfinite(fill)) return fail("nbe_mesh_to_field: fill is not finite");
    ToFieldArgs A;
    A.mesh = (const long long*)mesh;
    A.qmesh = (const long long*)qmesh;
    A.out = (float*)field;
    A.cells = (long long)res[0] * res[1] * res[2];
    A.nchan = nchan;
    A.mode = mode;
    for (int c = 0; c < NBE_PAINT_MAX_CHANNELS; ++c) A.e[c] = c < nchan ? exponents[c] : 0;
    A.ratio = (double)A.cells / (double)nparticles;
    A.fill = (float)fill;
    A.stats = (int*)stats;
    hipLaunchKernelGGL(mesh_to_field_kernel, dim3(grid_for(A.cells, 256)), dim3(256), 0, (hipStream_t)stream, A);
    return launched("nbe_mesh_to_field");
}

int nbe_deconvolve_mas(void* field, const int64_t res[3], int worder, void* stream) {
    if (!field || !res) return fail("nbe_deconvolve_mas: NULL argument");
    if (worder < 1 || worder > 4) return fail("nbe_deconvolve_mas: worder %d not in 1..4", worder);
    if (res[0] < 1 || res[1] < 1 || res[2] < 1) return fail("nbe_deconvolve_mas: bad sizes");
    const long long n = (long long)res[0] * res[1] * (res[2] / 2 + 1);
    with_worder(worder, [&](auto P) {
        hipLaunchKernelGGL(deconvolve_kernel<decltype(P)::value>, dim3(grid_for(n, 256)), dim3(256), 0,
                           (hipStream_t)stream, (float2*)field, res[0], res[1], res[2]);
    });
    return launched("nbe_deconvolve_mas");
}

int nbe_power_spectrum(const void* a, const void* b, int64_t n, void* binmax, void* sums, void* stream) {
    if (!a || !binmax || !sums) return fail("nbe_power_spectrum: NULL argument");
    if (n < 2 || n > 4096) return fail("nbe_power_spectrum: mesh size %lld unsupported (2 .. 4096)", (long long)n);
    const long long total = n * n * (n / 2 + 1);
    const int nb = (int)(n / 2) + 1;
    const dim3 g(grid_for(total, 256) < 2048 ? grid_for(total, 256) : 2048), blk(256);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pk_max_kernel, g, blk, nb * sizeof(unsigned), s, (const float2*)a, (const float2*)b, (long long)n,
                       (unsigned*)binmax);
    if (int rc = launched("nbe_power_spectrum (max)")) return rc;
    hipLaunchKernelGGL(pk_sum_kernel, g, blk, nb * (3 * sizeof(unsigned long long) + sizeof(int)), s, (const float2*)a,
                       (const float2*)b, (long long)n, (const unsigned*)binmax, (unsigned long long*)sums);
    return launched("nbe_power_spectrum (sum)");
}

int nbe_power_multipoles(const void* a, const void* b, int64_t n, int los, void* binmax, void* sums, void* stream) {
    if (!a || !binmax || !sums) return fail("nbe_power_multipoles: NULL argument");
    if (n < 2 || n > NBE_PK_ANISO_MAX_N)
        return fail("nbe_power_multipoles: mesh size %lld unsupported (2 .. %d)", (long long)n, NBE_PK_ANISO_MAX_N);
    if (los < 0 || los > 2) return fail("nbe_power_multipoles: los %d is not an array axis (0 .. 2)", los);
    const long long total = n * n * (n / 2 + 1);
    const int nb = (int)(n / 2) + 1;
    const dim3 g(grid_for(total, 256) < 2048 ? grid_for(total, 256) : 2048), blk(256);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pk_max_kernel, g, blk, nb * sizeof(unsigned), s, (const float2*)a, (const float2*)b, (long long)n,
                       (unsigned*)binmax);
    if (int rc = launched("nbe_power_multipoles (max)")) return rc;
    hipLaunchKernelGGL(pk_multipole_kernel, g, blk, nb * (5 * sizeof(unsigned long long) + sizeof(int)), s,
                       (const float2*)a, (const float2*)b, (long long)n, los, (const unsigned*)binmax,
                       (unsigned long long*)sums);
    return launched("nbe_power_multipoles (sum)");
}

int nbe_power_wedges(const void* a, const void* b, int64_t n, int los, int nmu, int max_bins, void* binmax, void* sums,
                     void* stream) {
    if (!a || !binmax || !sums) return fail("nbe_power_wedges: NULL argument");
    if (n < 2 || n > NBE_PK_ANISO_MAX_N)
        return fail("nbe_power_wedges: mesh size %lld unsupported (2 .. %d)", (long long)n, NBE_PK_ANISO_MAX_N);
    if (los < 0 || los > 2) return fail("nbe_power_wedges: los %d is not an array axis (0 .. 2)", los);
    if (nmu < 1 || nmu > NBE_PK_MAX_MU) return fail("nbe_power_wedges: %d mu bins unsupported (1 .. %d)", nmu, NBE_PK_MAX_MU);
    const long long total = n * n * (n / 2 + 1);
    const int nb = (int)(n / 2) + 1;
    // the (mu, s) bins of one launch: 4 words each and the shells' exponents in a 64 KiB image
    constexpr int kImageBytes = 65536, kBinBytes = 4 * (int)sizeof(unsigned long long);
    const int fit = (kImageBytes - nb * (int)sizeof(int)) / kBinBytes;
    const int cap = max_bins > 0 && max_bins < fit ? max_bins : fit;
    if (max_bins < 0 || cap < nb)
        return fail("nbe_power_wedges: max_bins %d holds no mu bin of %d shells", max_bins, nb);
    const int per = cap / nb;
    const dim3 g(grid_for(total, 256) < 2048 ? grid_for(total, 256) : 2048), blk(256);
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(pk_max_kernel, g, blk, nb * sizeof(unsigned), s, (const float2*)a, (const float2*)b, (long long)n,
                       (unsigned*)binmax);
    if (int rc = launched("nbe_power_wedges (max)")) return rc;
    for (int mu0 = 0; mu0 < nmu; mu0 += per) {
        const int mu1 = mu0 + per < nmu ? mu0 + per : nmu;
        hipLaunchKernelGGL(pk_wedge_kernel, g, blk, (size_t)(mu1 - mu0) * nb * kBinBytes + nb * sizeof(int), s,
                           (const float2*)a, (const float2*)b, (long long)n, los, nmu, mu0, mu1, (const unsigned*)binmax,
                           (unsigned long long*)sums);
        if (int rc = launched("nbe_power_wedges (sum)")) return rc;
    }
    return 0;
}

int nbe_field_moments(const void* field, int64_t n, void* moments, void* stream) {
    if (!field || !moments) return fail("nbe_field_moments: NULL argument");
    if (n < 1 || n > NBE_MF_MAX_N) return fail("nbe_field_moments: mesh size %lld unsupported (1 .. %d)", (long long)n,
                                               NBE_MF_MAX_N);
    const long long total = (long long)n * n * n;
    field_moments<2>((const float*)field, total, (double*)moments, (hipStream_t)stream);
    return launched("nbe_field_moments");
}

int nbe_minkowski_counts(const void* field, int64_t n, const void* thresholds, int nthresholds, const void* moments,
                         void* counts, void* stream) {
    if (!field || !thresholds || !counts) return fail("nbe_minkowski_counts: NULL argument");
    if (n < 1 || n > NBE_MF_MAX_N) return fail("nbe_minkowski_counts: mesh size %lld unsupported (1 .. %d)",
                                               (long long)n, NBE_MF_MAX_N);
    if (nthresholds < 1 || nthresholds > NBE_MF_MAX_THRESHOLDS)
        return fail("nbe_minkowski_counts: %d thresholds unsupported (1 .. %d)", nthresholds, NBE_MF_MAX_THRESHOLDS);
    MfArgs A;
    A.x = (const float*)field;
    A.n = n;
    A.thr = (const float*)thresholds;
    A.T = nthresholds;
    A.mom = (const double*)moments;
    A.counts = (unsigned long long*)counts;
    A.nj = (int)((n + kMfJ - 1) / kMfJ);
    A.nk = (int)((n + kMfK - 1) / kMfK);
    A.ni = (int)((n + kMfI - 1) / kMfI);
    A.items = (long long)A.nj * A.nk * A.ni;
    // a few resident workgroups per CU loop over the columns: the 64-bit flush is one add per bin per workgroup
    int dev = 0, cus = 256;
    if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) !=
                                                 hipSuccess || cus < 1)
        cus = 256;
    const long long grid = A.items < 4LL * cus ? A.items : 4LL * cus;
    hipLaunchKernelGGL(minkowski_counts_kernel, dim3((unsigned)grid), dim3(kMfThreads), 0, (hipStream_t)stream, A);
    return launched("nbe_minkowski_counts");
}

int nbe_shell_filter(const void* spectrum, int64_t n, const void* shells, int nshells, void* filtered, void* binmax,
                     void* sums, void* stream) {
    if (!spectrum || !shells) return fail("nbe_shell_filter: NULL argument");
    if (n < NBE_BK_MIN_N || n > NBE_BK_MAX_N)
        return fail("nbe_shell_filter: mesh size %lld unsupported (%d .. %d)", (long long)n, NBE_BK_MIN_N, NBE_BK_MAX_N);
    if (nshells < 1 || nshells > NBE_BK_MAX_SHELLS)
        return fail("nbe_shell_filter: %d shells unsupported (1 .. %d)", nshells, NBE_BK_MAX_SHELLS);
    if (!filtered && !sums) return fail("nbe_shell_filter: nothing to do (filtered and sums are both NULL)");
    if ((binmax == nullptr) != (sums == nullptr)) return fail("nbe_shell_filter: binmax and sums go together");
    ShellArgs A;
    A.spec = (const float2*)spectrum;
    A.n = n;
    A.par = (const long long*)shells;
    A.S = nshells;
    A.out = (float2*)filtered;
    A.binmax = (unsigned*)binmax;
    A.sums = (unsigned long long*)sums;
    const long long total = n * n * (n / 2 + 1);
    const int grid = grid_for(total, 4 * kBkThreads);
    hipStream_t s = (hipStream_t)stream;
    if (sums) {
        hipLaunchKernelGGL(shell_max_kernel, dim3(grid < 2048 ? grid : 2048), dim3(kBkThreads), 0, s, A);
        if (int rc = launched("nbe_shell_filter (max)")) return rc;
    }
    hipLaunchKernelGGL(shell_filter_kernel, dim3(grid < 4096 ? grid : 4096), dim3(kBkThreads), 0, s, A);
    return launched("nbe_shell_filter");
}

int nbe_triple_sums(const void* f1, const void* f2, const void* f3, int nfields, int64_t n, void* partials, void* out,
                    void* stream) {
    if (!f1 || !f2 || !f3 || !partials || !out) return fail("nbe_triple_sums: NULL argument");
    if (n < 1 || n > NBE_BK_MAX_N) return fail("nbe_triple_sums: mesh size %lld unsupported (1 .. %d)", (long long)n,
                                               NBE_BK_MAX_N);
    if (nfields < 1 || nfields > NBE_BK_MAX_SHELLS)
        return fail("nbe_triple_sums: %d fields unsupported (1 .. %d)", nfields, NBE_BK_MAX_SHELLS);
    const long long total = (long long)n * n * n;
    const int nb = mom_blocks(total);
    hipStream_t s = (hipStream_t)stream;
    for (int j0 = 0; j0 < nfields; j0 += kTsFields) {
        TripleArgs A;
        A.f1 = (const float*)f1;
        A.f2 = (const float*)f2;
        A.nj = nfields - j0 < kTsFields ? nfields - j0 : kTsFields;
        for (int j = 0; j < kTsFields; ++j) A.f3[j] = (const float*)f3 + (long long)(j0 + (j < A.nj ? j : 0)) * total;
        A.total = total;
        A.partial = (double*)partials + (long long)j0 * NBE_BK_PARTIALS;
        hipLaunchKernelGGL(triple_sums_kernel, dim3(nb), dim3(kMomThreads), 0, s, A);
        if (int rc = launched("nbe_triple_sums")) return rc;
    }
    hipLaunchKernelGGL(sum_finish_kernel, dim3(nfields), dim3(kMomThreads), 0, s, (const double*)partials,
                       (long long)NBE_BK_PARTIALS, nb, (double*)out, 0LL, 0);
    return launched("nbe_triple_sums (finish)");
}

int nbe_triangle_counts(const void* modes1, int64_t count1, const void* modes2, int64_t count2, const void* edges,
                        int nedges, void* hist, void* stream) {
    if (!modes1 || !modes2 || !edges || !hist) return fail("nbe_triangle_counts: NULL argument");
    if (count1 < 1 || count2 < 1) return fail("nbe_triangle_counts: empty mode list");
    if (nedges < 2 || nedges > NBE_BK_MAX_EDGES)
        return fail("nbe_triangle_counts: %d bounds unsupported (2 .. %d)", nedges, NBE_BK_MAX_EDGES);
    PairArgs A;
    A.m1 = (const int4*)modes1; A.c1 = count1;
    A.m2 = (const int4*)modes2; A.c2 = count2;
    A.edges = (const int*)edges; A.K = nedges;
    A.hist = (unsigned long long*)hist;
    A.tiles2 = (count2 + kPcChunk - 1) / kPcChunk;
    const long long blocks = ((count1 + kBkThreads - 1) / kBkThreads) * A.tiles2;
    if (blocks > INT_MAX) return fail("nbe_triangle_counts: %lld x %lld pairs exceed one launch", (long long)count1,
                                      (long long)count2);
    hipLaunchKernelGGL(pair_count_kernel, dim3((unsigned)blocks), dim3(kBkThreads), 0, (hipStream_t)stream, A);
    return launched("nbe_triangle_counts");
}

int nbe_field_moments4(const void* field, int64_t count, void* moments, void* stream) {
    if (!field || !moments) return fail("nbe_field_moments4: NULL argument");
    if (count < 1 || count > NBE_ONEPOINT_MAX_VOXELS)
        return fail("nbe_field_moments4: %lld voxels unsupported (1 .. 2^40)", (long long)count);
    field_moments<4>((const float*)field, count, (double*)moments, (hipStream_t)stream);
    return launched("nbe_field_moments4");
}

int nbe_field_histogram(const void* field, int64_t count, double lo, double hi, const void* edges, int nbins,
                        void* counts, void* stream) {
    if (!field || !edges || !counts) return fail("nbe_field_histogram: NULL argument");
    if (count < 1 || count > NBE_ONEPOINT_MAX_VOXELS)
        return fail("nbe_field_histogram: %lld voxels unsupported (1 .. 2^40)", (long long)count);
    if (nbins < 2 || nbins > NBE_PDF_MAX_BINS)
        return fail("nbe_field_histogram: %d bins unsupported (2 .. %d)", nbins, NBE_PDF_MAX_BINS);
    if (!(hi > lo) || !std::isfinite(lo) || !std::isfinite(hi))
        return fail("nbe_field_histogram: edges %g .. %g are not an interval", lo, hi);
    hipStream_t s = (hipStream_t)stream;
    PdfArgs A;
    A.x = (const float*)field;
    A.total = count;
    A.lo = lo; A.hi = hi;
    A.scale = (double)nbins / (hi - lo);
    A.nbins = nbins;
    A.edges = (const double*)edges;
    A.counts = (unsigned long long*)counts;
    // a workgroup's 32-bit LDS bins hold at most count / grid voxels: at least count / 2^31 workgroups
    long long grid = (count + 8LL * kBkThreads - 1) / (8LL * kBkThreads);
    grid = grid > 2048 ? 2048 : grid;
    hipLaunchKernelGGL(field_histogram_kernel, dim3((unsigned)grid), dim3(kBkThreads), 0, s, A);
    return launched("nbe_field_histogram");
}

}  // extern "C"
