// Shared between nbe_kernels.hip (float32 path, data movement) and nbe_kernels_h3.hip (f16x3 path).
#pragma once
#include "nbe_conv_select.h"
#include <mutex>
#include <set>
#include <utility>

namespace nbe {

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half4 __attribute__((ext_vector_type(4)));

#define NBE_LDS_AS __attribute__((address_space(3)))
#define NBE_GLB_AS __attribute__((address_space(1)))

// Where a launcher's source tables point.  Chunk c of the input (16 channels = 4 planes; chunks >= csplit come from the
// second tensor) and chunk sc of a fused skip's input (likewise, from s_csplit on): first plane of the chunk, primal and
// tangent, and the plane stride in bytes.
struct ChunkSrc { const char* x; const char* dx; long psb; };
inline ChunkSrc input_chunk(const ConvKArgs& ka, int c) {
    const bool second = c >= ka.csplit;
    const long ps = second ? ka.in2_pstride : ka.in_pstride;
    const long off = (long)(second ? c - ka.csplit : c) * 4 * ps * 16;
    return {(const char*)(second ? ka.x2 : ka.x) + off, (const char*)(second ? ka.dx2 : ka.dx) + off, ps * 16};
}
inline ChunkSrc skip_chunk(const ConvKArgs& ka, int sc) {
    const bool second = sc >= ka.s_csplit;
    const long ps = second ? ka.s2_pstride : ka.s_pstride;
    const long off = (long)(second ? sc - ka.s_csplit : sc) * 4 * ps * 16;
    return {(const char*)(second ? ka.xs2 : ka.xs) + off, (const char*)(second ? ka.dxs2 : ka.dxs) + off, ps * 16};
}

__device__ __forceinline__ void dma16(const float* src, f32x4* dst_wave_base) {
    // 64 lanes x 16 B: LDS destination = wave-uniform base + lane*16 (hardware rule), source per lane.
    __builtin_amdgcn_global_load_lds((const NBE_GLB_AS void*)src, (NBE_LDS_AS void*)dst_wave_base, 16, 0, 0);
}

// Allow a kernel more than the default 64 KB of dynamic LDS: set once per (kernel, current device), from any thread.  The
// result is not checked: a launch beyond the limit fails and surfaces through the callers' error checks.
inline void ensure_lds_limit(const void* kernel, size_t bytes) {
    static std::mutex mu;
    static std::set<std::pair<const void*, int>> done;
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> lock(mu);
    if (done.insert({kernel, dev}).second)
        (void)hipFuncSetAttribute(kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
}

// XCD-aware tile order: blocks b and b+8 share an XCD (and its L2); give each XCD a contiguous run
// of tiles so that neighbouring tiles (which share input rows) hit the same L2.  Bijective form.
__device__ __forceinline__ int xcd_tile(int b, int nt) {
    const int qd = nt >> 3, rm = nt & 7, xcd = b & 7;
    return (xcd < rm ? xcd * (qd + 1) : rm * (qd + 1) + (xcd - rm) * qd) + (b >> 3);
}

// f16x3 path (nbe_kernels_h3.hip)
int launch_conv_h3(ConvKernel k, const PackedW& pw, const ConvKArgs& ka, bool vel, bool has_dx, hipStream_t s);
void launch_pack_h3(const float* w_oidhw, int cout, int cin, int kind, const PackedW& pw, float* dst, hipStream_t s);
void launch_gather_h8(const float* box, int C, int Db, int Hb, int Wb, int a0, int a1, int a2,
                      float* dst, const Planes& geom, float scale, int parts, hipStream_t s);
void launch_from_planes_h8(const float* src, const Planes& geom, int C, float* dst, int parts, hipStream_t s);
void launch_head_h8(const Planes& y, const Planes& xin, int c0, int C, const HeadScale& hs, bool vel,
                    void* disp, void* velo, int out_dtype, int Db, int Hb, int Wb, int a0, int a1, int a2,
                    int parts, hipStream_t s, int pad = 0);

}  // namespace nbe
