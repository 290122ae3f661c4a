// The per-voxel bodies of the cosmic-web classification (nbe_web.hip): the eigenvalues of a
// symmetric 3x3 tensor and the type of a voxel from them.  Both are inline and __host__ __device__: the kernels are loops
// around them, and tools/web_host_walk.hip walks the same bodies serially on the host.
//
// Eigenvalues.  The six float32 words (0,0), (1,1), (2,2), (0,1), (0,2), (1,2) are widened to float64 and the result is
// rounded to float32 once.  Where the three off-diagonal words are exactly 0 the result is the sorted diagonal itself, bit
// for bit.  Otherwise the trigonometric closed form (Smith 1961; Kopp 2008): q = tr A / 3, p = sqrt(tr((A - q I)^2) / 6),
// B = (A - q I) / p, phi = acos(clamp(det B / 2, -1, 1)) / 3, lambda_1 = q + 2 p cos(phi), lambda_3 = q + 2 p cos(phi +
// 2 pi / 3), lambda_2 = 3 q - lambda_1 - lambda_3.  Its float64 error against LAPACK's symmetric solver stays below
// 8.3e-9 |A|_F = 0.14 * 2^-24 |A|_F over random, nearly diagonal, rank-one, doubly degenerate, isotropic and wide-range
// input (the acos loses half the digits next to a degenerate pair, which is where that figure comes from), far below the one
// float32 rounding of 2^-24 |A|_F that follows.  On degenerate input lambda_2 can land a rounding outside
// [lambda_3, lambda_1], so the three float64 values are sorted before they are rounded; rounding is monotonic, so the
// float32 words are ordered too.  A non-finite word gives three NaNs.
//
// Type.  m = the number of eigenvalues > threshold in float32 comparison: 0 void, 1 sheet, 2 filament, 3 knot (Hahn et al.
// 2007 with threshold 0; Forero-Romero et al. 2009 with a free threshold; Hoffman et al. 2012 for the velocity shear).  A
// voxel with a NaN eigenvalue has no type: kWebNaN.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>

namespace nbe {

constexpr int kWebTypes = 4;                               // void, sheet, filament, knot
constexpr int kWebNaN = 4;                                 // the slot of counts[t][.] for voxels without a type
constexpr unsigned char kWebNaNType = 255;                 // what such a voxel gets in `types`

__host__ __device__ inline void web_sort3(double& a, double& b, double& c) {      // a >= b >= c
    double t;
    if (a < b) { t = a; a = b; b = t; }
    if (b < c) { t = b; b = c; c = t; }
    if (a < b) { t = a; a = b; b = t; }
}

// e[0] >= e[1] >= e[2] of the tensor (h0 h3 h4; h3 h1 h5; h4 h5 h2)
__host__ __device__ inline void web_eigenvalues(float h0, float h1, float h2, float h3, float h4, float h5, float* e) {
    const double a = h0, b = h1, c = h2, d = h3, f = h4, g = h5;
    const double nan = __builtin_nan("");
    // a sum of finite float32 magnitudes is finite in float64, and non-finite as soon as one word is
    if (!(fabs(a) + fabs(b) + fabs(c) + fabs(d) + fabs(f) + fabs(g) < __builtin_inf())) {
        e[0] = e[1] = e[2] = (float)nan;
        return;
    }
    double l1 = a, l2 = b, l3 = c;
    if (d != 0.0 || f != 0.0 || g != 0.0) {
        const double q = (a + b + c) / 3.0;
        const double x = a - q, y = b - q, z = c - q;
        const double p2 = ((x * x + y * y) + z * z) + 2.0 * ((d * d + f * f) + g * g);
        const double p = sqrt(p2 / 6.0);
        if (p > 0.0) {
            const double ip = 1.0 / p;
            const double bx = x * ip, by = y * ip, bz = z * ip, bd = d * ip, bf = f * ip, bg = g * ip;
            const double det = bx * (by * bz - bg * bg) - bd * (bd * bz - bg * bf) + bf * (bd * bg - by * bf);
            double r = 0.5 * det;
            r = r < -1.0 ? -1.0 : r > 1.0 ? 1.0 : r;
            const double phi = acos(r) / 3.0;
            l1 = q + 2.0 * p * cos(phi);
            l3 = q + 2.0 * p * cos(phi + 2.0943951023931953);      // 2 pi / 3
            l2 = 3.0 * q - l1 - l3;
        }
    }
    web_sort3(l1, l2, l3);
    e[0] = (float)l1; e[1] = (float)l2; e[2] = (float)l3;
}

// the type of a voxel with the eigenvalues (e0, e1, e2), in any order: 0 .. 3, or kWebNaN
__host__ __device__ inline int web_type(float e0, float e1, float e2, float threshold) {
    if (e0 != e0 || e1 != e1 || e2 != e2) return kWebNaN;
    return (int)(e0 > threshold) + (int)(e1 > threshold) + (int)(e2 > threshold);
}

}  // namespace nbe
