// Which kernel runs a convolution launch: one pure host function of (PackedW, ConvKArgs, velocity, input tangent), the
// limits it tests, and the profile label of the result.  No device code: launch_conv / launch_conv_h3 switch over
// conv_select(), every launcher checks its own predicate below once, the engine's planners (block_fused, up8_launch,
// two_source_width, the packers) use the same constants and predicates, and tools/conv_select_walk.hip walks it on a CPU.
#pragma once
#include "nbe_kernels.h"
#include <algorithm>
#include <cstdio>
#include <string>

namespace nbe {

// ---- the geometry the conditions test (the kernels' own constants; their derived sizes stay beside the kernels) ----------
constexpr int H3_CHUNK = 16;                       // channels of one K chunk of the f16-based kernels
constexpr int HP_ROWS = 8, HP_COLS = 32;           // the 2-D patch of conv_h3p / h3q / h3g / h3nz / h3w: rows x columns of one plane
constexpr int H2_ROWS = 16;                        // conv_h2q_kernel: 16 rows x HP_COLS columns
#ifndef NBE_STEM_ROWS
#define NBE_STEM_ROWS 1
#endif
constexpr int ST_ROWS = NBE_STEM_ROWS, ST_COLS = 128 / ST_ROWS;   // stem_h3_kernel's tile
constexpr int UP_MAXCH = 4;                        // up_h3_kernel: Cin <= 64
constexpr int HNZ_MAXCH = 4;                       // conv_h3nz_kernel: at most 64 input channels, and 64 of the block input
constexpr int HNZ_R = 4;                           // conv_h3nz_kernel: weight rows kept per 16-row unit = its couts
constexpr int NBE_MAX_WSTAGES = 32;                // conv_h3w_kernel: 4 * Cin / 16 transformed stages: Cin <= 128
constexpr int NBE_MAX_WSKIP = 16;                  // its fused skip: 2 planes x Cin_block / 16 source entries behind the transformed stages'
constexpr int H3W_F16_CHUNKS = 2;                  // its float16 form: a stage covers two 16-channel chunks (32 channels)

// one value per kernel instantiation family
enum ConvKernel : int {
    CONV_NONE = 0,          // the layer / flag combination has no kernel (an engine bug: launch_conv returns 1)
    CONV_STEM,              // stem_h3_kernel
    CONV_UP8,               // up_h3_kernel
    CONV_H3_FLAT1,          // conv_h3_kernel<MODE_FLAT1>
    CONV_H3_DOWN,           // conv_h3_kernel<MODE_DOWN>
    CONV_H3P,               // conv_h3p_kernel
    CONV_H3Q,               // conv_h3q_kernel
    CONV_H2Q_SPLIT,         // conv_h2q_kernel<true>: f16x3, displacement only
    CONV_H2Q_F16,           // conv_h2q_kernel<false>: float16, velocity
    CONV_H2Q_F16_G,         // conv_h2q_kernel<false, true>: float16, gauged input tangent
    CONV_H3G_WIDE,          // conv_h3g_kernel<false>
    CONV_H3G_NARROW,        // conv_h3g_kernel<true>
    CONV_H3NZ,              // conv_h3nz_kernel
    CONV_H3W_F16X3,         // conv_h3w_kernel<SKIP, false>
    CONV_H3W_NOVEL,         // conv_h3w_kernel<SKIP, true>
    CONV_H3W_F16,           // conv_h3w_kernel<SKIP, false, true>
    CONV_MFMA,              // conv_mfma_kernel (strict float32)
    CONV_MFMA_G,            // conv_mfma_kernel<..., G6>
};
inline const char* conv_kernel_name(ConvKernel k) {
    static const char* const n[] = {"none", "stem", "up8", "h3_flat1", "h3_down", "h3p", "h3q", "h2q_split", "h2q_f16", "h2q_f16_g",
                                    "h3g_wide", "h3g_narrow", "h3nz", "h3w_f16x3", "h3w_novel", "h3w_f16", "mfma", "mfma_g"};
    return n[k];
}
inline bool conv_is_wino(ConvKernel k) { return k == CONV_H3W_F16X3 || k == CONV_H3W_NOVEL || k == CONV_H3W_F16; }
inline bool conv_is_narrow(ConvKernel k) { return k == CONV_H3G_NARROW || k == CONV_H3NZ; }

// ---- limits the engine plans with before a launch exists ------------------------------------------------------------------
inline constexpr bool up8_fits(int cin_pad) { return cin_pad / H3_CHUNK <= UP_MAXCH; }          // up_h3_kernel keeps the whole input in LDS
inline constexpr bool h3w_pairs_planes(int nplanes) { return (nplanes & 1) == 0; }               // conv_h3w_kernel computes output planes in pairs
// transformed stages / fused-skip entries of conv_h3w_kernel for `cin_pad` channels (chunks: 1 = f16x3, H3W_F16_CHUNKS = float16)
inline constexpr bool h3w_stages_fit(int cin_pad, int chunks = 1) { return 4 * (cin_pad / (H3_CHUNK * chunks)) <= NBE_MAX_WSTAGES; }
inline constexpr bool h3w_skip_fits(int cin_pad, int chunks = 1) { return 2 * (cin_pad / (H3_CHUNK * chunks)) <= NBE_MAX_WSKIP; }
// channels between which a kernel with two input tensors may switch sources (whole K chunks; whole stages in the float16 form)
inline constexpr int two_source_chunk(int prec) { return prec == PREC_F16 ? H3_CHUNK * H3W_F16_CHUNKS : H3_CHUNK; }

// ---- patch tiles -------------------------------------------------------------------------------------------------------------
// tiles of `rows` x `cols` outputs over the (Hv, Wv) planes of a launch: sets ka.tny / ka.tnx, returns the tiles of `nz` plane groups
inline constexpr int tiles_of(int n, int tile) { return (n + tile - 1) / tile; }
inline long patch_tiles(ConvKArgs& ka, int rows, int cols, int nz) {
    ka.tny = tiles_of(ka.Hv, rows);
    ka.tnx = tiles_of(ka.Wv, cols);
    return (long)nz * ka.tny * ka.tnx;
}

// ---- what each launcher needs (conv_select decides with these; the launcher checks its own once) -----------------------------
inline bool cout_tiles_ok(const ConvKArgs& ka, int ctiles, int cout_t) {        // cout tiling mismatch: reported by the caller
    return ctiles == (ka.cout_groups + cout_t / 8 - 1) / (cout_t / 8);
}
inline bool stem_ok(const ConvKArgs& ka) {
    const long nt = (long)ka.Dv * tiles_of(ka.Hv, ST_ROWS) * tiles_of(ka.Wv, ST_COLS);
    return nt > 0 && nt < (1L << 31) && ka.cout_groups <= 8 && ka.nchunk == 1;
}
inline bool up8_ok(const ConvKArgs& ka) { return ka.nchunk <= UP_MAXCH; }
inline bool h3q_ok(const ConvKArgs& ka, int ctiles) { return cout_tiles_ok(ka, ctiles, 64); }
inline bool h2q_ok(const ConvKArgs& ka, int ctiles) { return cout_tiles_ok(ka, ctiles, 64); }
// the kernel reads its per-group sources from a table in its arguments (the engine does not wire a larger network for it)
inline bool h3g_ok(const ConvKArgs& ka, int ctiles, bool narrow) {
    return cout_tiles_ok(ka, ctiles, narrow ? 16 : 64) && 3 * ka.nchunk + ka.nskip <= NBE_MAX_GROUPS;
}
// conv_h3nz_kernel: not more than 4 couts or 64 channels, not the residual form, not a skip whose input has no tangent
inline bool h3nz_ok(const ConvKArgs& ka, int ctiles, int cout) {
    return ctiles == 1 && cout <= HNZ_R && ka.cout_groups == 1 && !(ka.flags & (F_RES | F_SKIP_NODX)) && ka.beta && ka.Dv >= 1 &&
           ka.nchunk <= HNZ_MAXCH && ka.nskip <= HNZ_MAXCH && ka.nchunk + ka.nskip <= NBE_MAX_GROUPS;
}
// conv_h3w_kernel.  novel: the displacement-only form (no tangent tensors, two row blocks per workgroup); f16: the float16
// model's form (32-channel stages, residual in the epilogue)
inline bool h3w_ok(const ConvKArgs& ka, int ctiles, bool novel, bool f16) {
    int nchunk = ka.nchunk, csplit = ka.csplit, nskip = ka.nskip;
    if (f16) {                                                   // 16-channel chunks -> 32-channel stages: whole stages per source
        if (novel || (nchunk & 1) || (csplit < nchunk && (csplit & 1))) return false;
        if (nskip > 0 && ((nskip & 1) || (ka.s_csplit < nskip && (ka.s_csplit & 1)) || (ka.flags & F_SKIP_NODX))) return false;
        nchunk /= H3W_F16_CHUNKS; nskip /= H3W_F16_CHUNKS; if (csplit < (1 << 29)) csplit /= H3W_F16_CHUNKS;
    }
    // the f16x3 forms have no residual; planes are computed in pairs; the gauged forms need the gauge
    if (!ka.ww || (!f16 && (ka.flags & F_RES)) || !h3w_pairs_planes(ka.Dv) || 4 * nchunk > NBE_MAX_WSTAGES || (!novel && !ka.beta)) return false;
    if (nskip > 0 && (!ka.wws || 2 * nskip > NBE_MAX_WSKIP)) return false;
    if (!cout_tiles_ok(ka, ctiles, 64)) return false;
    // the raw planes are fetched with buffer loads (32-bit offsets): lane offset + hi -> lo plane distance stay below 2^32
    return std::max(ka.in_pstride, csplit < nchunk ? ka.in2_pstride : 0L) * 16 + 16L * (HP_ROWS + 2) * ka.W < (1L << 32) - (1L << 20);
}

// ---- the decision ----------------------------------------------------------------------------------------------------------
// ka as launch_conv prepares it: ka.ww / ka.wws are NULL unless the engine allows the Winograd-z kernel for this launch.
inline ConvKernel conv_select(const PackedW& pw, const ConvKArgs& ka, bool vel, bool has_dx) {
    const int ct = pw.ctiles;
    const bool flat3 = pw.mode == MODE_FLAT3;
    const bool plain = ka.in_off == 0 && ka.osz == 1;           // 3x3x3 layers are never cropped or strided
    if (!prec_is_half(pw.prec)) {                                // strict float32: one kernel, every mode
        if (!ka.beta) return CONV_MFMA;
        return (flat3 && vel && has_dx) ? CONV_MFMA_G : CONV_NONE;   // gauged input tangent: 3x3x3 layers only
    }
    const bool split = pw.prec == PREC_F16X3;
    // the first layer in its own packing: no input tangent, nothing fused
    if (ka.stem_w && !(vel && has_dx) && flat3 && plain && !(ka.flags & F_RES) && ka.nskip == 0 && !ka.beta)
        return stem_ok(ka) ? CONV_STEM : CONV_NONE;
    // a second input segment / a fused skip exist only in the gauged f16x3 kernels and in conv_h3w_kernel's displacement-only
    // and float16 forms
    if ((ka.nskip > 0 || ka.csplit < ka.nchunk) && !(ka.beta && split)) {
        if (split && !vel && flat3 && plain) return h3w_ok(ka, ct, true, false) ? CONV_H3W_NOVEL : CONV_NONE;
        if (!split && vel && has_dx && ka.beta && flat3 && plain) return h3w_ok(ka, ct, false, true) ? CONV_H3W_F16 : CONV_NONE;
        return CONV_NONE;
    }
    if (ka.beta) {                                               // gauged input tangent: 3x3x3 layers with velocity and an input tangent
        if (!(flat3 && vel && has_dx && plain)) return CONV_NONE;
        if (split) {
            if (pw.cout_t == 16) {                              // the head convolution: one pass along z, dz in the MFMA rows, where the launch allows
                if (h3nz_ok(ka, ct, pw.cout)) return CONV_H3NZ;
                return h3g_ok(ka, ct, true) ? CONV_H3G_NARROW : CONV_NONE;
            }
            if (h3w_ok(ka, ct, false, false)) return CONV_H3W_F16X3;     // Winograd along z
            return h3g_ok(ka, ct, false) ? CONV_H3G_WIDE : CONV_NONE;
        }
        if (h3w_ok(ka, ct, false, true)) return CONV_H3W_F16;            // float16 model: Winograd along z
        return h2q_ok(ka, ct) ? CONV_H2Q_F16_G : CONV_NONE;
    }
    if (flat3) {
        if (!plain) return CONV_NONE;
        if (split && vel && has_dx) return h3q_ok(ka, ct) ? CONV_H3Q : CONV_NONE;
        if (split && !vel && h3w_ok(ka, ct, true, false)) return CONV_H3W_NOVEL;   // Winograd along z, displacement only
        if (split && !vel) return h2q_ok(ka, ct) ? CONV_H2Q_SPLIT : CONV_NONE;
        if (!split && vel && has_dx) return h2q_ok(ka, ct) ? CONV_H2Q_F16 : CONV_NONE;
        // left for the 32x32x16 patch kernel: the first layer without the stem (velocity, no input tangent) and the float16
        // model's displacement-only layers
        return CONV_H3P;
    }
    if (pw.mode == MODE_FLAT1) {
        if (!ka.up8) return CONV_H3_FLAT1;
        // all eight parities in one launch: an input tangent wherever there is velocity
        return ((vel && has_dx) || !vel) && up8_ok(ka) ? CONV_UP8 : CONV_NONE;
    }
    return CONV_H3_DOWN;
}

// The profile label of a launch (nbe_profile_read; bench.py and the tests match on these strings): pw gives the mode, the
// precision and ni.  conv_h3n covers both kernels of the narrow packing.
inline std::string conv_label(ConvKernel k, const PackedW& pw, bool vel, bool has_dx) {
    const char* m = pw.mode == MODE_FLAT3 ? "FLAT3" : pw.mode == MODE_FLAT1 ? "FLAT1" : "DOWN";
    const bool f16 = pw.prec == PREC_F16;
    char b[96];
    switch (k) {
    case CONV_NONE: return "none";
    case CONV_STEM: return vel ? "stem_h3<FLAT3,vel,nodx>" : "stem_h3<FLAT3,novel>";
    case CONV_UP8: return vel ? "up_h3<8 parities,vel,dx>" : "up_h3<8 parities,novel>";
    case CONV_H3W_F16X3: return "conv_h3w<FLAT3,vel,dx>";
    case CONV_H3W_NOVEL: return "conv_h3w<FLAT3,novel>";
    case CONV_H3W_F16: return "conv_h1w<FLAT3,vel,dx>";
    case CONV_H3G_WIDE: case CONV_H3G_NARROW: case CONV_H3NZ: case CONV_H2Q_F16_G:
        snprintf(b, sizeof b, "%s<%s,vel,dx>", k == CONV_H2Q_F16_G ? "conv_h1g" : conv_is_narrow(k) ? "conv_h3n" : "conv_h3g", m);
        return b;
    case CONV_MFMA_G: snprintf(b, sizeof b, "conv_mfma_g<%s,vel,dx,ni%d>", m, pw.ni); return b;
    case CONV_MFMA:
        snprintf(b, sizeof b, "conv_mfma<%s,%s,%s,ni%d>", m, vel ? "vel" : "novel", (vel && has_dx) ? "dx" : "nodx", pw.ni);
        return b;
    default:                                                     // conv_h3 / h3p / h3q / h2q: one label per (mode, velocity, input tangent)
        snprintf(b, sizeof b, "%s<%s,%s,%s>", f16 ? "conv_h1" : "conv_h3", m, vel ? "vel" : "novel", (vel && has_dx) ? "dx" : "nodx");
        return b;
    }
}

}  // namespace nbe
