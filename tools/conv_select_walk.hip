// conv_select() and conv_label() of csrc/nbe_conv_select.h on the host: which kernel a convolution launch gets, and the
// profile label it is given, for launch forms read from stdin.  Host code only; nothing here touches a device, the pointers
// of a case are dummies that are never followed, and plane strides are plain numbers.
//
//     hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -o conv_select_walk tools/conv_select_walk.hip
//     ./conv_select_walk < cases.txt
//
// tests/test_conv_select.py builds the same program without the sanitizers and holds its output to a table read from the
// try-and-fall-back chain this function replaced.
//
// A case is one line: NAME key=value ...; the answer is one line: NAME <tab> kernel <tab> label.  Keys (defaults in brackets):
//   prec f32|f16x3|f16 [f16x3]   mode flat3|flat1|down [flat3]   vel dx [1 1]   cin cout [64 64] (cin: padded to whole chunks)
//   cout_t [64; 16 = the narrow packing]   ni [2]   ctiles [from cout and the tile]
//   beta [0] gauged input tangent   ww [0] Winograd-z packing present and allowed   wws [0] the fused skip's   stem [0]
//   skip [0] channels of a fused skip   csplit, s_csplit [0] channels of the first of two sources (input, skip)
//   res nodx [0 0] F_RES, F_SKIP_NODX   up8 [0]   in_off [0]   osz [1]   Dv Hv Wv [8 30 30]   H W [32 32]
//   pstride pstride2 [H * W * (Dv + 2)] voxels between the planes of the input, of its second source

#include "../jax_nbody_emulator_with_dj_amd/csrc/nbe_conv_select.h"

#include <cstdlib>
#include <cstring>
#include <iostream>
#include <map>
#include <sstream>

using namespace nbe;

int main() {
    static float dummy[4];                                       // never read: conv_select tests pointers against NULL only
    std::string line;
    int rc = 0;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string name, kv;
        if (!(in >> name) || name[0] == '#') continue;
        std::map<std::string, std::string> a;
        while (in >> kv) {
            const size_t e = kv.find('=');
            if (e == std::string::npos) { fprintf(stderr, "%s: bad token %s\n", name.c_str(), kv.c_str()); rc = 2; continue; }
            a[kv.substr(0, e)] = kv.substr(e + 1);
        }
        size_t used = 0;
        auto str = [&](const char* k, const char* d) { auto it = a.find(k); if (it == a.end()) return std::string(d); ++used; return it->second; };
        auto num = [&](const char* k, long d) { auto it = a.find(k); if (it == a.end()) return d; ++used; return atol(it->second.c_str()); };

        const std::string prec = str("prec", "f16x3"), mode = str("mode", "flat3");
        PackedW pw;
        pw.prec = prec == "f32" ? PREC_F32 : prec == "f16" ? PREC_F16 : PREC_F16X3;
        pw.mode = mode == "flat1" ? MODE_FLAT1 : mode == "down" ? MODE_DOWN : MODE_FLAT3;
        const bool half = prec_is_half(pw.prec);
        const int ck = prec_ck(pw.prec, pw.mode);
        pw.cin = (int)num("cin", 64); pw.cout = (int)num("cout", 64);
        pw.cin_pad = (pw.cin + ck - 1) / ck * ck;
        pw.ni = (int)num("ni", 2); pw.cout_t = (int)num("cout_t", 64);
        const int tile = half ? pw.cout_t : 32 * pw.ni;
        pw.ctiles = (int)num("ctiles", (pw.cout + tile - 1) / tile);
        pw.w = dummy; pw.bias = dummy;
        const bool vel = num("vel", 1), has_dx = num("dx", 1);

        ConvKArgs ka;
        memset(&ka, 0, sizeof ka);
        ka.Dv = (int)num("Dv", 8); ka.Hv = (int)num("Hv", 30); ka.Wv = (int)num("Wv", 30);
        ka.H = (int)num("H", 32); ka.W = (int)num("W", 32); ka.D = ka.Dv + 2;
        ka.x = dummy; ka.dx = vel && has_dx ? dummy : nullptr; ka.y = dummy; ka.dy = vel ? dummy : nullptr;
        ka.w = dummy; ka.dw = vel ? dummy : nullptr; ka.bias = dummy;
        ka.in_pstride = num("pstride", (long)ka.H * ka.W * ka.D);
        ka.in2_pstride = num("pstride2", (long)ka.H * ka.W * ka.D);
        ka.in_off = num("in_off", 0); ka.osz = (int)num("osz", 1);
        ka.nchunk = pw.cin_pad / ck;
        ka.cout_groups = half ? (pw.cout + 7) / 8 : (pw.cout + 3) / 4;
        ka.flags = (num("res", 0) ? F_RES : 0) | (num("nodx", 0) ? F_SKIP_NODX : 0);
        ka.beta = num("beta", 0) ? dummy : nullptr;
        ka.ww = num("ww", 0) ? dummy : nullptr;
        ka.wws = num("wws", 0) ? dummy : nullptr;
        ka.stem_w = num("stem", 0) ? dummy : nullptr;
        ka.up8 = (int)num("up8", 0);
        const long csplit = num("csplit", 0), skip = num("skip", 0), s_csplit = num("s_csplit", 0);
        ka.csplit = csplit > 0 ? (int)(csplit / 16) : (1 << 30);
        if (csplit > 0) { ka.x2 = dummy; ka.dx2 = ka.dx; }
        ka.s_csplit = s_csplit > 0 ? (int)(s_csplit / 16) : (1 << 30);
        ka.nskip = (int)(skip / 16);
        if (skip > 0) { ka.xs = dummy; ka.dxs = dummy; ka.ws = dummy; ka.dws = dummy; ka.s_pstride = ka.s2_pstride = ka.in_pstride; }
        if (used != a.size()) { fprintf(stderr, "%s: unknown key\n", name.c_str()); rc = 2; }

        const ConvKernel k = conv_select(pw, ka, vel, has_dx);
        printf("%s\t%s\t%s\n", name.c_str(), conv_kernel_name(k), conv_label(k, pw, vel, has_dx).c_str());
    }
    return rc;
}
