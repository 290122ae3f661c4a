// Serial walk of the per-centre bodies of csrc/nbe_profiles.hip on the host, for a build under
// -fsanitize=address,undefined (host code only; nothing here touches a device).  It reads a case written by
// tools/profiles_host_walk.py, runs the bodies in the order of the entry points (coordinates and keys, a std::sort of the
// keys, the records, then every centre as the kernels take it: the 18 ranges, and the ranges end to end in the strides of
// 256 and of 64 lanes) and writes the count table of each form for the comparison with tests/profiles_ref.py:
//
//     hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -o profiles_host_walk tools/profiles_host_walk.hip
//     python tools/profiles_host_walk.py ./profiles_host_walk
//
// Case file: int64 kindA, rowsA, kindB, rowsB, ncell, nb; float64 L; int64 T[nb + 1]; the centres; the matter.  kind: 0
// (rows, 3) float32 positions, 1 (rows, 3) float64 positions, 2 a (3, n, n, n) float32 displacement with rows = n.  Result
// file: int64 bad; counts (rowsA, nb) int64 of the workgroup form; the same of the wave form.

#define NBE_PROFILES_BODIES_ONLY 1
#include "../jax_nbody_emulator_with_dj_amd/csrc/nbe_profiles.hip"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <numeric>
#include <vector>

namespace nbe { int api_fail(const char* msg) { fprintf(stderr, "%s\n", msg); return 1; } }

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

struct Catalogue {
    std::vector<FofParticle> P;
    std::vector<long long> sk;
    long long bad = 0;
};

static Catalogue load(FILE* f, long long kind, long long rows, double L, int ncell) {
    Catalogue c;
    const long long count = kind == 2 ? rows * rows * rows : rows;
    std::vector<int> X(3 * count);
    std::vector<long long> keys(count);
    if (kind == 2) {                                                            // fof_cells_kernel
        const long long n = rows;
        const std::vector<float> disp = read_n<float>(f, (size_t)(3 * count));
        for (long long x = 0; x < count; ++x) {
            const long long i2 = x % n, rest = x / n, i1 = rest % n, i0 = rest / n;
            int X0 = 0, X1 = 0, X2 = 0;
            const bool ok = fof_coordinate(i0, n, disp[x], L, &X0) & fof_coordinate(i1, n, disp[count + x], L, &X1) &
                            fof_coordinate(i2, n, disp[2 * count + x], L, &X2);
            if (!ok) { ++c.bad; X0 = X1 = X2 = 0; }
            X[x] = X0; X[count + x] = X1; X[2 * count + x] = X2;
        }
    } else {                                                                    // pair_coords_kernel
        const std::vector<char> pos = read_n<char>(f, (size_t)(3 * count * (kind ? 8 : 4)));
        for (long long x = 0; x < count; ++x) {
            int X0 = 0, X1 = 0, X2 = 0;
            const bool ok = pair_coordinate(pair_load_real(pos.data(), (int)kind, 3 * x), L, &X0) &
                            pair_coordinate(pair_load_real(pos.data(), (int)kind, 3 * x + 1), L, &X1) &
                            pair_coordinate(pair_load_real(pos.data(), (int)kind, 3 * x + 2), L, &X2);
            if (!ok) { ++c.bad; X0 = X1 = X2 = 0; }
            X[x] = X0; X[count + x] = X1; X[2 * count + x] = X2;
        }
    }
    for (long long x = 0; x < count; ++x)
        keys[x] = fof_key(fof_cell(X[x], ncell), fof_cell(X[count + x], ncell), fof_cell(X[2 * count + x], ncell), ncell);
    std::vector<long long> order(count);
    std::iota(order.begin(), order.end(), 0LL);
    std::sort(order.begin(), order.end(), [&](long long a, long long b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a > b; });
    c.P.resize(count);
    c.sk.resize(count);
    for (long long j = 0; j < count; ++j) {                                     // fof_gather_kernel
        const long long p = order[j];
        c.sk[j] = keys[p];
        c.P[j] = FofParticle{X[p], X[count + p], X[2 * count + p], (int)p};
    }
    return c;
}

// one centre as a group of `lanes` lanes takes it: the ranges by lanes 0 .. 17, the image, the row
static void walk_centre(const FofParticle& me, const Catalogue& B, int ncell, const std::vector<long long>& T, int nb, int s,
                        int lanes, std::vector<long long>& counts) {
    std::vector<long long> rlo(kPairRanges), rlen(kPairRanges);                 // exact sizes: an overrun is reported
    for (int t = 0; t < kPairRanges; ++t) profile_range(me, B.sk.data(), (long long)B.P.size(), ncell, t, rlo.data(), rlen.data());
    const long long total = profile_total(rlen.data());
    std::vector<unsigned int> image((size_t)nb, 0u);
    for (int lane = lanes - 1; lane >= 0; --lane)
        profile_stream(me, B.P.data(), rlo.data(), rlen.data(), total, lane, lanes, T.data(), nb, s,
                       [&](int b) { if (b >= 0) ++image.at((size_t)b); });
    for (int b = 0; b < nb; ++b) counts.at((size_t)me.p * nb + b) = image[(size_t)b];
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASE RESULT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int64_t> h = read_n<int64_t>(f, 6);
    const double L = read_n<double>(f, 1)[0];
    const int ncell = (int)h[4], nb = (int)h[5];
    const std::vector<long long> T = read_n<long long>(f, (size_t)nb + 1);
    const Catalogue A = load(f, h[0], h[1], L, ncell);
    const Catalogue B = load(f, h[2], h[3], L, ncell);
    fclose(f);

    const int s = (int)pair_isqrt(T[nb]);
    const long long bad = A.bad + B.bad;
    std::vector<long long> group(A.P.size() * (size_t)nb, -1), wave(A.P.size() * (size_t)nb, -1);   // -1: a row never written
    if (!bad)
        for (const FofParticle& me : A.P) {
            walk_centre(me, B, ncell, T, nb, s, kProfileThreads, group);
            walk_centre(me, B, ncell, T, nb, s, kProfileWave, wave);
        }

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t head[1] = {bad};
    fwrite(head, sizeof head, 1, o);
    fwrite(group.data(), sizeof(long long), group.size(), o);
    fwrite(wave.data(), sizeof(long long), wave.size(), o);
    fclose(o);
    return 0;
}
