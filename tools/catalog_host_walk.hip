// Serial walk of the bodies of csrc/nbe_catalog.h on the host, for a build under -fsanitize=address,undefined (host code
// only; nothing here touches a device).  It reads a case written by tools/catalog_host_walk.py, runs the bodies in the order
// of the entry points (the coordinates and keys of every row, a std::sort of the keys, the records, then the walk of its
// mode) and writes what they produced for the comparison with tests/fof_ref.py, tests/pairs_ref.py or tests/profiles_ref.py:
//
//     hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -o catalog_host_walk tools/catalog_host_walk.hip
//     python tools/catalog_host_walk.py ./catalog_host_walk
//
// tests/test_catalog_host_walk.py builds the same program without the sanitizers and runs the same cases.
//
//     catalog_host_walk fof|pairs|profiles|velocity CASE RESULT
//
// A catalogue in a case file is (kind, rows) in the header and its array in the body.  kind: 0 (rows, 3) float32 positions,
// 1 (rows, 3) float64 positions, 2 a (3, n, n, n) float32 displacement with rows = n, 3 the same in float16, -1 no catalogue
// (B of an auto count).
//   fof       int64 kind, n, ncell, R2, nmin, has_velocity; float64 L; int32 e[3]; the displacement; the velocity (3 n^3
//             float32) when has_velocity.  Result: int64 count, rows, bad; X (3 count int32); root (count int32); label (rows
//             int32); sums (rows, 6) int64.
//   pairs     int64 kindA, rowsA, kindB, rowsB, ncell, nb, nmu, los; float64 L; int64 T[nb + 1]; A; B.  Result: int64 bad;
//             counts (nb, nmu) int64.
//   profiles  int64 kindA, rowsA, kindB, rowsB, ncell, nb; float64 L; int64 T[nb + 1]; the centres; the matter.  Result:
//             int64 bad; counts (rowsA, nb) int64 as a workgroup of 256 lanes walks a centre; the same for a wave of 64.
//   velocity  int64 kindA, rowsA, kindB, rowsB, ncell, nb, e, has_va; float64 L; int64 T[nb + 1]; A; with has_va the velocity of
//             A in the layout and dtype of A's kind; B; the velocity of B.  Result: int64 bad; the (nb, 6) words of
//             nbe_pair_velocity (zero without has_va); with a catalogue B the (rowsA, nb, 6) words of
//             nbe_halo_velocity_profiles as a workgroup of 256 lanes walks a centre (at rest without has_va), and as a wave of
//             64 does.  The program is held to tests/pairvel_ref.py (tests/test_pairvel_host_walk.py).

#include "../jax_nbody_emulator_with_dj_amd/csrc/nbe_catalog.h"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>

using namespace nbe;

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

template <typename T>
static void write_n(FILE* f, const std::vector<T>& v) { fwrite(v.data(), sizeof(T), v.size(), f); }

struct Catalogue {
    std::vector<int> X, parent;                            // (3, count) coordinates; the identity forest of a lattice
    std::vector<FofParticle> P;                            // the records in key order, and their keys
    std::vector<long long> sk;
    int bad = 0;
};

// nbe_fof_cells or nbe_pair_coords, the caller's sort, nbe_fof_gather
static Catalogue load(FILE* f, long long kind, long long rows, double L, int ncell) {
    Catalogue c;
    const bool lattice = kind >= 2;
    const long long count = lattice ? rows * rows * rows : rows;
    c.X.resize(3 * count);
    std::vector<long long> keys(count);
    if (lattice) {
        c.parent.resize(count);
        const std::vector<char> disp = read_n<char>(f, (size_t)(3 * count * (kind == 3 ? 2 : 4)));
        for (long long x = 0; x < count; ++x)
            fof_lattice_row(disp.data(), kind == 3, rows, count, L, ncell, x, c.X.data(), keys.data(), c.parent.data(), &c.bad);
    } else {
        const std::vector<char> pos = read_n<char>(f, (size_t)(3 * count * (kind ? 8 : 4)));
        for (long long x = 0; x < count; ++x)
            pair_position_row(pos.data(), (int)kind, count, L, ncell, x, c.X.data(), keys.data(), &c.bad);
    }
    std::vector<long long> order(count);
    std::iota(order.begin(), order.end(), 0LL);
    std::sort(order.begin(), order.end(), [&](long long a, long long b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a > b; });
    c.P.resize(count);
    c.sk.resize(count);
    for (long long j = 0; j < count; ++j) {
        c.P[j] = fof_gather_record(c.X.data(), order.data(), count, j);
        c.sk[j] = keys[order[j]];
    }
    return c;
}

// nbe_fof_link in an order of its own, nbe_fof_labels, the caller's choice of halos, nbe_fof_catalog
static void walk_fof(FILE* f, FILE* o) {
    const std::vector<int64_t> h = read_n<int64_t>(f, 6);
    const double L = read_n<double>(f, 1)[0];
    const std::vector<int> e = read_n<int>(f, 3);
    const long long n = h[1], R2 = h[3], nmin = h[4];
    const int ncell = (int)h[2], has_vel = (int)h[5];
    Catalogue c = load(f, h[0], n, L, ncell);
    const long long count = n * n * n;
    const std::vector<float> vel = read_n<float>(f, has_vel ? (size_t)(3 * count) : 0);

    std::vector<int>& parent = c.parent;
    if (!c.bad)
        for (long long i = count - 1; i >= 0; --i) fof_link_particle(c.P.data(), c.sk.data(), count, i, ncell, R2, parent.data());
    std::vector<int> sizes(count, 0);
    for (long long x = 0; x < count; ++x) {
        const int r = fof_root(parent.data(), (int)x);
        parent[x] = r;
        ++sizes[r];
    }
    std::vector<int> label;
    for (long long x = 0; x < count; ++x) if (sizes[x] >= nmin) label.push_back((int)x);
    std::stable_sort(label.begin(), label.end(), [&](int a, int b) { return sizes[a] > sizes[b]; });
    std::vector<int> slot(count, -1);
    for (size_t s = 0; s < label.size(); ++s) slot[label[s]] = (int)s;
    std::vector<long long> sums(6 * label.size(), 0);
    const int qexp[3] = {24 - e[0], 24 - e[1], 24 - e[2]};
    for (long long x = 0; x < count; ++x) {
        const int r = parent[x], s = slot[r];
        if (s < 0) continue;
        long long t[6];
        fof_terms(c.X.data(), count, x, r, has_vel ? vel.data() : nullptr, 0, qexp, t);
        for (int k = 0; k < 6; ++k) sums[6 * (size_t)s + k] += t[k];
    }

    const int64_t head[3] = {count, (int64_t)label.size(), c.bad};
    fwrite(head, sizeof head, 1, o);
    write_n(o, c.X);
    write_n(o, parent);
    write_n(o, label);
    write_n(o, sums);
}

// the "particles" form of nbe_pair_count, in an order of its own
static void walk_pairs(FILE* f, FILE* o) {
    const std::vector<int64_t> h = read_n<int64_t>(f, 8);
    const double L = read_n<double>(f, 1)[0];
    const int ncell = (int)h[4], nb = (int)h[5], nmu = (int)h[6], los = (int)h[7];
    const std::vector<long long> T = read_n<long long>(f, (size_t)nb + 1);
    const Catalogue A = load(f, h[0], h[1], L, ncell);
    const bool half = h[2] < 0;
    const Catalogue Bown = half ? Catalogue() : load(f, h[2], h[3], L, ncell);
    const Catalogue& B = half ? A : Bown;

    const int s = (int)pair_isqrt(T[nb]);
    std::vector<long long> counts((size_t)nb * nmu, 0);
    const int64_t bad = A.bad + B.bad;
    if (!bad)
        for (long long i = (long long)A.P.size() - 1; i >= 0; --i)
            pair_count_particle(A.P.data(), i, B.P.data(), B.sk.data(), (long long)B.P.size(), ncell, half, T.data(), nb, s, nmu,
                                los, [&](int entry) { if (entry >= 0) ++counts.at((size_t)entry); });
    fwrite(&bad, sizeof bad, 1, o);
    write_n(o, counts);
}

// one centre as a group of `lanes` lanes takes it: the ranges by lanes 0 .. 17, the image, the row
static void walk_centre(const FofParticle& me, const Catalogue& B, int ncell, const std::vector<long long>& T, int nb, int s,
                        int lanes, std::vector<long long>& counts) {
    std::vector<long long> rlo(kPairRanges), rlen(kPairRanges);                 // exact sizes: an overrun is reported
    for (int t = 0; t < kPairRanges; ++t) profile_range(me, B.sk.data(), (long long)B.P.size(), ncell, t, rlo.data(), rlen.data());
    const long long total = pair_ranges_total(rlen.data());
    std::vector<unsigned int> image((size_t)nb, 0u);
    for (int lane = lanes - 1; lane >= 0; --lane)
        profile_stream(me, B.P.data(), rlo.data(), rlen.data(), total, lane, lanes, T.data(), nb, s,
                       [&](int b) { if (b >= 0) ++image.at((size_t)b); });
    for (int b = 0; b < nb; ++b) counts.at((size_t)me.p * nb + b) = image[(size_t)b];
}

// both forms of nbe_halo_profiles: the strides of profile_group_kernel (256) and of profile_wave_kernel (64)
static void walk_profiles(FILE* f, FILE* o) {
    const std::vector<int64_t> h = read_n<int64_t>(f, 6);
    const double L = read_n<double>(f, 1)[0];
    const int ncell = (int)h[4], nb = (int)h[5];
    const std::vector<long long> T = read_n<long long>(f, (size_t)nb + 1);
    const Catalogue A = load(f, h[0], h[1], L, ncell);
    const Catalogue B = load(f, h[2], h[3], L, ncell);

    const int s = (int)pair_isqrt(T[nb]);
    const int64_t bad = A.bad + B.bad;
    std::vector<long long> group(A.P.size() * (size_t)nb, -1), wave(A.P.size() * (size_t)nb, -1);   // -1: a row never written
    if (!bad)
        for (const FofParticle& me : A.P) {
            walk_centre(me, B, ncell, T, nb, s, 256, group);
            walk_centre(me, B, ncell, T, nb, s, 64, wave);
        }
    fwrite(&bad, sizeof bad, 1, o);
    write_n(o, group);
    write_n(o, wave);
}

// nbe_velocity_words: the velocity of a catalogue of `kind` (its layout and dtype) as records beside c.P
static std::vector<VelWord> load_words(FILE* f, long long kind, const Catalogue& c, int e) {
    const long long count = (long long)c.P.size();
    const int dtype = kind == 1 ? NBE_F64 : kind == 3 ? NBE_F16 : NBE_F32;
    const std::vector<char> vel = read_n<char>(f, (size_t)(3 * count * (kind == 1 ? 8 : kind == 3 ? 2 : 4)));
    std::vector<VelWord> w((size_t)count);
    for (long long j = 0; j < count; ++j) w[(size_t)j] = velocity_gather_record(vel.data(), dtype, kind >= 2, count, e, c.P.data(), j);
    return w;
}

// one centre as a group of `lanes` lanes takes it in nbe_halo_velocity_profiles: the ranges, the image of 6 nb words, the row
static void walk_velocity_centre(const FofParticle& me, const VelWord& mine, const Catalogue& B, const std::vector<VelWord>& WB,
                                 int ncell, const std::vector<long long>& T, int nb, int s, int lanes,
                                 std::vector<long long>& sums) {
    std::vector<long long> rlo(kPairRanges), rlen(kPairRanges);
    for (int t = 0; t < kPairRanges; ++t) profile_range(me, B.sk.data(), (long long)B.P.size(), ncell, t, rlo.data(), rlen.data());
    const long long total = pair_ranges_total(rlen.data());
    std::vector<unsigned long long> image((size_t)nb * kVelSums, 0ull);
    for (int lane = lanes - 1; lane >= 0; --lane)
        profile_velocity_stream(me, mine, B.P.data(), WB.data(), rlo.data(), rlen.data(), total, lane, lanes, T.data(), nb, s,
                                [&](int at, unsigned long long v) { image.at((size_t)at) += v; });
    for (int k = 0; k < nb * kVelSums; ++k) sums.at((size_t)me.p * nb * kVelSums + k) = (long long)image[(size_t)k];
}

// nbe_pair_velocity in an order of its own (with a velocity of A), and with a catalogue B both forms of
// nbe_halo_velocity_profiles in strides of 256 and of 64
static void walk_velocity(FILE* f, FILE* o) {
    const std::vector<int64_t> h = read_n<int64_t>(f, 8);
    const double L = read_n<double>(f, 1)[0];
    const int ncell = (int)h[4], nb = (int)h[5], e = (int)h[6];
    const bool has_va = h[7] != 0, half = h[2] < 0;
    const std::vector<long long> T = read_n<long long>(f, (size_t)nb + 1);
    const Catalogue A = load(f, h[0], h[1], L, ncell);
    const std::vector<VelWord> WA = has_va ? load_words(f, h[0], A, e) : std::vector<VelWord>();
    const Catalogue Bown = half ? Catalogue() : load(f, h[2], h[3], L, ncell);
    const std::vector<VelWord> WBown = half ? std::vector<VelWord>() : load_words(f, h[2], Bown, e);
    const Catalogue& B = half ? A : Bown;
    const std::vector<VelWord>& WB = half ? WA : WBown;

    const int s = (int)pair_isqrt(T[nb]);
    const int64_t bad = A.bad + B.bad;
    std::vector<unsigned long long> pairs((size_t)nb * kVelSums, 0ull);
    if (!bad && has_va)
        for (long long i = (long long)A.P.size() - 1; i >= 0; --i)
            pair_velocity_particle(A.P.data(), WA.data(), i, B.P.data(), WB.data(), B.sk.data(), (long long)B.P.size(), ncell, half,
                                   T.data(), nb, s, [&](int at, unsigned long long v) { pairs.at((size_t)at) += v; });
    fwrite(&bad, sizeof bad, 1, o);
    write_n(o, pairs);
    if (half) return;
    const size_t rows = A.P.size() * (size_t)nb * kVelSums;
    std::vector<long long> group(rows, -1), wave(rows, -1);                     // -1: a word never written
    const VelWord rest = {0, 0, 0, 0};
    if (!bad)
        for (size_t j = 0; j < A.P.size(); ++j) {
            walk_velocity_centre(A.P[j], has_va ? WA[j] : rest, B, WB, ncell, T, nb, s, 256, group);
            walk_velocity_centre(A.P[j], has_va ? WA[j] : rest, B, WB, ncell, T, nb, s, 64, wave);
        }
    write_n(o, group);
    write_n(o, wave);
}

int main(int argc, char** argv) {
    void (*walk)(FILE*, FILE*) = nullptr;
    if (argc == 4) walk = !strcmp(argv[1], "fof") ? walk_fof : !strcmp(argv[1], "pairs") ? walk_pairs :
                          !strcmp(argv[1], "profiles") ? walk_profiles : !strcmp(argv[1], "velocity") ? walk_velocity : nullptr;
    if (!walk) { fprintf(stderr, "usage: %s fof|pairs|profiles|velocity CASE RESULT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[2], "rb");
    if (!f) { perror(argv[2]); return 2; }
    FILE* o = fopen(argv[3], "wb");
    if (!o) { perror(argv[3]); return 2; }
    walk(f, o);
    fclose(f);
    return fclose(o) ? 2 : 0;
}
