// Serial walk of the per-particle bodies of csrc/nbe_fof.hip on the host, for a build under -fsanitize=address,undefined
// (host code only; nothing here touches a device).  It reads a case written by tools/fof_host_walk.py, runs the bodies in
// the order of the entry points (coordinates and keys, a std::sort of the keys, the link pass, the labels, the catalogue
// sums) and writes what they produced for the comparison with tests/fof_ref.py:
//
//     hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -o fof_host_walk tools/fof_host_walk.hip
//     python tools/fof_host_walk.py ./fof_host_walk
//
// Case file: int64 n, half, ncell, R2, nmin, has_velocity; float64 L; int32 e[3]; the displacement (3 n^3 float32 or
// float16); the velocity (3 n^3 float32) when has_velocity.  Result file: int64 count, rows, bad; X (3 count int32); root
// (count int32); label (rows int32); sums (rows, 6) int64.

#define NBE_FOF_BODIES_ONLY 1
#include "../jax_nbody_emulator_with_dj_amd/csrc/nbe_fof.hip"

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

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: %s CASE RESULT\n", argv[0]); return 2; }
    FILE* f = fopen(argv[1], "rb");
    if (!f) { perror(argv[1]); return 2; }
    const std::vector<int64_t> h = read_n<int64_t>(f, 6);
    const double L = read_n<double>(f, 1)[0];
    const std::vector<int> e = read_n<int>(f, 3);
    const long long n = h[0], R2 = h[3], nmin = h[4];
    const int half = (int)h[1], ncell = (int)h[2], has_vel = (int)h[5];
    const long long count = n * n * n;
    const std::vector<char> disp = read_n<char>(f, (size_t)(3 * count * (half ? 2 : 4)));
    const std::vector<float> vel = read_n<float>(f, has_vel ? (size_t)(3 * count) : 0);
    fclose(f);

    std::vector<int> X(3 * count), parent(count), sizes(count, 0);
    std::vector<long long> keys(count);
    long long bad = 0;
    for (long long x = 0; x < count; ++x) {                                     // fof_cells_kernel
        const long long i2 = x % n, rest = x / n, i1 = rest % n, i0 = rest / n;
        int X0 = 0, X1 = 0, X2 = 0;
        const bool ok = fof_coordinate(i0, n, fof_load_real(disp.data(), half, x), L, &X0) &
                        fof_coordinate(i1, n, fof_load_real(disp.data(), half, count + x), L, &X1) &
                        fof_coordinate(i2, n, fof_load_real(disp.data(), half, 2 * count + x), L, &X2);
        if (!ok) { ++bad; X0 = X1 = X2 = 0; }
        X[x] = X0; X[count + x] = X1; X[2 * count + x] = X2;
        keys[x] = fof_key(fof_cell(X0, ncell), fof_cell(X1, ncell), fof_cell(X2, ncell), ncell);
        parent[x] = (int)x;
    }
    std::vector<long long> order(count);
    std::iota(order.begin(), order.end(), 0LL);
    std::sort(order.begin(), order.end(), [&](long long a, long long b) { return keys[a] != keys[b] ? keys[a] < keys[b] : a > b; });
    std::vector<long long> sk(count);
    std::vector<FofParticle> P(count);
    for (long long j = 0; j < count; ++j) {                                     // fof_gather_kernel
        const long long p = order[j];
        sk[j] = keys[p];
        P[j] = FofParticle{X[p], X[count + p], X[2 * count + p], (int)p};
    }
    if (!bad)
        for (long long i = count - 1; i >= 0; --i)                              // fof_link_kernel, in an order of its own
            fof_link_particle(P.data(), sk.data(), count, i, ncell, R2, parent.data());
    for (long long x = 0; x < count; ++x) {                                     // fof_labels_kernel
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
    for (long long x = 0; x < count; ++x) {                                     // fof_catalog_kernel
        const int r = parent[x], s = slot[r];
        if (s < 0) continue;
        long long t[6];
        fof_terms(X.data(), count, x, r, has_vel ? vel.data() : nullptr, 0, qexp, t);
        for (int c = 0; c < 6; ++c) sums[6 * (size_t)s + c] += t[c];
    }

    FILE* o = fopen(argv[2], "wb");
    if (!o) { perror(argv[2]); return 2; }
    const int64_t head[3] = {count, (int64_t)label.size(), bad};
    fwrite(head, sizeof head, 1, o);
    fwrite(X.data(), sizeof(int), X.size(), o);
    fwrite(parent.data(), sizeof(int), parent.size(), o);
    fwrite(label.data(), sizeof(int), label.size(), o);
    fwrite(sums.data(), sizeof(long long), sums.size(), o);
    fclose(o);
    return 0;
}
