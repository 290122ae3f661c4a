// Serial walk of the bodies of csrc/nbe_web.h on the host, for a build under -fsanitize=address,undefined (host code only;
// nothing here touches a device).  It reads a case written by tools/web_host_walk.py, runs web_eigenvalues on every tensor
// and web_type on the words it returned under every threshold, and writes both for the comparison with tests/web_ref.py:
//
//     hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//         -o web_host_walk tools/web_host_walk.hip
//     python tools/web_host_walk.py ./web_host_walk
//
// tests/test_web_host_walk.py builds the same program without the sanitizers and runs the same cases.
//
//     web_host_walk CASE RESULT
//
// CASE: int64 count, nthresholds; float32 thresholds[nthresholds]; float32 tensor[6][count] in the pair order (0,0), (1,1),
// (2,2), (0,1), (0,2), (1,2).  RESULT: float32 eig[3][count]; uint8 types[nthresholds][count], 255 for a voxel without one.

#include "../jax_nbody_emulator_with_dj_amd/csrc/nbe_web.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

template <typename T>
static std::vector<T> read_n(FILE* f, size_t n) {
    std::vector<T> v(n);
    if (n && fread(v.data(), sizeof(T), n, f) != n) { fprintf(stderr, "short read\n"); exit(2); }
    return v;
}

int main(int argc, char** argv) {
    if (argc != 3) { fprintf(stderr, "usage: web_host_walk CASE RESULT\n"); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    const std::vector<long long> head = read_n<long long>(in, 2);
    const long long count = head[0], nth = head[1];
    if (count < 0 || count > (1LL << 28) || nth < 1 || nth > 64) { fprintf(stderr, "bad header\n"); return 2; }
    const std::vector<float> th = read_n<float>(in, (size_t)nth);
    const std::vector<float> h = read_n<float>(in, (size_t)(6 * count));
    fclose(in);

    std::vector<float> eig((size_t)(3 * count));
    std::vector<unsigned char> types((size_t)(nth * count));
    for (long long i = 0; i < count; ++i) {
        float e[3];
        nbe::web_eigenvalues(h[i], h[count + i], h[2 * count + i], h[3 * count + i], h[4 * count + i], h[5 * count + i], e);
        for (int c = 0; c < 3; ++c) eig[c * count + i] = e[c];
        for (long long t = 0; t < nth; ++t) {
            const int m = nbe::web_type(e[0], e[1], e[2], th[t]);
            types[t * count + i] = m == nbe::kWebNaN ? nbe::kWebNaNType : (unsigned char)m;
        }
    }
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    fwrite(eig.data(), sizeof(float), eig.size(), out);
    fwrite(types.data(), 1, types.size(), out);
    fclose(out);
    return 0;
}
