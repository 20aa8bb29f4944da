// error_bounded_lod.cpp -- level of detail bounded by error, from C++ through the C ABI: what every cut of four 16^3
// bricks costs against their own full-depth decode (vrhip::error_table), the per-brick cuts that cost nothing
// (vrhip::select_error_bounded, bound 0), and the proof: the FNV-1a-64 hash of vr_brickset_decode_lod at those cuts next
// to the hash of the full decode.  Plain C++ (g++), no HIP headers.  tests/test_error_table_cpu.py builds it;
// tests/test_gpu_error_table.py runs it and compares its table with the Python one.
//
//   g++ -std=c++14 -O2 -Iinclude examples/error_bounded_lod.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/error_bounded_lod
//   /tmp/error_bounded_lod [bricks.raw]      bricks.raw: 4 x 4096 bytes to use in place of the built-in bricks
// prints, per brick, "brick b max_abs <one value per cut 0 .. max_tree_depth>", then "cuts <four cuts>", then
// "lod fnv1a64 <16 hex digits> full fnv1a64 <16 hex digits>".
#include "vrhip/CutError.hpp"
#include <cstdio>
#include <vector>

static const int N = 16, B = 4;
static const int64_t V = (int64_t)N * N * N;

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

static uint64_t fnv1a64(const std::vector<uint8_t> &v)
{
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < v.size(); ++i) { h ^= v[i]; h *= 1099511628211ull; }
    return h;
}

// a constant brick, two flat halves, a noisy ramp, a noisy ball: from "any cut will do" to "every level counts"
static std::vector<uint8_t> builtin_bricks()
{
    std::vector<uint8_t> vox((size_t)(B * V));
    uint32_t lcg = 12345u;
    for (int z = 0; z < N; ++z)
        for (int y = 0; y < N; ++y)
            for (int x = 0; x < N; ++x) {
                const size_t i = (size_t)x + (size_t)N * ((size_t)y + (size_t)N * (size_t)z);
                lcg = lcg * 1664525u + 1013904223u;
                const int noise = (int)((lcg >> 24) & 3u);
                const int dx = 2 * x - (N - 1), dy = 2 * y - (N - 1), dz = 2 * z - (N - 1);
                vox[i] = 90;
                vox[(size_t)V + i] = (uint8_t)(z <= 7 ? 40 : 200);
                vox[(size_t)(2 * V) + i] = (uint8_t)(8 * z + 5 * y + 2 * x + noise);
                vox[(size_t)(3 * V) + i] = (uint8_t)((dx * dx + dy * dy + dz * dz < 170 ? 200 : 20) + noise);
            }
    return vox;
}

int main(int argc, char **argv)
{
    std::vector<uint8_t> vox = builtin_bricks();
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "rb");
        const size_t got = f ? std::fread(vox.data(), 1, vox.size(), f) : 0;
        if (f) std::fclose(f);
        if (got != vox.size()) { std::fprintf(stderr, "%s: expected %zu bytes\n", argv[1], vox.size()); return 1; }
    }
    const int64_t dims[3] = {N, N, N};
    vr_brickset *set = nullptr;
    void *dvox = nullptr, *dfull = nullptr, *dlod = nullptr, *dscratch = nullptr;
    vr_status s;
    if ((s = vr_brickset_create(&set, B, dims, /*tolerance*/ 2, /*max_epochs*/ 3, VR_VARIANT_RECOVER)) != VR_OK) return fail("vr_brickset_create", s);
    void **bufs[4] = {&dvox, &dfull, &dlod, &dscratch};
    for (int k = 0; k < 4; ++k) if ((s = vr_malloc(bufs[k], B * V)) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvox, vox.data(), B * V, nullptr)) != VR_OK) return fail("vr_upload", s);
    if ((s = vr_brickset_build(set, (const uint8_t *)dvox, nullptr)) != VR_OK) return fail("vr_brickset_build", s);
    if ((s = vr_brickset_decode(set, -1, (uint8_t *)dfull, nullptr)) != VR_OK) return fail("vr_brickset_decode", s);
    std::vector<uint8_t> full((size_t)(B * V)), lod((size_t)(B * V), 0);
    if ((s = vr_download(full.data(), dfull, B * V, nullptr)) != VR_OK) return fail("vr_download", s);

    try {
        // the reference is the set's own full-depth decode: a cut with max_abs 0 reproduces it bit for bit
        const vrhip::ErrorTable table = vrhip::error_table(set, (const uint8_t *)dfull, (uint8_t *)dscratch, B);
        for (int b = 0; b < B; ++b) {
            std::printf("brick %d max_abs", b);
            for (int c = table.cut_lo; c <= table.cut_hi; ++c) std::printf(" %u", (unsigned)table.at(c, b).max_abs);
            std::printf("\n");
        }
        const std::vector<int32_t> cuts = vrhip::select_error_bounded(table, 0);
        std::printf("cuts");
        for (int b = 0; b < B; ++b) std::printf(" %d", (int)cuts[(size_t)b]);
        std::printf("\n");
        if ((s = vr_brickset_decode_lod(set, cuts.data(), (uint8_t *)dlod, nullptr)) != VR_OK) return fail("vr_brickset_decode_lod", s);
        if ((s = vr_download(lod.data(), dlod, B * V, nullptr)) != VR_OK) return fail("vr_download", s);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    std::printf("lod fnv1a64 %016llx full fnv1a64 %016llx\n", (unsigned long long)fnv1a64(lod), (unsigned long long)fnv1a64(full));
    for (int k = 0; k < 4; ++k) vr_free(*bufs[k]);
    vr_brickset_destroy(set);
    return 0;
}
