// histogram.cpp -- what values a volume holds, from C++ through the C ABI: the histograms of a 32 x 24 x 20 volume taken
// as four bricks (vrhip::Histogram::of_bricks), of a small hand-made pool with a full, an absent and a coarse cell
// (of_pool), the joint table of value and gradient magnitude (vrhip::histogram2d), and the display window between the
// 5th and the 95th percentile (vrhip::window_from_histogram).  Plain C++ (g++), no HIP headers.
// tests/test_histogram_cpu.py builds it; tests/test_gpu_histogram.py runs it and compares its hashes with Python's.
//
//   g++ -std=c++14 -O2 -Iinclude examples/histogram.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/histogram
//   /tmp/histogram [volume.raw]      volume.raw: 32 * 24 * 20 bytes, x fastest, to use in place of the built-in volume
// prints the FNV-1a-64 of each table's bytes, "<name> fnv1a64 <16 hex digits>" for bricks, total, pool_cells,
// pool_total and hist2d, then "window <lo> <hi>".
#include "vrhip/Histogram.hpp"
#include <cstdio>
#include <vector>

static const int64_t X = 32, Y = 24, Z = 20, N = X * Y * Z;
static const int32_t B = 4;

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

template <class T> static uint64_t fnv1a64(const std::vector<T> &v)
{
    const uint8_t *p = (const uint8_t *)v.data();
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

// an empty border, a noisy ball, a flat slab: a background bin, a spread of values and a few strong edges
static std::vector<uint8_t> builtin_volume()
{
    std::vector<uint8_t> vox((size_t)N);
    uint32_t lcg = 2024u;
    for (int64_t z = 0; z < Z; ++z)
        for (int64_t y = 0; y < Y; ++y)
            for (int64_t x = 0; x < X; ++x) {
                lcg = lcg * 1664525u + 1013904223u;
                const int noise = (int)((lcg >> 24) & 7u);
                const int64_t dx = 2 * x - (X - 1), dy = 2 * y - (Y - 1), dz = 2 * z - (Z - 1);
                int v = 0;
                if (dx * dx + dy * dy + dz * dz < 300) v = 150 + 4 * noise;
                else if (z >= 15 && z < 18) v = 60;
                vox[(size_t)(x + X * (y + Y * z))] = (uint8_t)v;
            }
    return vox;
}

int main(int argc, char **argv)
{
    std::vector<uint8_t> vox = builtin_volume();
    if (argc > 1) {
        FILE *f = std::fopen(argv[1], "rb");
        const size_t got = f ? std::fread(vox.data(), 1, vox.size(), f) : 0;
        if (f) std::fclose(f);
        if (got != vox.size()) { std::fprintf(stderr, "%s: expected %zu bytes\n", argv[1], vox.size()); return 1; }
    }
    void *dvox = nullptr, *dtab = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvox, N)) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvox, vox.data(), N, nullptr)) != VR_OK) return fail("vr_upload", s);
    // a pool in the volume's first 576 bytes: an 8^3 cell at full resolution, an absent cell, a cell stored as 4^3
    const int64_t bd[3] = {8, 8, 8}, grid[3] = {3, 1, 1}, dims[3] = {X, Y, Z};
    vr_pool_entry tab[3] = {{0, {0, 0, 0}, {0, 0, 0, 0, 0}}, {-1, {0, 0, 0}, {0, 0, 0, 0, 0}}, {512, {1, 1, 1}, {0, 0, 0, 0, 0}}};
    if ((s = vr_malloc(&dtab, (int64_t)sizeof(tab))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dtab, tab, (int64_t)sizeof(tab), nullptr)) != VR_OK) return fail("vr_upload", s);
    try {
        const vrhip::Histogram bricks = vrhip::Histogram::of_bricks((const uint8_t *)dvox, B, N / B);
        const vrhip::Histogram pool = vrhip::Histogram::of_pool((const uint8_t *)dvox, (const vr_pool_entry *)dtab, bd, grid);
        const std::vector<uint64_t> h2 = vrhip::histogram2d((const uint8_t *)dvox, dims);
        const vrhip::Window w = vrhip::window_from_histogram(bricks.total, 0, 0.05, 0.95);
        std::printf("bricks fnv1a64 %016llx\n", (unsigned long long)fnv1a64(bricks.parts));
        std::printf("total fnv1a64 %016llx\n", (unsigned long long)fnv1a64(bricks.total));
        std::printf("pool_cells fnv1a64 %016llx\n", (unsigned long long)fnv1a64(pool.parts));
        std::printf("pool_total fnv1a64 %016llx\n", (unsigned long long)fnv1a64(pool.total));
        std::printf("hist2d fnv1a64 %016llx\n", (unsigned long long)fnv1a64(h2));
        std::printf("window %.9g %.9g\n", (double)w.lo, (double)w.hi);
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
    vr_free(dtab);
    vr_free(dvox);
    return 0;
}
