// archive_playback.cpp -- encode once, store, play back: two timesteps of four 32^3 bricks are built and saved as
// brick-set archives (vrhip::archive::save); the first is opened as a new set, the second loaded into the same set
// (the decode index is rebuilt on the GPU each time, no stream is parsed on the host), and every decode -- full depth,
// a cut inside the index and a cut above it -- is compared with the built set's own.  Prints "OK".  Plain C++ (g++), no
// HIP headers.  tests/test_archive_facade_cpp.py builds and runs it.
//
//   g++ -std=c++14 -O2 -Iinclude examples/archive_playback.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/archive_playback
//   /tmp/archive_playback <directory for the two files>
#include "vrhip/BrickArchive.hpp"
#include <cstdio>
#include <exception>
#include <vector>

static const int N = 32, B = 4;
static const int64_t V = (int64_t)N * N * N;

static std::vector<uint8_t> timestep(int t)
{
    std::vector<uint8_t> vox((size_t)(B * V));
    uint32_t lcg = 777u + (uint32_t)t;
    for (int b = 0; b < B; ++b)
        for (int z = 0; z < N; ++z)
            for (int y = 0; y < N; ++y)
                for (int x = 0; x < N; ++x) {
                    lcg = lcg * 1664525u + 1013904223u;
                    const int dx = x - 12 - 3 * t - b, dy = y - 16, dz = z - 14 + b;
                    const int r2 = dx * dx + dy * dy + dz * dz;
                    const int v = r2 < 90 + 20 * b ? 210 - r2 : (b == 3 ? 0 : 20 + (int)((lcg >> 24) & 3u));
                    vox[(size_t)b * (size_t)V + (size_t)x + (size_t)N * ((size_t)y + (size_t)N * (size_t)z)] = (uint8_t)v;
                }
    return vox;
}

static std::vector<uint8_t> decode(vr_brickset *set, int cut, void *dev)
{
    vrhip::archive::require(vr_brickset_decode(set, cut, (uint8_t *)dev, nullptr), "vr_brickset_decode");
    std::vector<uint8_t> out((size_t)(B * V));
    vrhip::archive::require(vr_download(out.data(), dev, B * V, nullptr), "vr_download");
    return out;
}

int main(int argc, char **argv)
{
    if (argc != 2) { std::fprintf(stderr, "usage: archive_playback <directory>\n"); return 2; }
    try {
        using vrhip::archive::require;
        const int64_t dims[3] = {N, N, N};
        void *dvox = nullptr, *dout = nullptr;
        require(vr_malloc(&dvox, B * V), "vr_malloc");
        require(vr_malloc(&dout, B * V), "vr_malloc");
        const int cuts[3] = {-1, 12, 4};          // full depth; inside the index (depth 15 - 6 = 9 and below); above it
        std::vector<std::vector<uint8_t>> want;
        std::vector<std::string> paths;
        for (int t = 0; t < 2; ++t) {
            vr_brickset *raw = nullptr;
            require(vr_brickset_create(&raw, B, dims, /*tolerance*/ 2, /*max_epochs*/ 2, VR_VARIANT_RECOVER), "vr_brickset_create");
            vrhip::BrickSetHandle built(raw);
            const std::vector<uint8_t> vox = timestep(t);
            require(vr_upload(dvox, vox.data(), B * V, nullptr), "vr_upload");
            require(vr_brickset_build(built.get(), (const uint8_t *)dvox, nullptr), "vr_brickset_build");
            for (int k = 0; k < 3; ++k) want.push_back(decode(built.get(), cuts[k], dout));
            paths.push_back(std::string(argv[1]) + "/timestep" + std::to_string(t) + ".vrbs");
            vrhip::archive::save(built.get(), paths.back());
        }
        bool same = true;
        vrhip::BrickSetHandle set = vrhip::archive::open(paths[0]);
        for (int k = 0; k < 3; ++k) same = same && decode(set.get(), cuts[k], dout) == want[(size_t)k];
        vrhip::archive::load(set.get(), paths[1]);
        for (int k = 0; k < 3; ++k) same = same && decode(set.get(), cuts[k], dout) == want[(size_t)(3 + k)];
        vr_tree_info ti;
        require(vr_brickset_info(set.get(), 0, &ti), "vr_brickset_info");
        std::printf("played back 2 timesteps of %d bricks; brick 0 of the second holds %lld tokens\n", B, (long long)ti.num_active_nodes);
        vr_free(dvox);
        vr_free(dout);
        if (!same) { std::fprintf(stderr, "a decode of the archive differs from the built set's\n"); return 1; }
        std::printf("OK\n");
        return 0;
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return 1;
    }
}
