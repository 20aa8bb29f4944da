// isomesh.cpp -- the iso-surface of a small analytic ball as a triangle mesh, from C++ through the C ABI
// (vrhip::IsoMesher, vrhip/IsoMesh.hpp): counts, emits, downloads, and writes a PLY.  Plain C++ (g++), no HIP headers.
// tests/test_isomesh_cpu.py builds it; tests/test_gpu_isomesh.py runs it and compares its hashes with Python's.
//
//   g++ -std=c++14 -O2 -Iinclude examples/isomesh.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/isomesh
//   /tmp/isomesh [out.ply]
// The ball: a 24^3 volume, v = max(0, 255 - 255 r2 / 400) in integers with r2 = the squared distance from the centre
// in half voxels; iso_value 0.5, capped, with gradients.  Prints "vertices <V>", "triangles <T>", the FNV-1a-64 of the
// position, gradient and index bytes as "<name> fnv1a64 <16 hex digits>", then "OK".
#include "vrhip/IsoMesh.hpp"
#include <cstdio>
#include <vector>

static const int64_t N = 24;

template <class T> static uint64_t fnv1a64(const std::vector<T> &v)
{
    const uint8_t *p = (const uint8_t *)v.data();
    uint64_t h = 14695981039346656037ull;
    for (size_t i = 0; i < v.size() * sizeof(T); ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}

int main(int argc, char **argv)
{
    std::vector<uint8_t> vox((size_t)(N * N * N));
    for (int64_t z = 0; z < N; ++z)
        for (int64_t y = 0; y < N; ++y)
            for (int64_t x = 0; x < N; ++x) {
                const int64_t dx = 2 * x - (N - 1), dy = 2 * y - (N - 1), dz = 2 * z - (N - 1);
                const int64_t v = 255 - 255 * (dx * dx + dy * dy + dz * dz) / 400;
                vox[(size_t)(x + N * (y + N * z))] = (uint8_t)(v < 0 ? 0 : v);
            }
    void *dvox = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvox, N * N * N)) != VR_OK || (s = vr_upload(dvox, vox.data(), N * N * N, nullptr)) != VR_OK) {
        std::fprintf(stderr, "device volume: %s\n", vr_status_string(s));
        return 1;
    }
    int rc = 0;
    try {
        const int64_t dims[3] = {N, N, N};
        vrhip::IsoMesher mesher;
        const vrhip::Mesh m = mesher.extract((const uint8_t *)dvox, dims, vrhip::IsoMesher::whole(dims, 0.5f, true), true);
        std::printf("vertices %zu\ntriangles %zu\n", m.num_vertices(), m.num_triangles());
        std::printf("positions fnv1a64 %016llx\n", (unsigned long long)fnv1a64(m.positions));
        std::printf("gradients fnv1a64 %016llx\n", (unsigned long long)fnv1a64(m.gradients));
        std::printf("indices fnv1a64 %016llx\n", (unsigned long long)fnv1a64(m.indices));
        if (argc > 1 && !vrhip::write_ply(argv[1], m)) {
            std::fprintf(stderr, "cannot write %s\n", argv[1]);
            rc = 1;
        }
    } catch (const std::exception &e) {
        std::fprintf(stderr, "%s\n", e.what());
        rc = 1;
    }
    vr_free(dvox);
    if (rc == 0) std::printf("OK\n");
    return rc;
}
