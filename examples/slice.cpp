// slice.cpp -- an axial slice and an oblique thick slab (a slab MIP) of a synthetic volume from C++, through the C ABI
// (vrhip::Slicer over vr_reslice), and the FNV-1a-64 hash of each frame's bytes.  Plain C++ (g++), no HIP headers.
// tests/test_reslice_cpu.py builds it; tests/test_gpu_reslice.py compares the hashes with the Python frames'.
//
//   g++ -std=c++14 -O2 -Iinclude examples/slice.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/slice
//   /tmp/slice                 prints "slice 48 x 40 fnv1a64 <16 hex digits>" and "slice 96 x 64 fnv1a64 <...>"
#include "vrhip/Slice.hpp"
#include <cstdio>
#include <vector>

static const int X = 48, Y = 40, Z = 32;

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

// draws the slice and prints its hash
static int show(const vrhip::Slicer &sl, const uint8_t *dvol, const int64_t dims[3])
{
    const int W = sl.plane.width, H = sl.plane.height;
    void *dimg = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dimg, (int64_t)W * H * 4 * sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = sl.frame(dvol, dims, (float *)dimg)) != VR_OK) return fail("vr_reslice", s);
    std::vector<float> img((size_t)W * H * 4);
    if ((s = vr_download(img.data(), dimg, (int64_t)img.size() * (int64_t)sizeof(float), nullptr)) != VR_OK) return fail("vr_download", s);
    vr_free(dimg);
    uint64_t h = 14695981039346656037ull;           // FNV-1a, 64 bits, over the frame's bytes
    const unsigned char *b = (const unsigned char *)img.data();
    for (size_t i = 0; i < img.size() * sizeof(float); ++i) { h ^= b[i]; h *= 1099511628211ull; }
    std::printf("slice %d x %d fnv1a64 %016llx\n", W, H, (unsigned long long)h);
    return 0;
}

int main()
{
    std::vector<uint8_t> vol((size_t)X * Y * Z);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                const int v = ((x * 5 + y * 3) ^ (z * 7)) & 255;
                vol[x + (size_t)X * (y + (size_t)Y * z)] = (uint8_t)(v > 200 ? v : v / 16);
            }
    void *dvol = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvol, (int64_t)vol.size())) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvol, vol.data(), (int64_t)vol.size(), nullptr)) != VR_OK) return fail("vr_upload", s);
    const int64_t dims[3] = {X, Y, Z};

    // the axial slice through voxel layer 13, one pixel per voxel
    const vrhip::Slicer axial(vrhip::axis_aligned_slice(dims, 2, 13), vrhip::default_projection(VR_PROJECT_MAX));
    if (show(axial, (const uint8_t *)dvol, dims)) return 1;

    // an oblique slab MIP of five layers through the centre; its corners stick out of the volume (background there)
    const double center[3] = {0.5, 0.5, 0.5}, right[3] = {1.0, 0.3, 0.2}, down[3] = {-0.2, 1.0, 0.4};
    vr_projection mip = vrhip::default_projection(VR_PROJECT_MAX);
    mip.background[2] = 0.25f;
    const vrhip::Slicer oblique(vrhip::slice_from_frame(center, right, down, 96, 64, 0.012, 5, 0.02), mip);
    if (show(oblique, (const uint8_t *)dvol, dims)) return 1;
    vr_free(dvol);
    return 0;
}
