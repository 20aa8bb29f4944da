// projection.cpp -- a maximum intensity projection (MIP) of a synthetic volume from C++, through the C ABI
// (vrhip::Projector over vr_raycast_projection), and the FNV-1a-64 hash of the frame's bytes.  Plain C++ (g++), no HIP
// headers.  tests/test_projection_cpu.py builds it; tests/test_gpu_projection.py compares the hash with the Python
// frame's.
//
//   g++ -std=c++14 -O2 -Iinclude examples/projection.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/projection
//   /tmp/projection            prints "mip 96 x 64 fnv1a64 <16 hex digits>"
#include "vrhip/Projection.hpp"
#include <cstdio>
#include <cstring>
#include <vector>

static const int X = 48, Y = 40, Z = 32, W = 96, H = 64;

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

int main()
{
    // a bright, sparse structure in a dark field: what a MIP is for
    std::vector<uint8_t> vol((size_t)X * Y * Z);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                const int v = ((x * 5 + y * 3) ^ (z * 7)) & 255;
                vol[x + (size_t)X * (y + (size_t)Y * z)] = (uint8_t)(v > 200 ? v : v / 16);
            }
    void *dvol = nullptr, *dimg = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvol, (int64_t)vol.size())) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dimg, (int64_t)W * H * 4 * sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvol, vol.data(), (int64_t)vol.size(), nullptr)) != VR_OK) return fail("vr_upload", s);

    vr_camera cam;
    cam.pos[0] = 0.15f; cam.pos[1] = -0.1f; cam.pos[2] = -0.8f;
    cam.front[0] = 0.0f; cam.front[1] = 0.0f; cam.front[2] = 1.0f;
    cam.up[0] = 0.0f; cam.up[1] = 1.0f; cam.up[2] = 0.0f;
    cam.fov_deg = 40.0f; cam.z_near = 0.1f; cam.z_far = 100.0f;
    vr_render_params P;
    std::memset(&P, 0, sizeof(P));
    P.width = W; P.height = H;
    P.step_size[0] = (float)(1.0 / X); P.step_size[1] = (float)(1.0 / Y); P.step_size[2] = (float)(1.0 / Z);
    P.max_samples = 300;
    P.box_max[0] = P.box_max[1] = P.box_max[2] = 1.0f;
    const int64_t dims[3] = {X, Y, Z};
    const vrhip::Projector mip(cam, vrhip::default_projection(VR_PROJECT_MAX));
    if ((s = mip.frame((const uint8_t *)dvol, dims, P, (float *)dimg)) != VR_OK) return fail("vr_raycast_projection", s);
    std::vector<float> img((size_t)W * H * 4);
    if ((s = vr_download(img.data(), dimg, (int64_t)img.size() * (int64_t)sizeof(float), nullptr)) != VR_OK) return fail("vr_download", s);
    vr_free(dimg); vr_free(dvol);
    uint64_t h = 14695981039346656037ull;           // FNV-1a, 64 bits, over the frame's bytes
    const unsigned char *b = (const unsigned char *)img.data();
    for (size_t i = 0; i < img.size() * sizeof(float); ++i) { h ^= b[i]; h *= 1099511628211ull; }
    std::printf("mip %d x %d fnv1a64 %016llx\n", W, H, (unsigned long long)h);
    return 0;
}
