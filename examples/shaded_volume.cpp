// shaded_volume.cpp -- a gradient-lit frame through a user transfer function from C++: the table from control points
// (vrhip::transfer_function_from_points), the default lighting (vrhip::default_shading) with a fixed light, and one
// frame of vrhip::HeadlessViewer::draw with both (vr_raycast_tf_shaded).  Plain C++ (g++), no HIP headers: everything
// GPU goes through the C ABI.  tests/test_gpu_shading.py compares the frame with the Python surface.
//
//   g++ -std=c++14 -O2 -Iinclude examples/shaded_volume.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/shaded_volume
//   /tmp/shaded_volume render FILE      writes the 96 x 64 float32 RGBA frame to FILE
#include "vrhip/Viewer.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>

static const int X = 48, Y = 40, Z = 32, W = 96, H = 64;

static std::vector<vrhip::TfPoint> points()
{
    // clear below 60, a translucent orange shell, an opaque white core
    return {{0, 0.0, 0.0, 0.0, 0.0}, {60, 0.9, 0.5, 0.1, 0.0}, {120, 0.9, 0.6, 0.2, 0.3}, {200, 1.0, 1.0, 1.0, 0.9}};
}

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

int main(int argc, char **argv)
{
    const std::vector<float> lut = vrhip::transfer_function_from_points(points());
    if (argc < 3 || std::strcmp(argv[1], "render")) {
        std::fprintf(stderr, "usage: %s render FILE\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> vol((size_t)X * Y * Z);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                // a smooth blob: 230 at the centre, falling off with the squared distance
                const double dx = (x - 0.5 * X) / X, dy = (y - 0.5 * Y) / Y, dz = (z - 0.5 * Z) / Z;
                vol[x + (size_t)X * (y + (size_t)Y * z)] = (uint8_t)std::lround(230.0 * std::exp(-8.0 * (dx * dx + dy * dy + dz * dz)));
            }
    void *dvol = nullptr, *dlut = nullptr, *dimg = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvol, (int64_t)vol.size())) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dlut, 256 * 4 * sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dimg, (int64_t)W * H * 4 * sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvol, vol.data(), (int64_t)vol.size(), nullptr)) != VR_OK) return fail("vr_upload", s);
    if ((s = vr_upload(dlut, lut.data(), 256 * 4 * sizeof(float), nullptr)) != VR_OK) return fail("vr_upload", s);

    vrhip::HeadlessViewer v(W, H);
    v.cameraPos[0] = 0.15f; v.cameraPos[1] = -0.1f; v.cameraPos[2] = -0.8f;
    v.fov = 40.0f;
    const int64_t dims[3] = {X, Y, Z};
    vr_render_params P;
    std::memset(&P, 0, sizeof(P));
    P.step_size[0] = (float)(1.0 / X); P.step_size[1] = (float)(1.0 / Y); P.step_size[2] = (float)(1.0 / Z);
    P.max_samples = 300;
    P.mode = VR_RENDER_SHADED;
    P.box_max[0] = P.box_max[1] = P.box_max[2] = 1.0f;
    vr_transfer_function tf;
    tf.lut_dev = (const float *)dlut;
    tf.opacity_unit = 1.0f / 64.0f;
    tf.background[0] = 0.2f; tf.background[1] = 0.2f; tf.background[2] = 0.25f;
    vr_shading sh = vrhip::default_shading();
    sh.light_dir[0] = 0.5f; sh.light_dir[1] = 1.0f; sh.light_dir[2] = -0.5f;
    if ((s = v.draw((const uint8_t *)dvol, dims, P, &tf, &sh, (float *)dimg)) != VR_OK) return fail("draw", s);
    std::vector<float> img((size_t)W * H * 4);
    if ((s = vr_download(img.data(), dimg, (int64_t)img.size() * (int64_t)sizeof(float), nullptr)) != VR_OK) return fail("vr_download", s);
    FILE *f = std::fopen(argv[2], "wb");
    if (!f || std::fwrite(img.data(), sizeof(float), img.size(), f) != img.size() || std::fclose(f) != 0) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    vr_free(dimg); vr_free(dlut); vr_free(dvol);
    std::printf("frame %d x %d written\n", W, H);
    return 0;
}
