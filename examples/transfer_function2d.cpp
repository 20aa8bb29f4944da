// transfer_function2d.cpp -- boundary emphasis with a two-dimensional transfer function from C++: a volume of two
// materials (a dense core inside a softer ball), a 1-D table that colours them by value, and row weights that make the
// interiors (gradient 0) clear and the material boundaries (large gradients) opaque: vrhip::transfer_function2d_separable,
// vr_tf2d_columns_build and one lit frame of vrhip::HeadlessViewer::draw (vr_raycast_tf2d).  Plain C++ (g++), no HIP
// headers: everything GPU goes through the C ABI.  tests/test_transfer_function2d_cpu.py compares the table and
// tests/test_gpu_transfer_function2d.py the frame with the Python surface.
//
//   g++ -std=c++14 -O2 -Iinclude examples/transfer_function2d.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/transfer_function2d
//   /tmp/transfer_function2d table               prints the 111 x 256 table, one entry per line (hex floats)
//   /tmp/transfer_function2d render PPM [F32]    writes the 96 x 64 frame as a PPM (and as float32 RGBA to F32)
#include "vrhip/Viewer.hpp"
#include <cstdio>
#include <cstring>

static const int X = 48, Y = 40, Z = 36, W = 96, H = 64, ROWS = VR_HIST_GRAD_BINS;

static std::vector<float> table()
{
    // blue-grey for the ball (value 90), warm white for the core (value 200), some opacity from value 30 on
    const std::vector<vrhip::TfPoint> pts = {{0, 0.0, 0.0, 0.0, 0.0}, {30, 0.2, 0.3, 0.6, 0.0}, {90, 0.3, 0.5, 0.9, 0.5},
                                             {200, 1.0, 0.9, 0.7, 0.9}, {255, 1.0, 1.0, 1.0, 0.9}};
    std::vector<double> w(ROWS);
    for (int j = 0; j < ROWS; ++j) w[j] = j < 8 ? j / 8.0 : 1.0;       // clear where the gradient vanishes
    return vrhip::transfer_function2d_separable(vrhip::transfer_function_from_points(pts), w);
}

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

int main(int argc, char **argv)
{
    const std::vector<float> lut = table();
    if (argc == 2 && !std::strcmp(argv[1], "table")) {
        for (int e = 0; e < ROWS * 256; ++e)
            std::printf("%d %a %a %a %a\n", e, lut[4 * e], lut[4 * e + 1], lut[4 * e + 2], lut[4 * e + 3]);
        return 0;
    }
    if (argc < 3 || std::strcmp(argv[1], "render")) {
        std::fprintf(stderr, "usage: %s table | render PPM [F32]\n", argv[0]);
        return 2;
    }
    std::vector<uint8_t> vol((size_t)X * Y * Z);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                // squared distance from the centre in half voxels (integers): core within 9 voxels, ball within 16
                const int dx = 2 * x + 1 - X, dy = 2 * y + 1 - Y, dz = 2 * z + 1 - Z, d2 = dx * dx + dy * dy + dz * dz;
                vol[x + (size_t)X * (y + (size_t)Y * z)] = d2 < 18 * 18 ? 200 : (d2 < 32 * 32 ? 90 : 0);
            }
    const int64_t lutBytes = (int64_t)lut.size() * (int64_t)sizeof(float);
    void *dvol = nullptr, *dlut = nullptr, *dcol = nullptr, *dimg = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvol, (int64_t)vol.size())) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dlut, lutBytes)) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dcol, 256 * sizeof(uint16_t))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dimg, (int64_t)W * H * 4 * sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvol, vol.data(), (int64_t)vol.size(), nullptr)) != VR_OK) return fail("vr_upload", s);
    if ((s = vr_upload(dlut, lut.data(), lutBytes, nullptr)) != VR_OK) return fail("vr_upload", s);
    if ((s = vr_tf2d_columns_build((const float *)dlut, ROWS, (uint16_t *)dcol, nullptr)) != VR_OK) return fail("vr_tf2d_columns_build", s);

    vrhip::HeadlessViewer v(W, H);
    v.cameraPos[0] = 0.2f; v.cameraPos[1] = -0.15f; v.cameraPos[2] = -0.85f;
    v.fov = 40.0f;
    const int64_t dims[3] = {X, Y, Z};
    vr_render_params P;
    std::memset(&P, 0, sizeof(P));
    P.step_size[0] = (float)(1.0 / X); P.step_size[1] = (float)(1.0 / Y); P.step_size[2] = (float)(1.0 / Z);
    P.max_samples = 300;
    P.mode = VR_RENDER_SHADED;
    P.box_max[0] = P.box_max[1] = P.box_max[2] = 1.0f;
    vr_transfer_function2d tf;
    tf.lut_dev = (const float *)dlut;
    tf.columns_dev = (const uint16_t *)dcol;
    tf.rows = ROWS;
    tf.grad_scale = vrhip::default_grad_scale(ROWS);
    tf.opacity_unit = 1.0f / 64.0f;
    tf.background[0] = 0.05f; tf.background[1] = 0.05f; tf.background[2] = 0.1f;
    vr_shading sh = vrhip::default_shading();
    sh.light_dir[0] = 0.5f; sh.light_dir[1] = 1.0f; sh.light_dir[2] = -0.5f;
    if ((s = v.draw((const uint8_t *)dvol, dims, P, &tf, &sh, (float *)dimg)) != VR_OK) return fail("draw", s);
    std::vector<float> img((size_t)W * H * 4);
    if ((s = vr_download(img.data(), dimg, (int64_t)img.size() * (int64_t)sizeof(float), nullptr)) != VR_OK) return fail("vr_download", s);
    if (!vrhip::HeadlessViewer::dumpPPM(argv[2], img, W, H)) {
        std::fprintf(stderr, "cannot write %s\n", argv[2]);
        return 1;
    }
    if (argc > 3) {
        FILE *f = std::fopen(argv[3], "wb");
        if (!f || std::fwrite(img.data(), sizeof(float), img.size(), f) != img.size() || std::fclose(f) != 0) {
            std::fprintf(stderr, "cannot write %s\n", argv[3]);
            return 1;
        }
    }
    vr_free(dimg); vr_free(dcol); vr_free(dlut); vr_free(dvol);
    std::printf("frame %d x %d written\n", W, H);
    return 0;
}
