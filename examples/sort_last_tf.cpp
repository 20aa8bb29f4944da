// sort_last_tf.cpp -- a transfer-function frame drawn as two slabs on one GPU: each slab's colour partial
// (vrhip::SortLastTf::partial = vr_raycast_tf_partial), the two combined per pixel in view order (combineSlabs =
// vr_composite_slabs_tf) and compared with the single pass (vr_raycast_tf / vr_raycast_tf_shaded without early exit).
// On several GPUs each rank would draw one slab and call SortLastTf::composite with its vr_compositor.  Plain C++
// (g++), no HIP headers.  tests/test_gpu_sort_last_tf.py runs it.
//
//   g++ -std=c++14 -O2 -Iinclude examples/sort_last_tf.cpp -Lvolumerenderer_amd -lvrhip
//       -Wl,-rpath,$PWD/volumerenderer_amd -o /tmp/sort_last_tf
//   /tmp/sort_last_tf [lit]        prints the largest difference between the two-slab frame and the single pass
#include "vrhip/TransferFunction.hpp"
#include <cmath>
#include <cstdio>
#include <cstring>

static const int X = 48, Y = 40, Z = 36, W = 96, H = 64;

static int fail(const char *what, vr_status s)
{
    std::fprintf(stderr, "%s: %s\n", what, vr_status_string(s));
    return 1;
}

int main(int argc, char **argv)
{
    const bool lit = argc > 1 && !std::strcmp(argv[1], "lit");
    int32_t ndev = 0;
    if (vr_device_count(&ndev) != VR_OK || ndev <= 0) {
        std::fprintf(stderr, "no usable HIP device\n");
        return 1;
    }
    const std::vector<float> lut = vrhip::transfer_function_from_points(
        {{0, 0.1, 0.3, 0.9, 0.0}, {30, 0.1, 0.3, 0.9, 0.0}, {110, 0.2, 0.5, 0.9, 0.3}, {150, 0.9, 0.5, 0.1, 0.0}, {255, 1.0, 0.9, 0.2, 0.9}});
    std::vector<uint8_t> vol((size_t)X * Y * Z);
    for (int z = 0; z < Z; ++z)
        for (int y = 0; y < Y; ++y)
            for (int x = 0; x < X; ++x) {
                const double dx = (x + 0.5) / X - 0.45, dy = (y + 0.5) / Y - 0.55, dz = (z + 0.5) / Z - 0.5;
                const double v = 230.0 * std::exp(-(dx * dx + dy * dy + dz * dz) / 0.05) + 20.0 * (((x / 4 + y / 4 + z / 4) & 1));
                vol[x + (size_t)X * (y + (size_t)Y * z)] = (uint8_t)(v > 255.0 ? 255.0 : v);
            }
    const int64_t dims[3] = {X, Y, Z}, npix = (int64_t)W * H;
    void *dvol = nullptr, *dlut = nullptr, *dparts = nullptr, *dtwo = nullptr, *dsingle = nullptr, *dslab = nullptr;
    vr_status s;
    if ((s = vr_malloc(&dvol, (int64_t)vol.size())) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dslab, (int64_t)vol.size())) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dlut, 256 * 4 * sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dparts, 2 * npix * 4 * (int64_t)sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dtwo, npix * 4 * (int64_t)sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_malloc(&dsingle, npix * 4 * (int64_t)sizeof(float))) != VR_OK) return fail("vr_malloc", s);
    if ((s = vr_upload(dvol, vol.data(), (int64_t)vol.size(), nullptr)) != VR_OK) return fail("vr_upload", s);
    if ((s = vr_upload(dlut, lut.data(), 256 * 4 * sizeof(float), nullptr)) != VR_OK) return fail("vr_upload", s);

    vr_camera cam;
    const float pos[3] = {0.3f, 0.2f, -1.1f}, front[3] = {-0.25f, -0.15f, 1.0f}, up[3] = {0.0f, 1.0f, 0.0f};
    for (int k = 0; k < 3; ++k) { cam.pos[k] = pos[k]; cam.front[k] = front[k]; cam.up[k] = up[k]; }
    cam.fov_deg = 50.0f; cam.z_near = 0.1f; cam.z_far = 100.0f;
    vr_transfer_function tf;
    tf.lut_dev = (const float *)dlut;
    tf.opacity_unit = 1.0f / 64.0f;
    tf.background[0] = 0.2f; tf.background[1] = 0.2f; tf.background[2] = 0.25f;
    vr_render_params P;
    std::memset(&P, 0, sizeof(P));
    P.width = W; P.height = H;
    P.step_size[0] = (float)(0.5 / X); P.step_size[1] = (float)(0.5 / Y); P.step_size[2] = (float)(0.5 / Z);
    P.max_samples = 300;
    P.box_max[0] = P.box_max[1] = P.box_max[2] = 1.0f;
    P.no_early_exit = 1;        // across slabs the early exit is per slab: compare without it

    const vrhip::SortLastTf sl = lit ? vrhip::SortLastTf(cam, tf, vrhip::default_shading()) : vrhip::SortLastTf(cam, tf);
    const int axis = 2, world = 2;
    for (int r = 0; r < world; ++r) {
        int64_t local[3], range[2];
        const vr_render_params Pr = sl.slab(P, dims, axis, r, world, local, range);
        // z slabs are contiguous in memory: the slab's voxels are planes range[0] .. range[1]
        const size_t plane = (size_t)X * Y;
        if ((s = vr_upload(dslab, vol.data() + plane * (size_t)range[0], (int64_t)(plane * (size_t)(range[1] - range[0])), nullptr)) != VR_OK)
            return fail("vr_upload", s);
        if ((s = sl.partial((const uint8_t *)dslab, local, Pr, (float *)dparts + (size_t)r * npix * 4)) != VR_OK) return fail("partial", s);
    }
    if ((s = sl.combineSlabs((const float *)dparts, world, npix, 0, axis, P, (float *)dtwo)) != VR_OK) return fail("combineSlabs", s);
    P.mode = lit ? VR_RENDER_SHADED : VR_RENDER_COMPOSITE;
    s = lit ? vr_raycast_tf_shaded((const uint8_t *)dvol, dims, &cam, &P, &tf, &sl.shading, (float *)dsingle, nullptr)
            : vr_raycast_tf((const uint8_t *)dvol, dims, &cam, &P, &tf, (float *)dsingle, nullptr);
    if (s != VR_OK) return fail("vr_raycast_tf", s);
    std::vector<float> two((size_t)npix * 4), single((size_t)npix * 4);
    if ((s = vr_download(two.data(), dtwo, npix * 4 * (int64_t)sizeof(float), nullptr)) != VR_OK) return fail("vr_download", s);
    if ((s = vr_download(single.data(), dsingle, npix * 4 * (int64_t)sizeof(float), nullptr)) != VR_OK) return fail("vr_download", s);
    double worst = 0.0, seen = 0.0;
    for (size_t i = 0; i < two.size(); ++i) {
        worst = std::fmax(worst, std::fabs((double)two[i] - (double)single[i]));
        if (i % 4 == 3) seen = std::fmax(seen, (double)single[i]);
    }
    vr_free(dsingle); vr_free(dtwo); vr_free(dparts); vr_free(dlut); vr_free(dslab); vr_free(dvol);
    std::printf("two slabs against the single pass (%s): max difference %.3e, max alpha %.3f\n", lit ? "lit" : "unlit", worst, seen);
    return worst <= 2e-3 && seen > 0.5 ? 0 : 1;
}
