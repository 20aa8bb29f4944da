// vrhip/TransferFunction.hpp -- a transfer-function table for vr_raycast_tf / vr_raycast_pool_tf from control points,
// without Python: the rule of volumerenderer_amd.render.transfer_function_table; a separable two-dimensional table for
// vr_raycast_tf2d; and SortLastTf, the sort-last colour
// partials of such frames (vr_raycast_tf_partial and its combine calls).  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <cmath>
#include <stdexcept>
#include <string>
#include <vector>

namespace vrhip {

struct TfPoint { double value, r, g, b, a; };      // value in [0, 255], colours in [0, 1]

// 256 x (r, g, b, a) float32, entry k for the scalar k / 255.  The points are sorted by value (non-decreasing).  Entry
// k is linear between the last point at or below k and the point after it, the first point's colour below the first
// value and the last point's from the last value on; computed in double and rounded to float.  Throws
// std::invalid_argument for an empty list, unsorted values, a value outside [0, 255] or a colour outside [0, 1].
inline std::vector<float> transfer_function_from_points(const std::vector<TfPoint> &pts)
{
    if (pts.empty()) throw std::invalid_argument("transfer function: no control points");
    for (size_t i = 0; i < pts.size(); ++i) {
        const TfPoint &p = pts[i];
        const double c[5] = {p.value, p.r, p.g, p.b, p.a};
        for (double q : c)
            if (!std::isfinite(q)) throw std::invalid_argument("transfer function: point " + std::to_string(i) + " is not finite");
        if (!(p.value >= 0.0 && p.value <= 255.0)) throw std::invalid_argument("transfer function: point " + std::to_string(i) + ": value outside [0, 255]");
        for (int k = 1; k < 5; ++k)
            if (!(c[k] >= 0.0 && c[k] <= 1.0)) throw std::invalid_argument("transfer function: point " + std::to_string(i) + ": r, g, b, a outside [0, 1]");
        if (i && p.value < pts[i - 1].value) throw std::invalid_argument("transfer function: points are not sorted by value");
    }
    std::vector<float> lut(256 * 4);
    const int n = (int)pts.size();
    int j = -1;                                     // the last point at or below k
    for (int k = 0; k < 256; ++k) {
        while (j + 1 < n && pts[j + 1].value <= k) ++j;
        const TfPoint &p0 = pts[j < 0 ? 0 : j];
        const double c0[4] = {p0.r, p0.g, p0.b, p0.a};
        if (j < 0 || j + 1 == n) {
            for (int c = 0; c < 4; ++c) lut[4 * k + c] = (float)c0[c];
            continue;
        }
        const TfPoint &p1 = pts[j + 1];
        const double c1[4] = {p1.r, p1.g, p1.b, p1.a};
        const double t = (k - p0.value) / (p1.value - p0.value);
        for (int c = 0; c < 4; ++c) lut[4 * k + c] = (float)(c0[c] + t * (c1[c] - c0[c]));
    }
    return lut;
}

// rows x 256 x (r, g, b, a) float32 for vr_raycast_tf2d: row j holds the 1-D table's colours and its alpha scaled by
// weight_by_row[j] -- rgb[j][k] = lut1d[k].rgb, a[j][k] = (float)((double)lut1d[k].a * weight_by_row[j]); the rule of
// volumerenderer_amd.render.tf2d_separable_table.  Throws std::invalid_argument unless lut1d holds 256 x 4 floats, there
// are 2 .. VR_TF2D_MAX_ROWS weights and every weight lies in [0, 1].
inline std::vector<float> transfer_function2d_separable(const std::vector<float> &lut1d, const std::vector<double> &weight_by_row)
{
    if (lut1d.size() != 256 * 4) throw std::invalid_argument("transfer function 2d: the 1-D table must hold 256 x 4 floats");
    if (weight_by_row.size() < 2 || weight_by_row.size() > VR_TF2D_MAX_ROWS)
        throw std::invalid_argument("transfer function 2d: 2 .. " + std::to_string(VR_TF2D_MAX_ROWS) + " rows");
    for (double w : weight_by_row)
        if (!(w >= 0.0 && w <= 1.0)) throw std::invalid_argument("transfer function 2d: weights outside [0, 1]");
    std::vector<float> lut(weight_by_row.size() * 256 * 4);
    for (size_t j = 0; j < weight_by_row.size(); ++j)
        for (int k = 0; k < 256; ++k) {
            float *e = &lut[(j * 256 + k) * 4];
            e[0] = lut1d[4 * k]; e[1] = lut1d[4 * k + 1]; e[2] = lut1d[4 * k + 2];
            e[3] = (float)((double)lut1d[4 * k + 3] * weight_by_row[j]);
        }
    return lut;
}

// the row scale volumerenderer_amd.render.TransferFunction2D defaults to: the rows spread over the whole gradient range
inline float default_grad_scale(int rows) { return (float)(127.5 * (rows - 1) / 110.0); }

// the lighting volumerenderer_amd.render.Shading() defaults to: ka 0.3, kd 0.7, ks 0.2, shininess 32, head light,
// grad_min 1/255
inline vr_shading default_shading()
{
    vr_shading s;
    s.ambient = 0.3f; s.diffuse = 0.7f; s.specular = 0.2f; s.shininess = 32.0f;
    s.light_dir[0] = s.light_dir[1] = s.light_dir[2] = 0.0f;
    s.grad_min = (float)(1.0 / 255.0);
    return s;
}

// Sort-last frames through a transfer function, lit or not: what is the same for every slab of a frame (camera, table,
// lighting) is set once, the calls take what differs.  Buffers are the caller's device memory: a colour partial and a
// frame are width * height float4 each.  The rule is in vrhip.h (vr_raycast_tf_partial).  With a vr_transfer_function2d
// the partials come from vr_raycast_tf2d_partial (the mode is VR_RENDER_SHADED lit or not, two halo layers); the
// combine calls are the same: they read only the background.
class SortLastTf {
public:
    vr_camera cam;
    vr_transfer_function tf;        // two-dimensional: the background the combine calls read, no table
    bool lit;
    vr_shading shading;
    bool twoD;
    vr_transfer_function2d tf2d;

    SortLastTf(const vr_camera &c, const vr_transfer_function &t) : cam(c), tf(t), lit(false), shading(default_shading()), twoD(false), tf2d() {}
    SortLastTf(const vr_camera &c, const vr_transfer_function &t, const vr_shading &s) : cam(c), tf(t), lit(true), shading(s), twoD(false), tf2d() {}
    SortLastTf(const vr_camera &c, const vr_transfer_function2d &t) : cam(c), tf(background_of(t)), lit(false), shading(default_shading()), twoD(true), tf2d(t) {}
    SortLastTf(const vr_camera &c, const vr_transfer_function2d &t, const vr_shading &s) : cam(c), tf(background_of(t)), lit(true), shading(s), twoD(true), tf2d(t) {}

    static vr_transfer_function background_of(const vr_transfer_function2d &t)
    {
        vr_transfer_function b;
        b.lut_dev = nullptr; b.opacity_unit = t.opacity_unit;
        for (int k = 0; k < 3; ++k) b.background[k] = t.background[k];
        return b;
    }

    // halo layers a slab must hold beyond each cut: the trilinear taps, and the gradient's taps one voxel further (a
    // two-dimensional table takes the gradient of every sample, lit or not)
    int halo() const { return (lit || twoD) ? 2 : 1; }

    // Rank `rank`'s slab of a volume of `dims` voxels cut into `world` slabs along `axis` (volumerenderer_amd.distributed.
    // slab_params): P with box_min / box_max (the last rank's box_max is 2: it owns the far face), vol_origin and
    // global_dims set; local = the extents of the voxels [range[0], range[1]) along `axis` the rank holds.
    vr_render_params slab(vr_render_params P, const int64_t dims[3], int axis, int rank, int world, int64_t local[3],
                          int64_t range[2]) const
    {
        if (axis < 0 || axis > 2 || rank < 0 || rank >= world || world > dims[axis]) throw std::invalid_argument("SortLastTf::slab");
        const int64_t n = dims[axis], q = n / world, m = n % world;
        const int64_t lo = rank * q + (rank < m ? rank : m), hi = lo + q + (rank < m ? 1 : 0);
        range[0] = lo - halo() < 0 ? 0 : lo - halo();
        range[1] = hi + halo() > n ? n : hi + halo();
        for (int k = 0; k < 3; ++k) {
            P.box_min[k] = 0.0f; P.box_max[k] = 1.0f; P.vol_origin[k] = 0; P.global_dims[k] = dims[k]; local[k] = dims[k];
        }
        P.box_min[axis] = (float)((double)lo / (double)n);
        P.box_max[axis] = rank < world - 1 ? (float)((double)hi / (double)n) : 2.0f;
        P.vol_origin[axis] = range[0];
        local[axis] = range[1] - range[0];
        return P;
    }

    // the colour partial of a slab (or of the whole volume); P.mode is set to what the call needs
    vr_status partial(const uint8_t *vol_dev, const int64_t dims[3], vr_render_params P, float *partial_dev,
                      void *stream = nullptr) const
    {
        P.mode = (lit || twoD) ? VR_RENDER_SHADED : VR_RENDER_COMPOSITE;
        if (twoD) return vr_raycast_tf2d_partial(vol_dev, dims, &cam, &P, &tf2d, lit ? &shading : nullptr, partial_dev, stream);
        return vr_raycast_tf_partial(vol_dev, dims, &cam, &P, &tf, lit ? &shading : nullptr, partial_dev, stream);
    }
    vr_status partialPool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                          const int64_t grid[3], vr_render_params P, float *partial_dev, void *stream = nullptr) const
    {
        P.mode = (lit || twoD) ? VR_RENDER_SHADED : VR_RENDER_COMPOSITE;
        if (twoD)
            return vr_raycast_pool_tf2d_partial(pool_dev, table_dev, brick_dims, grid, &cam, &P, &tf2d, lit ? &shading : nullptr,
                                                partial_dev, stream);
        return vr_raycast_pool_tf_partial(pool_dev, table_dev, brick_dims, grid, &cam, &P, &tf, lit ? &shading : nullptr,
                                          partial_dev, stream);
    }
    // front = front OVER back; (C + T background, 1 - T); num_slabs partials of a tile combined per pixel in view order
    vr_status over(float *front_dev, const float *back_dev, int64_t num_pixels, void *stream = nullptr) const
    {
        return vr_composite_over_tf(front_dev, back_dev, num_pixels, stream);
    }
    vr_status finish(const float *partial_dev, float *rgba_dev, int64_t num_pixels, void *stream = nullptr) const
    {
        return vr_composite_finish_tf(partial_dev, &tf, rgba_dev, num_pixels, stream);
    }
    vr_status combineSlabs(const float *partials_dev, int num_slabs, int64_t num_pixels, int64_t first_pixel, int axis,
                           const vr_render_params &P, float *rgba_dev, void *stream = nullptr) const
    {
        return vr_composite_slabs_tf(partials_dev, num_slabs, num_pixels, first_pixel, axis, &cam, &P, &tf, rgba_dev, stream);
    }
    // across ranks: the exchange of a vr_compositor handle, the tile combined by combineSlabs' kernel
    vr_status composite(vr_compositor *c, const float *partial_dev, int axis, const vr_render_params &P, float *rgba_dev,
                        void *stream = nullptr) const
    {
        return vr_compositor_composite_tf(c, partial_dev, axis, &cam, &P, &tf, rgba_dev, stream);
    }
};

} // namespace vrhip
