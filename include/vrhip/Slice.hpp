// vrhip/Slice.hpp -- slice views (axial, coronal, sagittal and oblique planes, thick slabs) from C++: vr_slice_plane
// builders with the rules of volumerenderer_amd.render.SlicePlane, and Slicer, the frame and the sort-last partial
// (vr_reslice, vr_reslice_partial; the rule is in vrhip.h).  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include "Projection.hpp"
#include <cmath>
#include <stdexcept>

namespace vrhip {

// one GPU's plane: the whole cube is owned, the volume is the global one
inline vr_slice_plane blank_slice(int32_t width, int32_t height, int32_t layers, int32_t filter)
{
    if (width < 1 || height < 1 || layers < 1 || layers > (1 << 24)) throw std::invalid_argument("slice: width, height or layers");
    if (filter != VR_SLICE_NEAREST && filter != VR_SLICE_LINEAR) throw std::invalid_argument("slice: filter");
    vr_slice_plane p;
    p.width = width; p.height = height; p.layers = layers; p.filter = filter;
    for (int k = 0; k < 3; ++k) {
        p.origin[k] = p.du[k] = p.dv[k] = p.dw[k] = 0.0f;
        p.box_min[k] = 0.0f; p.box_max[k] = 1.0f;
        p.global_dims[k] = 0; p.vol_origin[k] = 0;
    }
    return p;
}

// SlicePlane.axis_aligned with one pixel per voxel: the slice through voxel layer `index` along `axis`, pixel centres
// on voxel centres; axial (axis 2) shows x across and y down, coronal (1) x and z, sagittal (0) y and z
inline vr_slice_plane axis_aligned_slice(const int64_t dims[3], int axis, int64_t index, int32_t layers = 1,
                                         int32_t filter = VR_SLICE_LINEAR)
{
    if (axis < 0 || axis > 2 || dims[0] < 1 || dims[1] < 1 || dims[2] < 1 || index < 0 || index >= dims[axis])
        throw std::invalid_argument("axis_aligned_slice: axis, index or extents");
    const int cu = axis == 0 ? 1 : 0, cv = axis == 2 ? 1 : 2;
    vr_slice_plane p = blank_slice((int32_t)dims[cu], (int32_t)dims[cv], layers, filter);
    p.du[cu] = (float)(1.0 / (double)p.width);
    p.dv[cv] = (float)(1.0 / (double)p.height);
    p.dw[axis] = (float)(1.0 / (double)dims[axis]);
    p.origin[cu] = (float)(0.5 / (double)p.width);
    p.origin[cv] = (float)(0.5 / (double)p.height);
    p.origin[axis] = (float)(((double)index + 0.5) / (double)dims[axis]);
    return p;
}

// SlicePlane.from_frame: centred on `center`, columns along `right`, rows along `down` (texture-space directions,
// normalised here), `pitch` apart; layers along right x down, `layer_pitch` (0: pitch) apart, centred on `center` too
inline vr_slice_plane slice_from_frame(const double center[3], const double right[3], const double down[3], int32_t width,
                                       int32_t height, double pitch, int32_t layers = 1, double layer_pitch = 0.0,
                                       int32_t filter = VR_SLICE_LINEAR)
{
    vr_slice_plane p = blank_slice(width, height, layers, filter);
    auto unit = [](const double v[3], double o[3]) {
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        if (!(l > 0.0)) throw std::invalid_argument("slice_from_frame: right and down must span a plane");
        o[0] = v[0] / l; o[1] = v[1] / l; o[2] = v[2] / l;
    };
    double r[3], d[3], n[3];
    unit(right, r); unit(down, d);
    const double c[3] = {r[1] * d[2] - r[2] * d[1], r[2] * d[0] - r[0] * d[2], r[0] * d[1] - r[1] * d[0]};
    unit(c, n);
    if (!(pitch > 0.0) || !std::isfinite(pitch) || !std::isfinite(layer_pitch)) throw std::invalid_argument("slice_from_frame: pitch");
    const double lp = layer_pitch != 0.0 ? layer_pitch : pitch;
    const double hw = 0.5 * (width - 1), hh = 0.5 * (height - 1), hl = 0.5 * (layers - 1);
    for (int k = 0; k < 3; ++k) {
        const double du = r[k] * pitch, dv = d[k] * pitch, dw = n[k] * lp;
        p.du[k] = (float)du; p.dv[k] = (float)dv; p.dw[k] = (float)dw;
        p.origin[k] = (float)(center[k] - hw * du - hh * dv - hl * dw);
    }
    return p;
}

// What is the same for every call (plane, projection) is set once.  Buffers are the caller's device memory: a partial
// and a frame are plane.width * plane.height float4 each.  A rank's slab sets the plane's box, vol_origin and
// global_dims and holds one halo layer; its partials combine through Projector's combine calls.
class Slicer {
public:
    vr_slice_plane plane;
    vr_projection proj;

    Slicer(const vr_slice_plane &pl, const vr_projection &p) : plane(pl), proj(p) {}

    vr_status frame(const uint8_t *vol_dev, const int64_t dims[3], float *rgba_dev, void *stream = nullptr) const
    {
        return vr_reslice(vol_dev, dims, &plane, &proj, rgba_dev, stream);
    }
    vr_status partial(const uint8_t *vol_dev, const int64_t dims[3], float *partial_dev, void *stream = nullptr) const
    {
        return vr_reslice_partial(vol_dev, dims, &plane, &proj, partial_dev, stream);
    }
    // the finish of a combined partial (vr_composite_finish_proj)
    vr_status finish(const float *partial_dev, float *rgba_dev, void *stream = nullptr) const
    {
        return vr_composite_finish_proj(partial_dev, &proj, rgba_dev, (int64_t)plane.width * plane.height, stream);
    }
};

} // namespace vrhip
