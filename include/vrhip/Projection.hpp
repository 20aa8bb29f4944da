// vrhip/Projection.hpp -- intensity projections (MIP, MinIP, the mean along the ray) from C++: a vr_projection with the
// defaults of volumerenderer_amd.render.Projection, and Projector, the frame, the sort-last partial and its combine calls
// (vr_raycast_projection & co.; the rule is in vrhip.h).  Plain C++14, host only.
#pragma once
#include "../vrhip.h"
#include <stdexcept>

namespace vrhip {

// a grey projection: identity window (0, 1), black background, no colour map
inline vr_projection default_projection(int32_t op = VR_PROJECT_MAX)
{
    if (op < VR_PROJECT_MAX || op > VR_PROJECT_MEAN) throw std::invalid_argument("default_projection: op");
    vr_projection p;
    p.lut_dev = nullptr;
    p.op = op;
    p.window_lo = 0.0f; p.window_hi = 1.0f;
    p.background[0] = p.background[1] = p.background[2] = 0.0f;
    return p;
}

// What is the same for every slab of a frame (camera, projection) is set once, the calls take what differs.  Buffers are
// the caller's device memory: a projection partial and a frame are width * height float4 each.  A slab holds one halo
// layer (SortLastTf::slab of an unlit SortLastTf lays it out).
class Projector {
public:
    vr_camera cam;
    vr_projection proj;

    Projector(const vr_camera &c, const vr_projection &p) : cam(c), proj(p) {}

    // the frame, or the partial, of a dense volume or a pool; P.mode is set to what the call needs
    vr_status frame(const uint8_t *vol_dev, const int64_t dims[3], vr_render_params P, float *rgba_dev, void *stream = nullptr) const
    {
        P.mode = VR_RENDER_PROJECTION;
        return vr_raycast_projection(vol_dev, dims, &cam, &P, &proj, rgba_dev, stream);
    }
    vr_status framePool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                        const int64_t grid[3], vr_render_params P, float *rgba_dev, void *stream = nullptr) const
    {
        P.mode = VR_RENDER_PROJECTION;
        return vr_raycast_pool_projection(pool_dev, table_dev, brick_dims, grid, &cam, &P, &proj, rgba_dev, stream);
    }
    vr_status partial(const uint8_t *vol_dev, const int64_t dims[3], vr_render_params P, float *partial_dev,
                      void *stream = nullptr) const
    {
        P.mode = VR_RENDER_PROJECTION;
        return vr_raycast_projection_partial(vol_dev, dims, &cam, &P, &proj, partial_dev, stream);
    }
    vr_status partialPool(const uint8_t *pool_dev, const vr_pool_entry *table_dev, const int64_t brick_dims[3],
                          const int64_t grid[3], vr_render_params P, float *partial_dev, void *stream = nullptr) const
    {
        P.mode = VR_RENDER_PROJECTION;
        return vr_raycast_pool_projection_partial(pool_dev, table_dev, brick_dims, grid, &cam, &P, &proj, partial_dev, stream);
    }
    // front = combine(front, back); the finish; num_slabs stacked partials combined and finished
    vr_status combine(float *front_dev, const float *back_dev, int64_t num_pixels, void *stream = nullptr) const
    {
        return vr_composite_combine_proj(front_dev, back_dev, num_pixels, proj.op, stream);
    }
    vr_status finish(const float *partial_dev, float *rgba_dev, int64_t num_pixels, void *stream = nullptr) const
    {
        return vr_composite_finish_proj(partial_dev, &proj, rgba_dev, num_pixels, stream);
    }
    vr_status combineSlabs(const float *partials_dev, int num_slabs, int64_t num_pixels, float *rgba_dev,
                           void *stream = nullptr) const
    {
        return vr_composite_slabs_proj(partials_dev, num_slabs, num_pixels, &proj, rgba_dev, stream);
    }
    // across ranks: the exchange of a vr_compositor handle, the tile combined by combineSlabs' kernel
    vr_status composite(vr_compositor *c, const float *partial_dev, float *rgba_dev, void *stream = nullptr) const
    {
        return vr_compositor_composite_proj(c, partial_dev, &proj, rgba_dev, stream);
    }
};

} // namespace vrhip
