// raymarch.h -- what raymarch.hip offers the other units of the library (capi.hip, compositor.hip): the launchers of its
// kernels, the frame's view basis and the kind of a partial image.  Every launcher returns launch_status(): 0, or 1
// where the launch failed.
#pragma once
#include "../../include/vrhip.h"
#include <hip/hip_runtime.h>
#include <atomic>

namespace vr {

// The basis every ray of a frame is formed from, dir = f + nx tanX s + ny tanY u: glm::lookAt's axes and
// glm::perspectiveFov's half-angle tangents (main.cpp:396-397) in float.  The marchers, the slab order of the
// compositing kernels and vr_lod_select's culling agree because all of them take it from here.
struct ViewBasis { float f[3], s[3], u[3], tanX, tanY; };
ViewBasis view_basis(const vr_camera *cam, int width, int height);

// A partial image is one float4 per pixel of one of three kinds (the rules are in vrhip.h): grey (c, tau, covered, 0),
// colour (C.r, C.g, C.b, T) or projection (v, n, 0, 0).  A kind folds two partials and finishes one into a frame; tf
// (colour: its background) and proj (projection: op folds; window, table and background finish) are what that takes.
// A fold of colour partials needs no tf.
struct PartialKind {
    enum Which { GREY, COLOUR, PROJECTION } which;
    const vr_transfer_function *tf;
    const vr_projection *proj;
};

// front = fold(front, back) and rgba = finish(partial) over n pixels
int composite_over_launch(const PartialKind &, float *front, const float *back, int64_t n, hipStream_t);
int composite_finish_launch(const PartialKind &, const float *partial, float *rgba, int64_t n, hipStream_t);
// rgba = finish(fold of nslabs partials of npix pixels each); grey and colour fold in each pixel's view order along axis
// (pixel i is pixel first + i of cam's P->width x P->height frame), projection in ascending order: it reads neither
int composite_slabs_launch(const PartialKind &, const float *partials, int nslabs, int64_t npix, int64_t first, int axis,
                           const vr_camera *cam, const vr_render_params *P, float *rgba, hipStream_t);

int raycast_launch(const uint8_t *vol, const int64_t dims[3], const vr_camera *, const vr_render_params *,
                   const vr_transfer_function *, const vr_shading *, bool partial, float *rgba, hipStream_t);
int raycast_pool_launch(const uint8_t *pool, const vr_pool_entry *, const int64_t bd[3], const int64_t grid[3], const vr_camera *,
                        const vr_render_params *, const vr_transfer_function *, const vr_shading *, bool partial, float *rgba,
                        hipStream_t);
int raycast_tf2d_launch(const uint8_t *vol, const int64_t dims[3], const vr_camera *, const vr_render_params *,
                        const vr_transfer_function2d *, const vr_shading *, bool partial, float *rgba, hipStream_t);
int raycast_pool_tf2d_launch(const uint8_t *pool, const vr_pool_entry *, const int64_t bd[3], const int64_t grid[3],
                             const vr_camera *, const vr_render_params *, const vr_transfer_function2d *, const vr_shading *,
                             bool partial, float *rgba, hipStream_t);
int tf2d_columns_launch(const float *lut, int rows, uint16_t *columns, hipStream_t);
int raycast_proj_launch(const uint8_t *vol, const int64_t dims[3], const vr_camera *, const vr_render_params *, const vr_projection *,
                        bool partial, float *rgba, hipStream_t);
int raycast_pool_proj_launch(const uint8_t *pool, const vr_pool_entry *, const int64_t bd[3], const int64_t grid[3],
                             const vr_camera *, const vr_render_params *, const vr_projection *, bool partial, float *rgba,
                             hipStream_t);
int reslice_launch(const uint8_t *vol, const int64_t dims[3], const vr_slice_plane *, const vr_projection *, bool partial,
                   float *out, hipStream_t);
int skip_grid_launch(const uint8_t *vol, const int64_t dims[3], int cell, uint8_t *grid, hipStream_t);
int skip_grid_pool_launch(const uint8_t *pool, const vr_pool_entry *, const int64_t bd[3], const int64_t grid[3], int cell,
                          uint8_t *out, hipStream_t);
int assemble_launch(bool toVolume, const uint8_t *src, uint8_t *dst, int nbricks, const int64_t bd[3], const int64_t *ijkDev,
                    const int64_t grid[3], hipStream_t);
int measure_error_launch(const uint8_t *a, const uint8_t *b, int64_t n, int *maxErrDev, unsigned long long *sumDev, hipStream_t);
int query_error_launch(const uint8_t *a, const uint8_t *b, int64_t n, uint8_t *out, hipStream_t);

// a vr_projection the kernels may take (vrhip.h); defined in capi.hip
bool projection_ok(const vr_projection *);

// process-wide debugging switches (vr_debug_set), defined beside the launchers that read them
extern std::atomic<int> g_skipGridV1;
extern std::atomic<int> g_resliceTileLog2;
extern std::atomic<int> g_histPlain;          // histogram.hip: the kernels without their data-aware paths
extern std::atomic<int> g_meshCountOnly;      // isomesh.hip: vr_isomesh_count without its scans (for measurements)

} // namespace vr
