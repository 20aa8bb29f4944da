"""volumerenderer_amd -- MI355X-native kd-tree volume codec + ray-march compositor.

The product is volumerenderer_amd/libvrhip.so (hand-written HIP for gfx950 behind the
C ABI of include/vrhip.h).  This package is the Python host-side mirror of the
reference's class interface, used by the parity tests and the bench."""
from ._lib import (RENDER_COMPOSITE, RENDER_ISOSURFACE, RENDER_PARTIAL, VARIANT_GUARDED, VARIANT_MIDRANGE,
                   VARIANT_RECOVER, Camera, RenderParams, VrError)

__all__ = ["BrickSet", "VolumeKdtree", "MidRangeTree", "HashedKdtree", "VolumeReader", "UnitBrick", "VrError", "Camera",
           "RenderParams"]


def __getattr__(name):  # torch is imported lazily so that `import volumerenderer_amd` stays cheap
    if name in ("BrickSet", "VolumeKdtree", "MidRangeTree", "HashedKdtree", "measure_error", "query_error",
                "measure_error_bricks", "BRICK_ERROR", "stream_block_table"):
        from . import codec
        return getattr(codec, name)
    if name in ("VolumeReader", "UnitBrick", "raycast", "default_camera", "default_params", "composite_over",
                "composite_finish", "assemble_bricks", "disassemble_bricks", "fill_volume_brick_map", "build_skip_grid",
                "use_skip_grid", "select_lod", "lod_pool_layout", "raycast_pool", "build_skip_grid_pool", "TransferFunction",
                "raycast_tf", "raycast_pool_tf", "transfer_function_table", "Shading", "raycast_tf_shaded",
                "raycast_pool_tf_shaded", "raycast_tf_partial", "raycast_pool_tf_partial", "composite_over_tf",
                "composite_finish_tf", "Projection", "raycast_projection", "raycast_pool_projection",
                "raycast_projection_partial", "raycast_pool_projection_partial", "composite_combine_proj",
                "composite_finish_proj", "SlicePlane", "reslice", "reslice_partial", "select_lod_error", "rate_distortion",
                "histogram_bricks", "histogram", "histogram_pool", "histogram2d", "window_from_histogram",
                "projection_from_histogram", "TransferFunction2D", "tf2d_separable_table", "raycast_tf2d",
                "raycast_pool_tf2d", "raycast_tf2d_partial", "raycast_pool_tf2d_partial", "IsoMesh", "isosurface_mesh",
                "write_ply", "read_ply"):
        from . import render
        return getattr(render, name)
    raise AttributeError(name)
