"""ctypes binding of the C ABI in include/vrhip.h (libvrhip.so).

The library is the product: if it is missing this module raises -- there is no
Python / CPU fallback for any compute entry point."""
import ctypes as C
import os

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(HERE, "libvrhip.so")

VR_OK = 0
STATUS = {0: "VR_OK", -1: "VR_ERR_INVALID", -2: "VR_ERR_NO_DEVICE", -3: "VR_ERR_OOM", -4: "VR_ERR_IO",
          -5: "VR_ERR_STATE", -6: "VR_ERR_FORMAT", -7: "VR_ERR_UNSUPPORTED"}
VARIANT_RECOVER, VARIANT_GUARDED, VARIANT_MIDRANGE = 0, 1, 2
RENDER_COMPOSITE, RENDER_ISOSURFACE, RENDER_PARTIAL, RENDER_SHADED, RENDER_PROJECTION = 0, 1, 2, 3, 4
PROJECT_MAX, PROJECT_MIN, PROJECT_MEAN = 0, 1, 2
TF2D_MAX_ROWS, HIST_GRAD_BINS = 256, 111
SLICE_NEAREST, SLICE_LINEAR = 0, 1


class VrError(RuntimeError):
    def __init__(self, status, what=""):
        self.status = status
        super().__init__("%s: %s (%d)" % (what, STATUS.get(status, "?"), status))


class TreeInfo(C.Structure):
    _fields_ = [("X", C.c_int64), ("Y", C.c_int64), ("Z", C.c_int64),
                ("orig_tree_depth", C.c_int32), ("max_tree_depth", C.c_int32),
                ("num_active_nodes", C.c_int64), ("tree_bytes", C.c_int64),
                ("tolerance", C.c_int32), ("max_epochs", C.c_int32), ("variant", C.c_int32),
                ("num_reverts", C.c_int32), ("max_error_before", C.c_int32), ("max_error_after", C.c_int32),
                ("mean_l1_after", C.c_double), ("zero_run_rewrites", C.c_int32), ("est_exact_segments", C.c_int32)]


class Camera(C.Structure):
    _fields_ = [("pos", C.c_float * 3), ("front", C.c_float * 3), ("up", C.c_float * 3),
                ("fov_deg", C.c_float), ("z_near", C.c_float), ("z_far", C.c_float)]


class RenderParams(C.Structure):
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("step_size", C.c_float * 3),
                ("iso_value", C.c_float), ("max_samples", C.c_int32), ("mode", C.c_int32),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("global_dims", C.c_int64 * 3), ("vol_origin", C.c_int64 * 3),
                ("no_early_exit", C.c_int32), ("skip_cell", C.c_int32), ("skip_grid_dev", C.c_void_p)]


class TransferFunctionDesc(C.Structure):
    """vr_transfer_function (24 bytes)."""
    _fields_ = [("lut_dev", C.c_void_p), ("opacity_unit", C.c_float), ("background", C.c_float * 3)]


class TransferFunction2DDesc(C.Structure):
    """vr_transfer_function2d (40 bytes)."""
    _fields_ = [("lut_dev", C.c_void_p), ("columns_dev", C.c_void_p), ("rows", C.c_int32), ("grad_scale", C.c_float),
                ("opacity_unit", C.c_float), ("background", C.c_float * 3)]


class ShadingDesc(C.Structure):
    """vr_shading (32 bytes)."""
    _fields_ = [("ambient", C.c_float), ("diffuse", C.c_float), ("specular", C.c_float), ("shininess", C.c_float),
                ("light_dir", C.c_float * 3), ("grad_min", C.c_float)]


class Projection(C.Structure):
    """vr_projection (32 bytes)."""
    _fields_ = [("lut_dev", C.c_void_p), ("op", C.c_int32), ("window_lo", C.c_float), ("window_hi", C.c_float),
                ("background", C.c_float * 3)]


class SlicePlaneDesc(C.Structure):
    """vr_slice_plane (136 bytes)."""
    _fields_ = [("width", C.c_int32), ("height", C.c_int32), ("layers", C.c_int32), ("filter", C.c_int32),
                ("origin", C.c_float * 3), ("du", C.c_float * 3), ("dv", C.c_float * 3), ("dw", C.c_float * 3),
                ("box_min", C.c_float * 3), ("box_max", C.c_float * 3),
                ("global_dims", C.c_int64 * 3), ("vol_origin", C.c_int64 * 3)]


class TreeDesc(C.Structure):
    """vr_tree_desc (56 bytes): host pointers."""
    _fields_ = [("tree", C.c_void_p), ("tree_bytes", C.c_int64), ("num_active", C.c_int64), ("distance_map", C.c_void_p),
                ("map_len", C.c_int32), ("block_off", C.c_void_p), ("top_val", C.c_void_p)]


class PoolEntry(C.Structure):
    _fields_ = [("offset", C.c_int64), ("shift", C.c_uint8 * 3), ("pad", C.c_uint8 * 5)]


class BrickError(C.Structure):
    """vr_brick_error (24 bytes)."""
    _fields_ = [("sum_abs", C.c_uint64), ("sum_sq", C.c_uint64), ("max_abs", C.c_uint32), ("num_diff", C.c_uint32)]


class IsoMeshDesc(C.Structure):
    """vr_isomesh_desc (104 bytes)."""
    _fields_ = [("iso_value", C.c_float), ("cap", C.c_int32), ("global_dims", C.c_int64 * 3), ("vol_origin", C.c_int64 * 3),
                ("own_lo", C.c_int64 * 3), ("own_hi", C.c_int64 * 3)]


# every symbol include/vrhip.h declares, with its signature
_P, _I32, _I64 = C.c_void_p, C.c_int32, C.c_int64
SIGNATURES = {
    "vr_device_count": (_I32, [C.POINTER(_I32)]),
    "vr_set_device": (_I32, [_I32]),
    "vr_status_string": (C.c_char_p, [_I32]),
    "vr_version": (C.c_char_p, []),
    "vr_malloc": (_I32, [C.POINTER(_P), _I64]),
    "vr_free": (_I32, [_P]),
    "vr_upload": (_I32, [_P, _P, _I64, _P]),
    "vr_download": (_I32, [_P, _P, _I64, _P]),
    "vr_brickset_create": (_I32, [C.POINTER(_P), _I32, C.POINTER(_I64), _I32, _I32, _I32]),
    "vr_brickset_destroy": (_I32, [_P]),
    "vr_brickset_set_error_tolerance": (_I32, [_P, _I32]),
    "vr_brickset_set_max_epochs": (_I32, [_P, _I32]),
    "vr_brickset_build": (_I32, [_P, _P, _P]),
    "vr_brickset_info": (_I32, [_P, _I32, C.POINTER(TreeInfo)]),
    "vr_brickset_get_tree": (_I32, [_P, _I32, _P, _I64]),
    "vr_brickset_get_distance_map": (_I32, [_P, _I32, _P, _I32]),
    "vr_brickset_get_tree_range": (_I32, [_P, _I32, _P, _I64]),
    "vr_brickset_get_distance_map_range": (_I32, [_P, _I32, _P, _I32]),
    "vr_brickset_get_packed4": (_I32, [_P, _I32, _P, _I64, C.POINTER(_I64)]),
    "vr_brickset_decode": (_I32, [_P, _I32, _P, _P]),
    "vr_brickset_decode_range": (_I32, [_P, _I32, _P, _P]),
    "vr_brickset_decode_lod": (_I32, [_P, C.POINTER(_I32), _P, _P]),
    "vr_lod_select": (_I32, [C.POINTER(Camera), C.POINTER(RenderParams), _I32, C.POINTER(_I64), C.POINTER(_I64),
                             C.POINTER(_I64), _I32, _I32, C.c_float, C.POINTER(_I32)]),
    "vr_lod_pool_layout": (_I32, [C.POINTER(_I64), _I32, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I32), _I32, _I32,
                                  _P, C.POINTER(_I64)]),
    "vr_brickset_decode_lod_pool": (_I32, [_P, C.POINTER(_I32), C.POINTER(_I64), C.POINTER(_I64), _P, _I64, _P, _P]),
    "vr_raycast_pool": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams), _P, _P]),
    "vr_skip_grid_build_pool": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), _I32, _P, _P]),
    "vr_brickset_set_tree": (_I32, [_P, _I32, _P, _I64, _I64, _P, _I32]),
    "vr_stream_block_table": (_I32, [C.POINTER(_I64), _P, _I64, _I64, _P, _I32, _P, _P]),
    "vr_brickset_set_trees": (_I32, [_P, _I32, C.POINTER(_I32), C.POINTER(TreeDesc), _P]),
    "vr_brickset_save_set": (_I32, [_P, C.c_char_p]),
    "vr_brickset_open_set": (_I32, [C.POINTER(_P), C.c_char_p, _P]),
    "vr_brickset_load_set": (_I32, [_P, C.c_char_p, _P]),
    "vr_brickset_load_set_memory": (_I32, [_P, _P, _I64, _P]),
    "vr_brickset_save": (_I32, [_P, _I32, C.c_char_p]),
    "vr_brickset_open": (_I32, [C.POINTER(_P), C.c_char_p]),
    "vr_brickset_open_variant": (_I32, [C.POINTER(_P), C.c_char_p, _I32]),
    "vr_measure_error": (_I32, [_P, _P, _I64, C.POINTER(_I32), C.POINTER(C.c_double), _P]),
    "vr_query_error": (_I32, [_P, _P, _I64, _P, _P]),
    "vr_measure_error_bricks": (_I32, [_P, _P, _I32, _I64, _P, _P]),
    "vr_brickset_error_table": (_I32, [_P, _P, _P, _I32, _I32, _P, _P]),
    "vr_lod_select_error": (_I32, [_P, _I32, _I32, _I32, _I64, C.POINTER(_I32), _I32, C.c_double, C.POINTER(_I32)]),
    "vr_histogram_bricks": (_I32, [_P, _I32, _I64, _P, _P, _P]),
    "vr_histogram_pool": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), _P, _P, _P]),
    "vr_histogram2d": (_I32, [_P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64), _P, _P]),
    "vr_window_from_histogram": (_I32, [_P, _I32, C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]),
    "vr_isomesh_workspace_bytes": (_I32, [C.POINTER(_I64), C.POINTER(IsoMeshDesc), C.POINTER(_I64)]),
    "vr_isomesh_count": (_I32, [_P, C.POINTER(_I64), C.POINTER(IsoMeshDesc), _P, C.POINTER(C.c_uint64), _P]),
    "vr_isomesh_emit": (_I32, [_P, C.POINTER(_I64), C.POINTER(IsoMeshDesc), _P, _I64, _I64, _P, _P, _P, _P]),
    "vr_assemble_bricks": (_I32, [_P, _I32, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64), _P, _P]),
    "vr_disassemble_bricks": (_I32, [_P, _I32, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(_I64), _P, _P]),
    "vr_raycast": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams), _P, _P]),
    "vr_skip_grid_build": (_I32, [_P, C.POINTER(_I64), _I32, _P, _P]),
    "vr_raycast_tf": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(TransferFunctionDesc),
                             _P, _P]),
    "vr_raycast_pool_tf": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                  C.POINTER(TransferFunctionDesc), _P, _P]),
    "vr_raycast_tf_shaded": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                    C.POINTER(TransferFunctionDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_raycast_pool_tf_shaded": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                         C.POINTER(TransferFunctionDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_raycast_tf_partial": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                     C.POINTER(TransferFunctionDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_raycast_pool_tf_partial": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                          C.POINTER(TransferFunctionDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_tf2d_columns_build": (_I32, [_P, _I32, _P, _P]),
    "vr_raycast_tf2d": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                               C.POINTER(TransferFunction2DDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_raycast_pool_tf2d": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                    C.POINTER(TransferFunction2DDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_raycast_tf2d_partial": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                       C.POINTER(TransferFunction2DDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_raycast_pool_tf2d_partial": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                            C.POINTER(TransferFunction2DDesc), C.POINTER(ShadingDesc), _P, _P]),
    "vr_composite_over_tf": (_I32, [_P, _P, _I64, _P]),
    "vr_composite_finish_tf": (_I32, [_P, C.POINTER(TransferFunctionDesc), _P, _I64, _P]),
    "vr_composite_slabs_tf": (_I32, [_P, _I32, _I64, _I64, _I32, C.POINTER(Camera), C.POINTER(RenderParams),
                                     C.POINTER(TransferFunctionDesc), _P, _P]),
    "vr_raycast_projection": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams), C.POINTER(Projection),
                                     _P, _P]),
    "vr_raycast_pool_projection": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                          C.POINTER(Projection), _P, _P]),
    "vr_raycast_projection_partial": (_I32, [_P, C.POINTER(_I64), C.POINTER(Camera), C.POINTER(RenderParams),
                                             C.POINTER(Projection), _P, _P]),
    "vr_raycast_pool_projection_partial": (_I32, [_P, _P, C.POINTER(_I64), C.POINTER(_I64), C.POINTER(Camera),
                                                  C.POINTER(RenderParams), C.POINTER(Projection), _P, _P]),
    "vr_composite_combine_proj": (_I32, [_P, _P, _I64, _I32, _P]),
    "vr_composite_finish_proj": (_I32, [_P, C.POINTER(Projection), _P, _I64, _P]),
    "vr_composite_slabs_proj": (_I32, [_P, _I32, _I64, C.POINTER(Projection), _P, _P]),
    "vr_reslice": (_I32, [_P, C.POINTER(_I64), C.POINTER(SlicePlaneDesc), C.POINTER(Projection), _P, _P]),
    "vr_reslice_partial": (_I32, [_P, C.POINTER(_I64), C.POINTER(SlicePlaneDesc), C.POINTER(Projection), _P, _P]),
    "vr_composite_over": (_I32, [_P, _P, _I64, _P]),
    "vr_composite_finish": (_I32, [_P, _P, _I64, _P]),
    "vr_composite_slabs": (_I32, [_P, _I32, _I64, _I64, _I32, C.POINTER(Camera), C.POINTER(RenderParams), _P, _P]),
    "vr_rccl_unique_id": (_I32, [_P]),
    "vr_compositor_create": (_I32, [C.POINTER(_P), _P, _I32, _I32, _I32, _I32]),
    "vr_compositor_create_from_comm": (_I32, [C.POINTER(_P), _P, _I32, _I32, _I32, _I32]),
    "vr_compositor_create_with_transport": (_I32, [C.POINTER(_P), _P, _P, _I32, _I32, _I32, _I32]),
    "vr_compositor_composite": (_I32, [_P, _P, _I32, C.POINTER(Camera), C.POINTER(RenderParams), _P, _P]),
    "vr_compositor_composite_tf": (_I32, [_P, _P, _I32, C.POINTER(Camera), C.POINTER(RenderParams),
                                          C.POINTER(TransferFunctionDesc), _P, _P]),
    "vr_compositor_composite_proj": (_I32, [_P, _P, C.POINTER(Projection), _P, _P]),
    "vr_compositor_destroy": (_I32, [_P]),
    "vr_stream_create": (_I32, [C.POINTER(_P)]),
    "vr_stream_destroy": (_I32, [_P]),
    "vr_stream_synchronize": (_I32, [_P]),
    "vr_stream_wait_event": (_I32, [_P, _P]),
    "vr_event_create": (_I32, [C.POINTER(_P)]),
    "vr_event_destroy": (_I32, [_P]),
    "vr_event_record": (_I32, [_P, _P]),
    "vr_event_synchronize": (_I32, [_P]),
    "vr_event_elapsed_ms": (_I32, [_P, _P, C.POINTER(C.c_float)]),
    "vr_malloc_host": (_I32, [C.POINTER(_P), _I64]),
    "vr_free_host": (_I32, [_P]),
    "vr_upload_async": (_I32, [_P, _P, _I64, _P]),
    "vr_download_async": (_I32, [_P, _P, _I64, _P]),
    "vr_brickset_last_timings": (_I32, [_P, C.POINTER(C.c_float)]),
    "vr_brickset_set_concurrency": (_I32, [_P, C.c_int32]),
    "vr_brickset_set_switch": (_I32, [_P, C.c_char_p, C.c_int32]),
    "vr_brickset_set_compaction": (_I32, [_P, C.c_int32]),
    "vr_debug_set": (_I32, [C.c_char_p, C.c_int32]),
}

_lib = None


def lib():
    """Loads libvrhip.so.  Raises ImportError if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError("libvrhip.so is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                              "(hipcc --offload-arch=gfx950).  There is no CPU fallback.")
        # PyTorch ships its own libamdhip64; it must be in the process BEFORE libvrhip.so is
        # loaded so that both bind to ONE HIP runtime (device pointers and streams are then
        # interchangeable).  Loading libvrhip.so first would start a second runtime that cannot
        # see the device torch holds.
        import torch  # noqa: F401
        L = C.CDLL(LIB_PATH)
        for name, (res, args) in SIGNATURES.items():
            fn = getattr(L, name)  # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
        _lib = L
    return _lib


def check(status, what=""):
    if status != VR_OK:
        raise VrError(status, what)
