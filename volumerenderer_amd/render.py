"""Host-side mirror of the reference's ingest + render interface over the C ABI.

  VolumeReader   volume_renderer/VolumeReader.h:28-290 (LoadBrickToTexture /
                 LoadBricksToTexture / transferToGPU; the "texture" is a device buffer)
  UnitBrick      volume_renderer/UnitBrick.h:17-119 (Setup/Bind/Draw/Unbind/Delete;
                 Draw() launches the ray-march kernel on the cube's pixel footprint)
"""
import collections
import ctypes as C
import math
import os

import numpy as np
import torch

from . import _lib
from ._lib import Camera, RenderParams, VrError, check
from .codec import _as_dev_u8, _stream_ptr


def default_camera():
    """Start camera of main.cpp:33-40."""
    cam = Camera()
    cam.pos[:] = (0.0, 0.0, -0.75)
    cam.front[:] = (0.0, 0.0, 1.0)
    cam.up[:] = (0.0, 1.0, 0.0)
    cam.fov_deg, cam.z_near, cam.z_far = 50.0, 0.1, 100.0
    return cam


def default_params(width=1600, height=1200, brick_dims=(256, 256, 128), mode=_lib.RENDER_COMPOSITE, iso=40.0 / 255.0):
    """Uniforms set at main.cpp:330-334; MAX_SAMPLES raycaster.frag:14; window main.cpp:27."""
    P = RenderParams()
    P.width, P.height = int(width), int(height)
    P.step_size[:] = tuple(1.0 / d for d in brick_dims)
    P.iso_value = iso
    P.max_samples = 300
    P.mode = mode
    P.box_min[:] = (0.0, 0.0, 0.0)
    P.box_max[:] = (1.0, 1.0, 1.0)
    P.global_dims[:] = (0, 0, 0)
    P.vol_origin[:] = (0, 0, 0)
    P.no_early_exit = 0
    P.skip_cell = 0
    P.skip_grid_dev = None
    return P


def _check_buf(t, what, dtype, numel, device):
    """The C ABI reads and writes through raw pointers: a buffer it is handed must be a contiguous `dtype` tensor of
    exactly `numel` elements on `device`, or the wrapper raises ValueError before anything is launched (as
    distributed.composite_sort_last does)."""
    if not isinstance(t, torch.Tensor):
        raise ValueError("%s must be a torch tensor, not %s" % (what, type(t).__name__))
    if t.dtype != dtype:
        raise ValueError("%s must be %s, not %s" % (what, dtype, t.dtype))
    if t.device != device:
        raise ValueError("%s must be on %s, not %s" % (what, device, t.device))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)
    if t.numel() != numel:
        raise ValueError("%s must hold %d elements, not %d" % (what, numel, t.numel()))


def _skip_grid_bytes(dims, cell):
    n = 2
    for q in dims:
        n *= (int(q) + int(cell) - 1) // int(cell)
    return n


# A volume the frame calls read, dense or a pool: `args` the leading ctypes arguments of its C entry points, `device` where
# it lives, `dims` its (virtual) extents, `keep` the tensors `args` points into.
_Source = collections.namedtuple("_Source", "args device dims keep")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _dense_source(volume, dims):
    """A dense volume of `dims` voxels; ValueError where they do not match."""
    v = _as_dev_u8(volume)
    d = (C.c_int64 * 3)(*[int(q) for q in dims])
    if any(q <= 0 for q in d) or v.numel() != d[0] * d[1] * d[2]:
        raise ValueError("volume size does not match dims")
    return _Source((_ptr(v), d), v.device, list(d), v)


def _check_attached_grid(params, dims, device):
    if params.skip_grid_dev and params.skip_cell > 0:
        # the grid must describe THIS volume at THIS cell size, or skip_bounds reads past it
        g = getattr(params, "_keep_grid", None)
        if g is None or g.data_ptr() != params.skip_grid_dev:
            raise ValueError("attach skip grids with use_skip_grid()")
        _check_buf(g, "skip grid", torch.uint8, _skip_grid_bytes(dims, params.skip_cell), device)


def _out_or_new(out, shape, device, dtype=torch.float32):
    """`out` checked to hold `shape`'s elements on `device`, or a new tensor of that shape."""
    if out is None:
        return torch.empty(shape, dtype=dtype, device=device)
    _check_buf(out, "out", dtype, math.prod(shape), device)
    return out


def _frame(fn, src, cam, params, descriptors, out, stream):
    """The frame call `fn` of the source `src`: the attached skip grid, then each (check, object) of `descriptors` in turn,
    then `out` are checked; the objects' desc() follow cam and params in the C call (None: a NULL argument).  Returns the
    [H][W][4] float32 frame."""
    _check_attached_grid(params, src.dims, src.device)
    for chk, obj in descriptors:
        chk(obj, src.device)
    out = _out_or_new(out, (params.height, params.width, 4), src.device)
    descs = [obj.desc() if obj is not None else None for _, obj in descriptors]
    check(getattr(_lib.lib(), fn)(*src.args, C.byref(cam), C.byref(params),
                                  *[C.byref(d) if d is not None else None for d in descs], _ptr(out), _stream_ptr(stream)), fn)
    return out


def build_skip_grid(volume, dims, cell=8, out=None, stream=None):
    """(min, max) per cell^3 voxels (+1 voxel reach of a trilinear fetch) of a device volume: 2 bytes per cell.
    Attach to render params with use_skip_grid(); the frame stays bit-identical, the marcher just does not fetch
    samples the grid proves irrelevant."""
    v = _as_dev_u8(volume)
    d = (C.c_int64 * 3)(*[int(q) for q in dims])
    if v.numel() != d[0] * d[1] * d[2]:
        raise ValueError("volume size does not match dims")
    if not 1 <= int(cell) <= 64:
        raise ValueError("cell must be 1..64, not %d" % int(cell))
    out = _out_or_new(out, (_skip_grid_bytes(dims, cell),), v.device, torch.uint8)
    check(_lib.lib().vr_skip_grid_build(_ptr(v), d, int(cell), _ptr(out), _stream_ptr(stream)), "vr_skip_grid_build")
    return out


def use_skip_grid(params, grid, cell=8):
    params.skip_cell = int(cell) if grid is not None else 0
    params.skip_grid_dev = grid.data_ptr() if grid is not None else None
    params._keep_grid = grid
    return params


def raycast(volume, dims, cam, params, out=None, stream=None):
    """volume: CUDA uint8 (X*Y*Z, x fastest). Returns float32 CUDA [H][W][4], row 0 = top."""
    return _frame("vr_raycast", _dense_source(volume, dims), cam, params, (), out, stream)


_GREY_PIXEL, _COLOUR_PIXEL = "(c, tau, covered, 0)", "(C.r, C.g, C.b, T)"


def _check_partial(t, what, pixel=_COLOUR_PIXEL):
    """A partial image handed to the combine calls: a contiguous float32 CUDA tensor of whole `pixel`s."""
    if not isinstance(t, torch.Tensor) or not t.is_cuda:
        raise ValueError("%s must be a CUDA tensor" % what)
    if t.numel() == 0 or t.numel() % 4:
        raise ValueError("%s must hold whole %s pixels, not %d floats" % (what, pixel, t.numel()))
    _check_buf(t, what, torch.float32, t.numel(), t.device)


def _check_pair(front, back, pixel=_COLOUR_PIXEL):
    _check_partial(front, "front", pixel)
    _check_buf(back, "back", torch.float32, front.numel(), front.device)


def composite_over(front, back, stream=None):
    """front = front OVER back, in place; both contiguous float32 (c, tau, covered, 0) images of the same size."""
    _check_pair(front, back, _GREY_PIXEL)
    check(_lib.lib().vr_composite_over(_ptr(front), _ptr(back), front.numel() // 4, _stream_ptr(stream)), "vr_composite_over")
    return front


def composite_finish(partial, out=None, stream=None):
    _check_partial(partial, "partial", _GREY_PIXEL)
    out = _out_or_new(out, partial.shape, partial.device)
    check(_lib.lib().vr_composite_finish(_ptr(partial), _ptr(out), partial.numel() // 4, _stream_ptr(stream)),
          "vr_composite_finish")
    return out


def assemble_bricks(bricks, brick_dims, brick_ijk, grid, out=None, stream=None):
    b = _as_dev_u8(bricks)
    bd = (C.c_int64 * 3)(*[int(q) for q in brick_dims])
    g = (C.c_int64 * 3)(*[int(q) for q in grid])
    ijk = np.ascontiguousarray(brick_ijk, np.int64).reshape(-1, 3)
    nb = ijk.shape[0]
    # the volume is the whole I x J x K grid (VolumeReader.h:184-198 writes at grid coordinates); cells with no
    # brick stay zero.  (The reference sizes it by numBricks, VolumeReader.h:163-168, and overruns for sparse lists.)
    vol_bytes = g[0] * g[1] * g[2] * bd[0] * bd[1] * bd[2]
    if b.numel() < nb * bd[0] * bd[1] * bd[2]:
        raise ValueError("assemble_bricks: %d bricks need %d bytes, got %d" % (nb, nb * bd[0] * bd[1] * bd[2], b.numel()))
    if out is None:
        out = torch.zeros(vol_bytes, dtype=torch.uint8, device="cuda")
    elif out.numel() < vol_bytes:
        raise ValueError("assemble_bricks: the volume needs I*J*K*X*Y*Z = %d bytes, out has %d" % (vol_bytes, out.numel()))
    check(_lib.lib().vr_assemble_bricks(C.c_void_p(b.data_ptr()), nb, bd, ijk.ctypes.data_as(C.POINTER(C.c_int64)), g,
                                        C.c_void_p(out.data_ptr()), _stream_ptr(stream)), "vr_assemble_bricks")
    return out


def disassemble_bricks(volume, brick_dims, brick_ijk, grid, out=None, stream=None):
    v = _as_dev_u8(volume)
    bd = (C.c_int64 * 3)(*[int(q) for q in brick_dims])
    g = (C.c_int64 * 3)(*[int(q) for q in grid])
    ijk = np.ascontiguousarray(brick_ijk, np.int64).reshape(-1, 3)
    nb = ijk.shape[0]
    vol_bytes = g[0] * g[1] * g[2] * bd[0] * bd[1] * bd[2]
    if v.numel() < vol_bytes:
        raise ValueError("disassemble_bricks: the volume must hold I*J*K*X*Y*Z = %d bytes, got %d" % (vol_bytes, v.numel()))
    if out is None:
        out = torch.empty(nb * bd[0] * bd[1] * bd[2], dtype=torch.uint8, device="cuda")
    elif out.numel() < nb * bd[0] * bd[1] * bd[2]:
        raise ValueError("disassemble_bricks: out is too small")
    check(_lib.lib().vr_disassemble_bricks(C.c_void_p(v.data_ptr()), nb, bd, ijk.ctypes.data_as(C.POINTER(C.c_int64)), g,
                                           C.c_void_p(out.data_ptr()), _stream_ptr(stream)), "vr_disassemble_bricks")
    return out


def select_lod(cam, params, brick_dims, brick_ijk, grid, orig_tree_depth, max_tree_depth, pixel_tolerance=1.0):
    """Per-brick cuts for BrickSet.decode_lod for the frame raycast(cam, params) draws (vr_lod_select, host only):
    -1 for bricks no ray of the frame reads, coarser cuts for bricks whose voxels project below pixel_tolerance
    pixels.  Bricks as in assemble_bricks.  Returns an int32 numpy array."""
    bd = (C.c_int64 * 3)(*[int(q) for q in brick_dims])
    g = (C.c_int64 * 3)(*[int(q) for q in grid])
    ijk = np.ascontiguousarray(brick_ijk, np.int64).reshape(-1, 3)
    cuts = np.empty(ijk.shape[0], np.int32)
    check(_lib.lib().vr_lod_select(C.byref(cam), C.byref(params), int(ijk.shape[0]), bd,
                                   ijk.ctypes.data_as(C.POINTER(C.c_int64)), g, int(orig_tree_depth), int(max_tree_depth),
                                   float(pixel_tolerance), cuts.ctypes.data_as(C.POINTER(C.c_int32))), "vr_lod_select")
    return cuts


def select_lod_error(table, cut_lo, voxels_per_brick, cuts_in=None, max_abs=0, mean_sq=-1.0):
    """Per-brick cuts bounded by error (vr_lod_select_error, host only; the rule is in vrhip.h): for every brick the
    smallest cut of the table, not above cuts_in[b], whose max_abs is at most `max_abs` and, when mean_sq >= 0, whose
    mean squared error is at most `mean_sq`; cuts_in[b] where none is, -1 where cuts_in[b] is -1.  table: as
    BrickSet.error_table returns it, its row 0 being cut `cut_lo`; cuts_in: what select_lod returns, or None for the
    table's last cut everywhere.  Returns an int32 numpy array."""
    from .codec import BRICK_ERROR
    t = np.ascontiguousarray(table, BRICK_ERROR)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError("select_lod_error: the table must have shape (cuts, bricks)")
    ci = None
    if cuts_in is not None:
        ci = np.ascontiguousarray(np.asarray(cuts_in).reshape(-1), dtype=np.int32)
        if ci.size != t.shape[1]:
            raise ValueError("select_lod_error: %d cuts for %d bricks" % (ci.size, t.shape[1]))
    cuts = np.empty(t.shape[1], np.int32)
    check(_lib.lib().vr_lod_select_error(C.c_void_p(t.ctypes.data), int(t.shape[1]), int(cut_lo),
                                         int(cut_lo) + t.shape[0] - 1, int(voxels_per_brick),
                                         None if ci is None else ci.ctypes.data_as(C.POINTER(C.c_int32)), int(max_abs),
                                         float(mean_sq), cuts.ctypes.data_as(C.POINTER(C.c_int32))), "vr_lod_select_error")
    return cuts


# one row of rate_distortion
RATE_DISTORTION = np.dtype([("cut", "<i4"), ("pool_bytes", "<i8"), ("psnr", "<f8")])


def rate_distortion(bs, table, brick_ijk, grid, cut_lo=0):
    """The rate / distortion curve of a set cut uniformly: per row of `table` (BrickSet.error_table; row 0 = cut
    `cut_lo`) the bytes of the level-of-detail pool with every brick at that cut (lod_pool_layout) and the PSNR of the
    whole volume, 10 log10(255^2 N / sum of sum_sq) dB (inf where the sum is 0).  Host arithmetic only; power-of-two
    brick extents (the pool's).  Returns a RATE_DISTORTION numpy array."""
    info = bs.info(0)
    out = np.zeros(len(table), RATE_DISTORTION)
    n = float(bs.num_bricks) * float(bs.voxels_per_brick)
    for r in range(len(table)):
        cut = int(cut_lo) + r
        _, nbytes = lod_pool_layout(bs.dims, brick_ijk, grid, np.full(bs.num_bricks, cut, np.int32),
                                    info["orig_tree_depth"], info["max_tree_depth"])
        sq = sum(int(v) for v in table[r]["sum_sq"])
        out[r] = (cut, nbytes, math.inf if sq == 0 else 10.0 * math.log10(255.0 * 255.0 * n / sq))
    return out


# vr_pool_entry as numpy: one row per grid cell, x fastest
POOL_ENTRY = np.dtype([("offset", "<i8"), ("shift", "u1", (3,)), ("pad", "u1", (5,))])


def lod_pool_layout(brick_dims, brick_ijk, grid, cuts, orig_tree_depth, max_tree_depth):
    """The pool layout of BrickSet.decode_lod_pool (vr_lod_pool_layout, host only; the rule is in vrhip.h).
    Returns (table, pool_bytes): table a POOL_ENTRY numpy array of grid[0]*grid[1]*grid[2] cells, x fastest."""
    bd = (C.c_int64 * 3)(*[int(q) for q in brick_dims])
    g = (C.c_int64 * 3)(*[int(q) for q in grid])
    ijk = np.ascontiguousarray(brick_ijk, np.int64).reshape(-1, 3)
    c = np.ascontiguousarray(np.asarray(cuts).reshape(-1), dtype=np.int32)
    if c.size != ijk.shape[0]:
        raise ValueError("lod_pool_layout: %d cuts for %d bricks" % (c.size, ijk.shape[0]))
    table = np.zeros(g[0] * g[1] * g[2], POOL_ENTRY)
    nbytes = C.c_int64(0)
    check(_lib.lib().vr_lod_pool_layout(bd, int(ijk.shape[0]), ijk.ctypes.data_as(C.POINTER(C.c_int64)), g,
                                        c.ctypes.data_as(C.POINTER(C.c_int32)), int(orig_tree_depth), int(max_tree_depth),
                                        C.c_void_p(table.ctypes.data), C.byref(nbytes)), "vr_lod_pool_layout")
    return table, int(nbytes.value)


def _check_pool(pool, table, grid, device):
    cells = int(grid[0]) * int(grid[1]) * int(grid[2])
    _check_buf(table, "table", torch.uint8, cells * POOL_ENTRY.itemsize, device)
    if not isinstance(pool, torch.Tensor) or pool.numel() == 0:
        raise ValueError("pool must be a non-empty torch tensor")
    _check_buf(pool, "pool", torch.uint8, pool.numel(), device)


def _pool_source(pool, table, brick_dims, grid):
    """A pool and its table, checked; the source's extents are the virtual volume's.  The table contract is vrhip.h's (at
    vr_pool_entry): any pool and table that keep it, not only decode_lod_pool's; a table that is not 16-byte aligned is
    refused by the C entry points (VrError, VR_ERR_INVALID)."""
    if not isinstance(pool, torch.Tensor):
        raise ValueError("pool must be a torch tensor")
    _check_pool(pool, table, grid, pool.device)
    bd, g = (C.c_int64 * 3)(*[int(q) for q in brick_dims]), (C.c_int64 * 3)(*[int(q) for q in grid])
    return _Source((_ptr(pool), _ptr(table), bd, g), pool.device, [g[k] * bd[k] for k in range(3)], (pool, table))


def build_skip_grid_pool(pool, table, brick_dims, grid, cell=8, out=None, stream=None):
    """build_skip_grid of the virtual volume of a pool (vr_skip_grid_build_pool): the same bytes as build_skip_grid of
    that volume assembled densely.  pool, table: as BrickSet.decode_lod_pool returns them."""
    src = _pool_source(pool, table, brick_dims, grid)
    if not 1 <= int(cell) <= 64:
        raise ValueError("cell must be 1..64, not %d" % int(cell))
    out = _out_or_new(out, (_skip_grid_bytes(src.dims, cell),), src.device, torch.uint8)
    check(_lib.lib().vr_skip_grid_build_pool(*src.args, int(cell), _ptr(out), _stream_ptr(stream)), "vr_skip_grid_build_pool")
    return out


def raycast_pool(pool, table, brick_dims, grid, cam, params, out=None, stream=None):
    """raycast of the virtual volume of a pool (vr_raycast_pool): bit-identical to raycast of that volume assembled
    densely (absent bricks 0).  A skip grid attached with use_skip_grid must come from build_skip_grid_pool (or
    build_skip_grid of the dense volume).  Returns float32 CUDA [H][W][4]."""
    return _frame("vr_raycast_pool", _pool_source(pool, table, brick_dims, grid), cam, params, (), out, stream)


# ---- direct volume rendering with a user transfer function (vr_raycast_tf; the rule is in vrhip.h) -------------------
def transfer_function_table(points):
    """The (256, 4) float32 table of control points (value, r, g, b, a): value in [0, 255], non-decreasing from point to
    point, colours in [0, 1].  Entry k is linear between the last point at or below k and the point after it, the first
    point's colour below the first value and the last point's from the last value on; computed in float64 and rounded
    to float32 (vrhip::transfer_function_from_points in include/vrhip/TransferFunction.hpp is the same rule)."""
    pts = [tuple(float(q) for q in p) for p in points]
    if not pts or any(len(p) != 5 for p in pts):
        raise ValueError("points must be a non-empty list of (value, r, g, b, a)")
    for i, p in enumerate(pts):
        if not all(math.isfinite(q) for q in p) or not 0.0 <= p[0] <= 255.0:
            raise ValueError("point %d: value must lie in [0, 255]" % i)
        if not all(0.0 <= q <= 1.0 for q in p[1:]):
            raise ValueError("point %d: r, g, b, a must lie in [0, 1]" % i)
        if i and p[0] < pts[i - 1][0]:
            raise ValueError("points must be sorted by value")
    out = np.empty((256, 4), np.float32)
    j = -1                                  # the last point at or below k
    for k in range(256):
        while j + 1 < len(pts) and pts[j + 1][0] <= k:
            j += 1
        if j < 0:
            row = pts[0][1:]
        elif j + 1 == len(pts):
            row = pts[-1][1:]
        else:
            (v0, *c0), (v1, *c1) = pts[j], pts[j + 1]
            t = (k - v0) / (v1 - v0)
            row = [a + t * (b - a) for a, b in zip(c0, c1)]
        out[k] = row
    return out


def _lut_host(lut, device):
    """A (256, 4) table of (r, g, b, a) in [0, 1] as contiguous float32 numpy, and the device it goes to (a CUDA
    tensor's own, else `device`)."""
    if isinstance(lut, torch.Tensor):
        device = lut.device if lut.is_cuda else device
        host = lut.detach().to("cpu", torch.float32).numpy()
    else:
        host = np.asarray(lut, np.float32)
    if host.shape != (256, 4):
        raise ValueError("lut must be 256 x (r, g, b, a), not %s" % (tuple(host.shape),))
    if not np.all(np.isfinite(host)) or host.min() < 0.0 or host.max() > 1.0:
        raise ValueError("lut values must lie in [0, 1]")
    return np.ascontiguousarray(host), device


def _enum_arg(value, names, what):
    """The int of a "string or enum int" argument: `names` maps the strings; ValueError(`what`, not ...) otherwise."""
    if isinstance(value, str) and value in names:
        return names[value]
    if isinstance(value, int) and not isinstance(value, bool) and value in names.values():
        return value
    raise ValueError("%s, not %r" % (what, value))


class TransferFunction:
    """A transfer function for raycast_tf / raycast_pool_tf (vr_transfer_function): `lut` the (256, 4) float32 CUDA
    tensor of (r, g, b, a) in [0, 1], entry k for the scalar k / 255; `opacity_unit` the texture-space distance the
    alphas are defined for (0: no correction); `background` the colour behind the volume."""

    def __init__(self, lut, opacity_unit=0.0, background=(1.0, 1.0, 1.0), device="cuda"):
        host, device = _lut_host(lut, device)
        self.opacity_unit = float(opacity_unit)
        if not math.isfinite(self.opacity_unit) or self.opacity_unit < 0.0:
            raise ValueError("opacity_unit must be finite and >= 0, not %r" % opacity_unit)
        self.background = tuple(float(v) for v in background)
        if len(self.background) != 3 or not all(math.isfinite(v) for v in self.background):
            raise ValueError("background must be three finite values")
        self.lut = torch.from_numpy(host).to(device)

    @classmethod
    def from_points(cls, points, opacity_unit=0.0, background=(1.0, 1.0, 1.0), device="cuda"):
        """The table transfer_function_table(points) builds: (value 0..255, r, g, b, a) control points."""
        return cls(transfer_function_table(points), opacity_unit, background, device)

    def desc(self):
        d = _lib.TransferFunctionDesc()
        d.lut_dev = self.lut.data_ptr()
        d.opacity_unit = self.opacity_unit
        d.background[:] = self.background
        return d


def _check_tf(tf, device):
    if not isinstance(tf, TransferFunction):
        raise ValueError("tf must be a TransferFunction, not %s" % type(tf).__name__)
    _check_buf(tf.lut, "tf.lut", torch.float32, 256 * 4, device)


def raycast_tf(volume, dims, cam, params, tf, out=None, stream=None):
    """raycast's frame set-up with the transfer function `tf` (vr_raycast_tf): each sample is looked up in tf's table
    and composited front to back.  params.mode must be RENDER_COMPOSITE.  Returns float32 CUDA [H][W][4] =
    (C + T * background, 1 - T), row 0 = top."""
    return _frame("vr_raycast_tf", _dense_source(volume, dims), cam, params, [(_check_tf, tf)], out, stream)


def raycast_pool_tf(pool, table, brick_dims, grid, cam, params, tf, out=None, stream=None):
    """raycast_tf of the virtual volume of a pool (vr_raycast_pool_tf): bit-identical to raycast_tf of that volume
    assembled densely.  Restrictions and skip grids as raycast_pool."""
    return _frame("vr_raycast_pool_tf", _pool_source(pool, table, brick_dims, grid), cam, params, [(_check_tf, tf)], out, stream)


# ---- gradient-shaded direct volume rendering (vr_raycast_tf_shaded; the rule is in vrhip.h) ---------------------------
class Shading:
    """Lighting for raycast_tf_shaded / raycast_pool_tf_shaded (vr_shading): c = min(1, e.rgb (ambient + diffuse |N.L|)
    + specular |N.H|^shininess) for samples whose gradient magnitude exceeds grad_min.  light_dir is the world direction
    towards the light; (0, 0, 0) is the head light (L = V).  Raises ValueError for negative or non-finite values."""

    def __init__(self, ambient=0.3, diffuse=0.7, specular=0.2, shininess=32.0, light_dir=(0.0, 0.0, 0.0), grad_min=1.0 / 255.0):
        vals = {"ambient": ambient, "diffuse": diffuse, "specular": specular, "shininess": shininess, "grad_min": grad_min}
        for name, v in vals.items():
            v = float(v)
            if not math.isfinite(v) or v < 0.0:
                raise ValueError("%s must be finite and >= 0, not %r" % (name, vals[name]))
            setattr(self, name, v)
        self.light_dir = tuple(float(v) for v in light_dir)
        if len(self.light_dir) != 3 or not all(math.isfinite(v) for v in self.light_dir):
            raise ValueError("light_dir must be three finite values")

    def desc(self):
        d = _lib.ShadingDesc()
        d.ambient, d.diffuse, d.specular, d.shininess = self.ambient, self.diffuse, self.specular, self.shininess
        d.light_dir[:] = self.light_dir
        d.grad_min = self.grad_min
        return d


def _check_shading(shading, device=None):
    if not isinstance(shading, Shading):
        raise ValueError("shading must be a Shading, not %s" % type(shading).__name__)


def _check_shading_or_none(shading, device=None):
    if shading is not None:
        _check_shading(shading)


def raycast_tf_shaded(volume, dims, cam, params, tf, shading, out=None, stream=None):
    """raycast_tf with gradient lighting (vr_raycast_tf_shaded): each sample that contributes is lit by `shading`
    through its lattice gradient.  params.mode must be RENDER_SHADED.  Returns float32 CUDA [H][W][4]."""
    return _frame("vr_raycast_tf_shaded", _dense_source(volume, dims), cam, params, [(_check_tf, tf), (_check_shading, shading)],
                  out, stream)


def raycast_pool_tf_shaded(pool, table, brick_dims, grid, cam, params, tf, shading, out=None, stream=None):
    """raycast_tf_shaded of the virtual volume of a pool (vr_raycast_pool_tf_shaded): bit-identical to
    raycast_tf_shaded of that volume assembled densely.  Restrictions and skip grids as raycast_pool."""
    return _frame("vr_raycast_pool_tf_shaded", _pool_source(pool, table, brick_dims, grid), cam, params,
                  [(_check_tf, tf), (_check_shading, shading)], out, stream)


# ---- sort-last colour partials (vr_raycast_tf_partial and the combine calls; the rule is in vrhip.h) -------------------
def raycast_tf_partial(volume, dims, cam, params, tf, shading=None, out=None, stream=None):
    """The colour partial of raycast_tf (shading=None, params.mode RENDER_COMPOSITE) or raycast_tf_shaded (a Shading,
    RENDER_SHADED) for sort-last compositing (vr_raycast_tf_partial): float32 CUDA [H][W][4] = (C.r, C.g, C.b, T) of the
    samples in params' box; (0, 0, 0, 1) where the ray owns none.  tf.background is not used."""
    return _frame("vr_raycast_tf_partial", _dense_source(volume, dims), cam, params,
                  [(_check_tf, tf), (_check_shading_or_none, shading)], out, stream)


def raycast_pool_tf_partial(pool, table, brick_dims, grid, cam, params, tf, shading=None, out=None, stream=None):
    """raycast_tf_partial of the virtual volume of a pool (vr_raycast_pool_tf_partial): bit-identical to the dense partial
    of that volume assembled densely.  Restrictions and skip grids as raycast_pool."""
    return _frame("vr_raycast_pool_tf_partial", _pool_source(pool, table, brick_dims, grid), cam, params,
                  [(_check_tf, tf), (_check_shading_or_none, shading)], out, stream)


def composite_over_tf(front, back, stream=None):
    """front = front OVER back on colour partials, in place: (C1 + T1 C2, T1 T2); both contiguous float32 (C.r, C.g,
    C.b, T) images of the same size."""
    _check_pair(front, back)
    check(_lib.lib().vr_composite_over_tf(_ptr(front), _ptr(back), front.numel() // 4, _stream_ptr(stream)),
          "vr_composite_over_tf")
    return front


def background_desc(tf):
    """The vr_transfer_function the compositing calls read the background from: tf's own, or for a TransferFunction2D one
    that carries its background and no table (they read only the background)."""
    if isinstance(tf, TransferFunction):
        return tf.desc()
    if isinstance(tf, TransferFunction2D):
        d = _lib.TransferFunctionDesc()
        d.lut_dev = None
        d.opacity_unit = tf.opacity_unit
        d.background[:] = tf.background
        return d
    raise ValueError("tf must be a TransferFunction or a TransferFunction2D, not %s" % type(tf).__name__)


def composite_finish_tf(partial, tf, out=None, stream=None):
    """The frame (C + T background, 1 - T) of a colour partial; of tf (either table class) only the background is used."""
    _check_partial(partial, "partial")
    desc = background_desc(tf)
    out = _out_or_new(out, partial.shape, partial.device)
    check(_lib.lib().vr_composite_finish_tf(_ptr(partial), C.byref(desc), _ptr(out), partial.numel() // 4, _stream_ptr(stream)),
          "vr_composite_finish_tf")
    return out


# ---- two-dimensional transfer functions (vr_raycast_tf2d; the rule is in vrhip.h) --------------------------------------
def tf2d_separable_table(lut1d, weight_by_row):
    """The (rows, 256, 4) float32 table whose row j is the 1-D table with its alpha scaled by w[j]: rgb[j][k] =
    lut1d[k].rgb, a[j][k] = float32(float64(lut1d[k].a) * float64(w[j])), w in [0, 1]
    (vrhip::transfer_function2d_separable in include/vrhip/TransferFunction.hpp is the same rule)."""
    lut = np.asarray(lut1d, np.float32)
    w = np.asarray(weight_by_row, np.float64)
    if lut.shape != (256, 4):
        raise ValueError("lut1d must be 256 x (r, g, b, a), not %s" % (tuple(lut.shape),))
    if w.ndim != 1 or not 2 <= w.shape[0] <= _lib.TF2D_MAX_ROWS:
        raise ValueError("weight_by_row must hold 2..%d weights" % _lib.TF2D_MAX_ROWS)
    if not np.all(np.isfinite(w)) or w.min() < 0.0 or w.max() > 1.0:
        raise ValueError("weights must lie in [0, 1]")
    out = np.empty((w.shape[0], 256, 4), np.float32)
    out[:, :, :3] = lut[None, :, :3]
    out[:, :, 3] = (lut[None, :, 3].astype(np.float64) * w[:, None]).astype(np.float32)
    return out


class TransferFunction2D:
    """A table indexed by value and gradient magnitude for raycast_tf2d & co. (vr_transfer_function2d): `lut` the
    (rows, 256, 4) float32 table of (r, g, b, a) in [0, 1], 2 <= rows <= 256; entry [j][k] for the scalar k / 255 and the
    row coordinate y = |g| * grad_scale = j.  The default grad_scale, 127.5 * (rows - 1) / 110, spreads the rows over the
    whole gradient range (with 111 rows: the row axis of histogram2d).  The column summary the skip grid needs is built
    here and kept (`columns`)."""

    def __init__(self, lut, grad_scale=None, opacity_unit=0.0, background=(1.0, 1.0, 1.0), device="cuda"):
        if isinstance(lut, torch.Tensor):
            device = lut.device if lut.is_cuda else device
            host = lut.detach().to("cpu", torch.float32).numpy()
        else:
            host = np.asarray(lut, np.float32)
        if host.ndim != 3 or host.shape[1:] != (256, 4) or not 2 <= host.shape[0] <= _lib.TF2D_MAX_ROWS:
            raise ValueError("lut must be rows x 256 x (r, g, b, a) with 2 <= rows <= %d, not %s"
                             % (_lib.TF2D_MAX_ROWS, tuple(host.shape)))
        if not np.all(np.isfinite(host)) or host.min() < 0.0 or host.max() > 1.0:
            raise ValueError("lut values must lie in [0, 1]")
        self.rows = int(host.shape[0])
        self.grad_scale = 127.5 * (self.rows - 1) / 110.0 if grad_scale is None else float(grad_scale)
        if not math.isfinite(self.grad_scale) or self.grad_scale <= 0.0:
            raise ValueError("grad_scale must be finite and > 0, not %r" % grad_scale)
        if np.float32(self.grad_scale) == 0.0 or not np.isfinite(np.float32(self.grad_scale)):
            raise ValueError("grad_scale must be finite and > 0 as float32, not %r" % grad_scale)
        self.opacity_unit = float(opacity_unit)
        if not math.isfinite(self.opacity_unit) or self.opacity_unit < 0.0:
            raise ValueError("opacity_unit must be finite and >= 0, not %r" % opacity_unit)
        self.background = tuple(float(v) for v in background)
        if len(self.background) != 3 or not all(math.isfinite(v) for v in self.background):
            raise ValueError("background must be three finite values")
        self.lut = torch.from_numpy(np.ascontiguousarray(host)).to(device)
        if self.lut.is_cuda:
            self.columns = torch.empty(256, dtype=torch.int16, device=self.lut.device)
            check(_lib.lib().vr_tf2d_columns_build(_ptr(self.lut), self.rows, _ptr(self.columns), _stream_ptr()),
                  "vr_tf2d_columns_build")
        else:
            # a host table (the CPU path of composite_sort_last_tf reads only the background): the same summary in
            # NumPy; host pointers never reach the kernel, and the frame calls refuse such a table (_check_tf2d)
            opaque = (host[:, :, 3] != 0.0).any(0)
            first = np.where(opaque, np.arange(256), 256)
            self.columns = torch.from_numpy(np.minimum.accumulate(first[::-1])[::-1].astype(np.int16))

    @classmethod
    def from_separable(cls, lut1d, weight_by_row, grad_scale=None, opacity_unit=0.0, background=(1.0, 1.0, 1.0), device="cuda"):
        """The table tf2d_separable_table(lut1d, weight_by_row) builds: the 1-D table's colours in every row, its alpha
        scaled by the row's weight."""
        if isinstance(lut1d, torch.Tensor):
            lut1d = lut1d.detach().cpu().numpy()
        return cls(tf2d_separable_table(lut1d, weight_by_row), grad_scale, opacity_unit, background, device)

    def desc(self):
        d = _lib.TransferFunction2DDesc()
        d.lut_dev = self.lut.data_ptr()
        d.columns_dev = self.columns.data_ptr()
        d.rows = self.rows
        d.grad_scale = self.grad_scale
        d.opacity_unit = self.opacity_unit
        d.background[:] = self.background
        return d


def _check_tf2d(tf, device):
    if not isinstance(tf, TransferFunction2D):
        raise ValueError("tf must be a TransferFunction2D, not %s" % type(tf).__name__)
    _check_buf(tf.lut, "tf.lut", torch.float32, tf.rows * 256 * 4, device)
    _check_buf(tf.columns, "tf.columns", torch.int16, 256, device)


def _tf2d_frame(fn, src, cam, params, tf, shading, out, stream):
    return _frame(fn, src, cam, params, [(_check_tf2d, tf), (_check_shading_or_none, shading)], out, stream)


def raycast_tf2d(volume, dims, cam, params, tf, shading=None, out=None, stream=None):
    """raycast_tf's march with the two-dimensional table `tf` (vr_raycast_tf2d): every sample is looked up by its value
    and the magnitude of its lattice gradient; with a Shading the colour is lit as raycast_tf_shaded lights it.
    params.mode must be RENDER_SHADED, lit or not; a slab holds two halo layers (slab_params(..., halo=2)).  Returns
    float32 CUDA [H][W][4]."""
    return _tf2d_frame("vr_raycast_tf2d", _dense_source(volume, dims), cam, params, tf, shading, out, stream)


def raycast_pool_tf2d(pool, table, brick_dims, grid, cam, params, tf, shading=None, out=None, stream=None):
    """raycast_tf2d of the virtual volume of a pool (vr_raycast_pool_tf2d): bit-identical to raycast_tf2d of that volume
    assembled densely.  Restrictions and skip grids as raycast_pool."""
    return _tf2d_frame("vr_raycast_pool_tf2d", _pool_source(pool, table, brick_dims, grid), cam, params, tf, shading, out, stream)


def raycast_tf2d_partial(volume, dims, cam, params, tf, shading=None, out=None, stream=None):
    """The colour partial (C.r, C.g, C.b, T) of raycast_tf2d for sort-last compositing (vr_raycast_tf2d_partial); it
    goes through composite_over_tf / composite_finish_tf and distributed.composite_sort_last_tf unchanged."""
    return _tf2d_frame("vr_raycast_tf2d_partial", _dense_source(volume, dims), cam, params, tf, shading, out, stream)


def raycast_pool_tf2d_partial(pool, table, brick_dims, grid, cam, params, tf, shading=None, out=None, stream=None):
    """raycast_tf2d_partial of the virtual volume of a pool (vr_raycast_pool_tf2d_partial): bit-identical to the dense
    partial of that volume assembled densely."""
    return _tf2d_frame("vr_raycast_pool_tf2d_partial", _pool_source(pool, table, brick_dims, grid), cam, params, tf, shading,
                       out, stream)


# ---- intensity projections (vr_raycast_projection and the combine calls; the rule is in vrhip.h) ----------------------
_PROJECT_OPS = {"max": _lib.PROJECT_MAX, "min": _lib.PROJECT_MIN, "mean": _lib.PROJECT_MEAN}


class Projection:
    """An intensity projection for raycast_projection & co. (vr_projection): `op` "max" (MIP), "min" (MinIP) or "mean"
    (or PROJECT_MAX / PROJECT_MIN / PROJECT_MEAN); `window` = (lo, hi), the displayed value is clamp((m - lo) / (hi - lo),
    0, 1); `background` the colour of pixels whose ray owns no sample; `lut` None for a grey frame, else a (256, 4)
    colour map of (r, g, b, a) in [0, 1] looked up with the displayed value.  Raises ValueError on bad values."""

    def __init__(self, op="max", window=(0.0, 1.0), background=(0.0, 0.0, 0.0), lut=None, device="cuda"):
        self.op = _enum_arg(op, _PROJECT_OPS, "op must be 'max', 'min' or 'mean'")
        try:
            self.window = tuple(float(v) for v in window)
        except TypeError:
            raise ValueError("window must be (lo, hi), not %r" % (window,))
        if len(self.window) != 2 or not all(math.isfinite(v) for v in self.window) or not self.window[1] > self.window[0]:
            raise ValueError("window must be finite with hi > lo, not %r" % (window,))
        # the C ABI holds the window as float32: hi > lo must survive the rounding
        if not np.float32(self.window[1]) > np.float32(self.window[0]) or not np.isfinite(np.float32(self.window[1]) - np.float32(self.window[0])):
            raise ValueError("window must be finite with hi > lo in float32, not %r" % (window,))
        self.background = tuple(float(v) for v in background)
        if len(self.background) != 3 or not all(math.isfinite(v) for v in self.background):
            raise ValueError("background must be three finite values")
        self.lut = None
        if lut is not None:
            host, device = _lut_host(lut, device)
            self.lut = torch.from_numpy(host).to(device)

    def desc(self):
        d = _lib.Projection()
        d.lut_dev = self.lut.data_ptr() if self.lut is not None else None
        d.op = self.op
        d.window_lo, d.window_hi = self.window
        d.background[:] = self.background
        return d


def _check_projection(proj, device):
    if not isinstance(proj, Projection):
        raise ValueError("proj must be a Projection, not %s" % type(proj).__name__)
    if proj.lut is not None:
        _check_buf(proj.lut, "proj.lut", torch.float32, 256 * 4, device)


def raycast_projection(volume, dims, cam, params, proj, out=None, stream=None):
    """The intensity projection `proj` of a dense volume (vr_raycast_projection): raycast's rays, no early exit; the
    maximum, minimum or mean of every ray's samples in params' box, windowed, grey or through proj.lut.  params.mode must
    be RENDER_PROJECTION.  Returns float32 CUDA [H][W][4], row 0 = top; (background, 0) where the ray owns no sample."""
    return _frame("vr_raycast_projection", _dense_source(volume, dims), cam, params, [(_check_projection, proj)], out, stream)


def raycast_pool_projection(pool, table, brick_dims, grid, cam, params, proj, out=None, stream=None):
    """raycast_projection of the virtual volume of a pool (vr_raycast_pool_projection): bit-identical to
    raycast_projection of that volume assembled densely.  Restrictions and skip grids as raycast_pool."""
    return _frame("vr_raycast_pool_projection", _pool_source(pool, table, brick_dims, grid), cam, params,
                  [(_check_projection, proj)], out, stream)


def raycast_projection_partial(volume, dims, cam, params, proj, out=None, stream=None):
    """The projection partial of raycast_projection for sort-last compositing (vr_raycast_projection_partial): float32
    CUDA [H][W][4] = (v, n, 0, 0), n the owned samples and v their maximum, minimum or sum; zeros where n = 0."""
    return _frame("vr_raycast_projection_partial", _dense_source(volume, dims), cam, params, [(_check_projection, proj)], out,
                  stream)


def raycast_pool_projection_partial(pool, table, brick_dims, grid, cam, params, proj, out=None, stream=None):
    """raycast_projection_partial of the virtual volume of a pool (vr_raycast_pool_projection_partial)."""
    return _frame("vr_raycast_pool_projection_partial", _pool_source(pool, table, brick_dims, grid), cam, params,
                  [(_check_projection, proj)], out, stream)


def composite_combine_proj(front, back, proj, stream=None):
    """front = combine(front, back) on projection partials, in place: n adds, v is the max, the min or the sum by
    proj.op; a partial with n = 0 is ignored.  Both contiguous float32 (v, n, 0, 0) images of the same size."""
    _check_pair(front, back)
    if not isinstance(proj, Projection):
        raise ValueError("proj must be a Projection, not %s" % type(proj).__name__)
    check(_lib.lib().vr_composite_combine_proj(_ptr(front), _ptr(back), front.numel() // 4, proj.op, _stream_ptr(stream)),
          "vr_composite_combine_proj")
    return front


def composite_finish_proj(partial, proj, out=None, stream=None):
    """The frame of a projection partial (vr_composite_finish_proj): the window, then grey or proj.lut."""
    _check_partial(partial, "partial")
    _check_projection(proj, partial.device)
    out = _out_or_new(out, partial.shape, partial.device)
    desc = proj.desc()
    check(_lib.lib().vr_composite_finish_proj(_ptr(partial), C.byref(desc), _ptr(out), partial.numel() // 4,
                                              _stream_ptr(stream)), "vr_composite_finish_proj")
    return out


# ---- slice views (vr_reslice; the rule is in vrhip.h) -------------------------------------------------------------------
_SLICE_FILTERS = {"nearest": _lib.SLICE_NEAREST, "linear": _lib.SLICE_LINEAR}
# the image axes (column, row) of an axis-aligned slice: axial (axis 2) shows x across and y down, coronal (1) x and z,
# sagittal (0) y and z
_SLICE_IMAGE_AXES = {0: (1, 2), 1: (0, 2), 2: (0, 1)}


def _vec3(v, what):
    try:
        t = tuple(float(q) for q in v)
    except TypeError:
        raise ValueError("%s must be three numbers, not %r" % (what, v))
    if len(t) != 3 or not all(abs(q) <= 3.4028234663852886e38 for q in t):      # finite as float32, the ABI's type
        raise ValueError("%s must be three finite values, not %r" % (what, v))
    return t


class SlicePlane:
    """A slice for reslice & co. (vr_slice_plane): `width` x `height` pixels by `layers` layers of samples at
    origin + px du + py dv + l dw in texture space ([0, 1]^3 is the volume; row 0 is the row of `origin`).  filter:
    "linear" (the marcher's trilinear fetch) or "nearest" (or SLICE_LINEAR / SLICE_NEAREST).  box_min, box_max,
    global_dims and vol_origin are a rank's slab (distributed.slab_plane sets them); the defaults are one GPU's.
    Raises ValueError on bad values."""

    def __init__(self, width, height, origin, du, dv, dw=(0.0, 0.0, 0.0), layers=1, filter="linear",
                 box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), global_dims=(0, 0, 0), vol_origin=(0, 0, 0)):
        for name, v in (("width", width), ("height", height), ("layers", layers)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError("%s must be a positive integer, not %r" % (name, v))
        self.width, self.height, self.layers = int(width), int(height), int(layers)
        if self.layers > 1 << 24 or self.width >= 1 << 31 or self.height >= 1 << 31:
            raise ValueError("width, height must fit an int32 and layers 2^24, not %r x %r x %r" % (width, height, layers))
        self.filter = _enum_arg(filter, _SLICE_FILTERS, "filter must be 'nearest' or 'linear'")
        self.origin, self.du, self.dv, self.dw = _vec3(origin, "origin"), _vec3(du, "du"), _vec3(dv, "dv"), _vec3(dw, "dw")
        self.box_min, self.box_max = _vec3(box_min, "box_min"), _vec3(box_max, "box_max")
        self.global_dims = tuple(int(q) for q in global_dims)
        self.vol_origin = tuple(int(q) for q in vol_origin)
        if len(self.global_dims) != 3 or len(self.vol_origin) != 3 or min(self.global_dims + self.vol_origin) < 0:
            raise ValueError("global_dims and vol_origin must be three non-negative integers")

    @classmethod
    def axis_aligned(cls, dims, axis, index, pixels_per_voxel=1, layers=1, filter="linear"):
        """The slice of a volume of `dims` = (X, Y, Z) voxels through voxel layer `index` along `axis`: axial (axis 2)
        shows x across and y down, coronal (1) x and z, sagittal (0) y and z.  With pixels_per_voxel = 1 the frame has
        one pixel per voxel and the pixel centres ARE the voxel centres; otherwise the frame covers the same extent
        with round(n * pixels_per_voxel) pixels per axis.  layers > 1: a slab of the voxel layers index, index + 1, ..."""
        dims = [int(q) for q in dims]
        if len(dims) != 3 or min(dims) < 1 or axis not in (0, 1, 2) or not 0 <= int(index) < dims[axis]:
            raise ValueError("axis_aligned: axis %r, index %r, extents %r" % (axis, index, dims))
        if not (float(pixels_per_voxel) > 0.0 and math.isfinite(float(pixels_per_voxel))):
            raise ValueError("pixels_per_voxel must be positive, not %r" % (pixels_per_voxel,))
        cu, cv = _SLICE_IMAGE_AXES[axis]
        W, H = max(1, int(round(dims[cu] * pixels_per_voxel))), max(1, int(round(dims[cv] * pixels_per_voxel)))
        origin, du, dv, dw = [0.0] * 3, [0.0] * 3, [0.0] * 3, [0.0] * 3
        du[cu], dv[cv], dw[axis] = 1.0 / W, 1.0 / H, 1.0 / dims[axis]
        origin[cu], origin[cv], origin[axis] = 0.5 / W, 0.5 / H, (int(index) + 0.5) / dims[axis]
        return cls(W, H, origin, du, dv, dw, layers, filter)

    @classmethod
    def from_frame(cls, center, right, down, width, height, pitch, layers=1, layer_pitch=None, filter="linear"):
        """An oblique slice: the frame is centred on `center` (texture space), its columns run along `right` and its
        rows along `down` (texture-space directions, normalised here), `pitch` apart; the layers are stacked along
        right x down, `layer_pitch` (default: pitch) apart and centred on `center` too."""
        # plain double arithmetic in a fixed order: vrhip::slice_from_frame (include/vrhip/Slice.hpp) is the same rule
        c, r, d = _vec3(center, "center"), _vec3(right, "right"), _vec3(down, "down")
        for name, v in (("width", width), ("height", height), ("layers", layers)):
            if isinstance(v, bool) or int(v) != v or int(v) < 1:
                raise ValueError("%s must be a positive integer, not %r" % (name, v))

        def unit(v, what):
            l = math.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])
            if not l > 0.0:
                raise ValueError(what)
            return (v[0] / l, v[1] / l, v[2] / l)

        r, d = unit(r, "right must not be zero"), unit(d, "down must not be zero")
        n = unit((r[1] * d[2] - r[2] * d[1], r[2] * d[0] - r[0] * d[2], r[0] * d[1] - r[1] * d[0]),
                 "right and down must not be parallel")
        pitch = float(pitch)
        lp = pitch if layer_pitch is None else float(layer_pitch)
        if not (math.isfinite(pitch) and pitch > 0.0 and math.isfinite(lp)):
            raise ValueError("pitch must be positive and layer_pitch finite")
        du, dv, dw = [q * pitch for q in r], [q * pitch for q in d], [q * lp for q in n]
        hw, hh, hl = 0.5 * (int(width) - 1), 0.5 * (int(height) - 1), 0.5 * (int(layers) - 1)
        origin = [c[k] - hw * du[k] - hh * dv[k] - hl * dw[k] for k in range(3)]
        return cls(width, height, origin, du, dv, dw, layers, filter)

    def desc(self):
        d = _lib.SlicePlaneDesc()
        d.width, d.height, d.layers, d.filter = self.width, self.height, self.layers, self.filter
        d.origin[:], d.du[:], d.dv[:], d.dw[:] = self.origin, self.du, self.dv, self.dw
        d.box_min[:], d.box_max[:] = self.box_min, self.box_max
        d.global_dims[:], d.vol_origin[:] = self.global_dims, self.vol_origin
        return d


def _check_plane(plane):
    if not isinstance(plane, SlicePlane):
        raise ValueError("plane must be a SlicePlane, not %s" % type(plane).__name__)


def _slice_out(out, plane, device):
    return _out_or_new(out, (plane.height, plane.width, 4), device)


def _reslice_dense(fn, volume, dims, plane, proj, out, stream):
    src = _dense_source(volume, dims)
    _check_plane(plane)
    _check_projection(proj, src.device)
    out = _slice_out(out, plane, src.device)
    pd, desc = plane.desc(), proj.desc()
    check(getattr(_lib.lib(), fn)(*src.args, C.byref(pd), C.byref(desc), _ptr(out), _stream_ptr(stream)), fn)
    return out


def reslice(volume, dims, plane, proj, out=None, stream=None):
    """The slice `plane` of a dense volume (vr_reslice): per pixel the maximum, minimum or mean (proj.op) of the plane's
    layers of samples, windowed, grey or through proj.lut; one layer is a thin slice.  Returns float32 CUDA [H][W][4];
    (background, 0) where no sample lies inside the volume."""
    return _reslice_dense("vr_reslice", volume, dims, plane, proj, out, stream)


def reslice_partial(volume, dims, plane, proj, out=None, stream=None):
    """The projection partial of reslice for sort-last compositing (vr_reslice_partial): float32 CUDA [H][W][4] =
    (v, n, 0, 0); it combines and finishes through composite_combine_proj / composite_finish_proj."""
    return _reslice_dense("vr_reslice_partial", volume, dims, plane, proj, out, stream)


# ---- volume histograms (vr_histogram_bricks & co.; the rule is in vrhip.h) ----------------------------------------------
HIST_BINS, HIST_GRAD_BINS = 256, 111


def histogram_bricks(data, num_bricks, stream=None):
    """The 256-bin histograms of `num_bricks` equal bricks laid out back to back (vr_histogram_bricks): returns
    (bricks, total), a (num_bricks, 256) uint32 and a (256,) uint64 numpy array of exact counts; the rows of `bricks` sum
    to `total`.  `data` may start at any byte."""
    d = _as_dev_u8(data)
    nb = int(num_bricks)
    if nb < 1 or nb >= 1 << 31 or d.numel() == 0 or d.numel() % nb or d.numel() // nb > 0xFFFFFFFF:
        raise ValueError("histogram_bricks: %d bytes for %d bricks (of 1 .. 2^32 - 1 bytes each)" % (d.numel(), nb))
    bricks, total = np.zeros((nb, HIST_BINS), np.uint32), np.zeros(HIST_BINS, np.uint64)
    check(_lib.lib().vr_histogram_bricks(_ptr(d), nb, d.numel() // nb, C.c_void_p(bricks.ctypes.data),
                                         C.c_void_p(total.ctypes.data), _stream_ptr(stream)), "vr_histogram_bricks")
    return bricks, total


def histogram(volume, stream=None):
    """The 256-bin histogram of a device buffer of up to 2^32 - 1 bytes (one brick = the whole tensor): a (256,) uint64
    numpy array.  Larger buffers: histogram_bricks, whose total is carried in 64 bits."""
    d = _as_dev_u8(volume)
    if d.numel() == 0 or d.numel() > 0xFFFFFFFF:
        raise ValueError("histogram: %d bytes (1 .. 2^32 - 1; cut larger buffers into bricks)" % d.numel())
    total = np.zeros(HIST_BINS, np.uint64)
    check(_lib.lib().vr_histogram_bricks(_ptr(d), 1, d.numel(), None, C.c_void_p(total.ctypes.data), _stream_ptr(stream)),
          "vr_histogram_bricks")
    return total


def histogram_pool(pool, table, brick_dims, grid, stream=None):
    """The histogram of the virtual volume of a pool (vr_histogram_pool), per grid cell and in total: (cells, total), a
    (cells, 256) uint32 and a (256,) uint64 numpy array.  Equal to histogram_bricks of that volume laid out brick by
    brick: a coarse cell's stored voxels count for the box they stand for, an absent cell is all zeros."""
    src = _pool_source(pool, table, brick_dims, grid)
    bd, g = [int(q) for q in brick_dims], [int(q) for q in grid]
    if len(bd) != 3 or len(g) != 3 or any(q < 1 or q & (q - 1) for q in bd) or any(q < 1 for q in g) \
            or bd[0] * bd[1] * bd[2] > 0xFFFFFFFF or g[0] * g[1] * g[2] >= 1 << 31 or any(g[k] >= (1 << 31) // bd[k] for k in range(3)):
        raise ValueError("histogram_pool: bricks %r (powers of two, at most 2^32 - 1 voxels) on a grid %r" % (bd, g))
    cells, total = np.zeros((g[0] * g[1] * g[2], HIST_BINS), np.uint32), np.zeros(HIST_BINS, np.uint64)
    check(_lib.lib().vr_histogram_pool(*src.args, C.c_void_p(cells.ctypes.data), C.c_void_p(total.ctypes.data),
                                       _stream_ptr(stream)), "vr_histogram_pool")
    return cells, total


def _int3(v, what):
    try:
        t = tuple(int(q) for q in v)
    except TypeError:
        raise ValueError("%s must be three integers, not %r" % (what, v))
    if len(t) != 3:
        raise ValueError("%s must be three integers, not %r" % (what, v))
    return t


def histogram2d(volume, dims, global_dims=None, vol_origin=(0, 0, 0), own_lo=None, own_hi=None, stream=None):
    """The joint histogram of value and gradient magnitude (vr_histogram2d): a (111, 256) uint64 numpy array, entry
    [r, v] the owned voxels of value v whose central-difference gradient has isqrt(dx^2 + dy^2 + dz^2) >> 2 == r.
    `volume` holds the voxels [vol_origin, vol_origin + dims) of a volume of `global_dims` (default: dims); the owned
    voxels are [own_lo, own_hi) in global coordinates (default: all the volume holds).  The volume must hold every
    clamped neighbour of every owned voxel -- one halo layer beyond the own box (distributed.slab_voxels) -- else
    ValueError, raised before anything touches a device.  Its column sums are the histogram of the owned voxels; the tables of boxes that tile a volume add up
    to the whole volume's."""
    d = _int3(dims, "dims")
    G = d if global_dims is None else tuple(g or q for g, q in zip(_int3(global_dims, "global_dims"), d))
    org = _int3(vol_origin, "vol_origin")
    lo = org if own_lo is None else _int3(own_lo, "own_lo")
    hi = tuple(o + q for o, q in zip(org, d)) if own_hi is None else _int3(own_hi, "own_hi")
    for k in range(3):
        end = org[k] + d[k]
        if not (0 < d[k] < 1 << 31 and 0 < G[k] < 1 << 31 and 0 <= org[k] and end <= G[k]):
            raise ValueError("histogram2d: axis %d: %d voxels at %d of %d" % (k, d[k], org[k], G[k]))
        if not (org[k] <= lo[k] < hi[k] <= end):
            raise ValueError("histogram2d: axis %d: own box [%d, %d) of the voxels [%d, %d)" % (k, lo[k], hi[k], org[k], end))
        if max(lo[k] - 1, 0) < org[k] or min(hi[k], G[k] - 1) > end - 1:
            raise ValueError("histogram2d: axis %d: the volume holds [%d, %d) and no halo layer around the own box [%d, %d)"
                             % (k, org[k], end, lo[k], hi[k]))
    src = _dense_source(volume, d)
    I3 = C.c_int64 * 3
    hist = np.zeros((HIST_GRAD_BINS, HIST_BINS), np.uint64)
    check(_lib.lib().vr_histogram2d(src.args[0], src.args[1], I3(*G), I3(*org), I3(*lo), I3(*hi), C.c_void_p(hist.ctypes.data),
                                    _stream_ptr(stream)), "vr_histogram2d")
    return hist


def window_from_histogram(hist, first_bin=0, lo_fraction=0.01, hi_fraction=0.99):
    """A display window (lo, hi) from the percentiles of a 256-bin histogram (vr_window_from_histogram, host only; the
    rule is in vrhip.h): lo is the bin where the cumulative count of the bins from `first_bin` on passes lo_fraction of
    their sum, hi where it reaches hi_fraction; both as value / 255, always 0 <= lo < hi <= 1.  first_bin = 1 leaves the
    background out.  A (111, 256) table of histogram2d is summed over its rows first."""
    h = np.asarray(hist)
    if h.shape == (HIST_GRAD_BINS, HIST_BINS):
        h = h.sum(0)
    if h.shape != (HIST_BINS,) or h.dtype.kind not in "ui" or (h.dtype.kind == "i" and h.min() < 0):
        raise ValueError("window_from_histogram: 256 counts, not %s %s" % (h.dtype, h.shape))
    h = np.ascontiguousarray(h, np.uint64)
    fb, lf, hf = int(first_bin), float(lo_fraction), float(hi_fraction)
    if not 0 <= fb <= 255 or not (0.0 <= lf <= hf <= 1.0):
        raise ValueError("window_from_histogram: first_bin %r, fractions %r .. %r" % (first_bin, lo_fraction, hi_fraction))
    if not h[fb:].any():
        raise ValueError("window_from_histogram: no counts from bin %d on" % fb)
    lo, hi = C.c_float(), C.c_float()
    check(_lib.lib().vr_window_from_histogram(C.c_void_p(h.ctypes.data), fb, lf, hf, C.byref(lo), C.byref(hi)),
          "vr_window_from_histogram")
    return lo.value, hi.value


def projection_from_histogram(hist, op="max", first_bin=0, lo_fraction=0.01, hi_fraction=0.99, background=(0.0, 0.0, 0.0),
                              lut=None, device="cuda"):
    """A Projection whose window is window_from_histogram(hist, first_bin, lo_fraction, hi_fraction)."""
    return Projection(op, window_from_histogram(hist, first_bin, lo_fraction, hi_fraction), background, lut, device)


class IsoMesh:
    """An indexed triangle mesh of an iso-surface (vrhip.h "iso-surface meshes"), device tensors: `positions` (V, 3)
    float32 in voxel-centre index coordinates, `gradients` (V, 3) float32 or None (unnormalised, exact; -g points
    outwards), `triangles` (T, 3) int32 holding the uint32 indices' bits (torch has no arithmetic on uint32 here; an index
    below 2^31 reads as itself, `triangles.to(torch.int64) & 0xFFFFFFFF` is exact for all)."""

    def __init__(self, positions, gradients, triangles):
        self.positions, self.gradients, self.triangles = positions, gradients, triangles

    @property
    def num_vertices(self):
        return int(self.positions.shape[0])

    @property
    def num_triangles(self):
        return int(self.triangles.shape[0])

    def world_positions(self, global_dims):
        """The positions in the renderer's world cube: (pos + 0.5) / G - 0.5."""
        G = torch.tensor(_int3(global_dims, "global_dims"), dtype=torch.float32, device=self.positions.device)
        return (self.positions + 0.5) / G - 0.5

    def normals(self):
        """Unit outward normals, -g / |g|; zero where g is zero.  ValueError for a mesh made without gradients."""
        if self.gradients is None:
            raise ValueError("IsoMesh.normals: the mesh has no gradients (isosurface_mesh(..., gradients=True))")
        n = torch.linalg.vector_norm(self.gradients, dim=1, keepdim=True)
        return torch.where(n > 0, -self.gradients / torch.where(n > 0, n, torch.ones_like(n)), torch.zeros_like(self.gradients))

    @staticmethod
    def concat(meshes):
        """One mesh of several (the meshes of disjoint cell boxes, e.g. of the ranks' slabs): vertices and triangles
        appended in order, the indices rebased.  Seam vertices stay duplicated."""
        meshes = list(meshes)
        if not meshes:
            raise ValueError("IsoMesh.concat: no meshes")
        with_g = [m.gradients is not None for m in meshes]
        if any(with_g) != all(with_g):
            raise ValueError("IsoMesh.concat: some meshes have gradients and some have none")
        if sum(m.num_vertices for m in meshes) > 0xFFFFFFFF:
            raise ValueError("IsoMesh.concat: more than 2^32 - 1 vertices")
        tris, base = [], 0
        for m in meshes:
            off = base - (1 << 32) if base >= 1 << 31 else base          # the same bits as an int32
            tris.append(m.triangles + off)
            base += m.num_vertices
        return IsoMesh(torch.cat([m.positions for m in meshes]),
                       torch.cat([m.gradients for m in meshes]) if all(with_g) else None, torch.cat(tris))


def isomesh_desc(dims, iso_value, cap=False, gradients=False, global_dims=None, vol_origin=(0, 0, 0), own_lo=None, own_hi=None):
    """The checked vr_isomesh_desc of isosurface_mesh's arguments (ValueError for what the C call would refuse)."""
    d = _int3(dims, "dims")
    G = d if global_dims is None else tuple(g or q for g, q in zip(_int3(global_dims, "global_dims"), d))
    org = _int3(vol_origin, "vol_origin")
    cap = bool(cap)
    lo = ((-1,) * 3 if cap else (0,) * 3) if own_lo is None else _int3(own_lo, "own_lo")
    hi = (G if cap else tuple(g - 1 for g in G)) if own_hi is None else _int3(own_hi, "own_hi")
    iso = float(iso_value)
    if not math.isfinite(iso) or abs(iso) > 3.4028234663852886e38:      # (the desc carries it as a float32)
        raise ValueError("isosurface_mesh: iso_value %r is not finite" % (iso_value,))
    grow = 1 if gradients else 0
    for k in range(3):
        end = org[k] + d[k]
        if not (0 < d[k] < 1 << 31 and 0 < G[k] < 1 << 31 and 0 <= org[k] and end <= G[k]):
            raise ValueError("isosurface_mesh: axis %d: %d voxels at %d of %d" % (k, d[k], org[k], G[k]))
        if not ((-1 if cap else 0) <= lo[k] <= hi[k] <= (G[k] if cap else G[k] - 1)):
            raise ValueError("isosurface_mesh: axis %d: own cells [%d, %d) of the cells [%d, %d)"
                             % (k, lo[k], hi[k], -1 if cap else 0, G[k] if cap else G[k] - 1))
        if max(lo[k] - grow, 0) < org[k] or min(hi[k] + grow, G[k] - 1) > end - 1:
            raise ValueError("isosurface_mesh: axis %d: the volume holds [%d, %d), not every point of [%d, %d]%s"
                             % (k, org[k], end, lo[k], hi[k], " grown by one for the gradients" if grow else ""))
    desc = _lib.IsoMeshDesc()
    desc.iso_value, desc.cap = iso, int(cap)
    desc.global_dims[:], desc.vol_origin[:], desc.own_lo[:], desc.own_hi[:] = G, org, lo, hi
    return desc


def isosurface_mesh(volume, dims, iso_value, cap=False, gradients=False, global_dims=None, vol_origin=(0, 0, 0), own_lo=None,
                    own_hi=None, stream=None):
    """The iso-surface of a dense device volume as an IsoMesh (vr_isomesh_count + vr_isomesh_emit; the rule is in
    vrhip.h).  `volume` holds the voxels [vol_origin, vol_origin + dims) of a volume of `global_dims` (default: dims);
    the call owns the cells own_lo <= c < own_hi in global cell coordinates (default: every cell; with cap=True the
    cells from -1 to G, which close the surface at the volume's faces).  iso_value as in RenderParams: the surface is
    at iso_value * 255.  The meshes of disjoint own boxes (distributed.slab_cells) concatenate to the whole mesh
    (IsoMesh.concat).  ValueError before any C call for arguments the library would refuse."""
    desc = isomesh_desc(dims, iso_value, cap, gradients, global_dims, vol_origin, own_lo, own_hi)
    held = volume.numel() if isinstance(volume, torch.Tensor) else np.size(volume)
    if held != math.prod(_int3(dims, "dims")):
        raise ValueError("isosurface_mesh: %d voxels do not fill dims %r" % (held, tuple(dims)))
    src = _dense_source(volume, _int3(dims, "dims"))
    L, st = _lib.lib(), _stream_ptr(stream)
    nbytes = C.c_int64()
    check(L.vr_isomesh_workspace_bytes(src.args[1], C.byref(desc), C.byref(nbytes)), "vr_isomesh_workspace_bytes")
    ws = torch.empty(nbytes.value, dtype=torch.uint8, device=src.device)
    counts = (C.c_uint64 * 2)()
    check(L.vr_isomesh_count(src.args[0], src.args[1], C.byref(desc), _ptr(ws), counts, st), "vr_isomesh_count")
    V, T = int(counts[0]), int(counts[1])
    pos = torch.empty((V, 3), dtype=torch.float32, device=src.device)
    grad = torch.empty((V, 3), dtype=torch.float32, device=src.device) if gradients else None
    tri = torch.empty((T, 3), dtype=torch.int32, device=src.device)
    if V or T:
        check(L.vr_isomesh_emit(src.args[0], src.args[1], C.byref(desc), _ptr(ws), V, T, _ptr(pos),
                                _ptr(grad) if gradients else None, _ptr(tri), st), "vr_isomesh_emit")
        if stream is not None:
            ws.record_stream(stream)                   # (emit is asynchronous: the workspace outlives this call)
    return IsoMesh(pos, grad, tri)


def write_ply(path, mesh):
    """Writes an IsoMesh as a binary little-endian PLY: x y z (and nx ny nz, the unit outward normals, where the mesh has
    gradients) as float32 per vertex, then every face as a uchar 3 and three uint32 indices.  Host side."""
    pos = mesh.positions.detach().cpu().numpy().astype("<f4")
    tri = (mesh.triangles.detach().cpu().numpy().astype(np.int64) & 0xFFFFFFFF).astype("<u4")
    cols = [pos]
    head = ["ply", "format binary_little_endian 1.0", "comment volumerenderer_amd iso-surface mesh",
            "element vertex %d" % len(pos), "property float x", "property float y", "property float z"]
    if mesh.gradients is not None:
        cols.append(mesh.normals().detach().cpu().numpy().astype("<f4"))
        head += ["property float nx", "property float ny", "property float nz"]
    head += ["element face %d" % len(tri), "property list uchar uint vertex_indices", "end_header"]
    faces = np.empty(len(tri), dtype=[("n", "u1"), ("v", "<u4", (3,))])
    faces["n"], faces["v"] = 3, tri
    with open(path, "wb") as f:
        f.write(("\n".join(head) + "\n").encode("ascii"))
        f.write(np.ascontiguousarray(np.concatenate(cols, axis=1)).tobytes())
        f.write(faces.tobytes())


def read_ply(path):
    """What write_ply wrote, back as numpy arrays: (positions (V, 3) float32, normals (V, 3) float32 or None,
    triangles (T, 3) uint32).  Reads only files of write_ply's own layout."""
    with open(path, "rb") as f:
        raw = f.read()
    end = raw.index(b"end_header\n") + len(b"end_header\n")
    head = raw[:end].decode("ascii").split("\n")
    if head[:2] != ["ply", "format binary_little_endian 1.0"]:
        raise ValueError("read_ply: %s is not a binary little-endian PLY" % path)
    nv = next(int(h.split()[2]) for h in head if h.startswith("element vertex"))
    nf = next(int(h.split()[2]) for h in head if h.startswith("element face"))
    ncol = sum(1 for h in head if h.startswith("property float"))
    if ncol not in (3, 6) or len(raw) != end + nv * ncol * 4 + nf * 13:
        raise ValueError("read_ply: %s does not have write_ply's layout" % path)
    v = np.frombuffer(raw, "<f4", nv * ncol, end).reshape(nv, ncol)
    faces = np.frombuffer(raw, np.dtype([("n", "u1"), ("v", "<u4", (3,))]), nf, end + nv * ncol * 4)
    if nf and (faces["n"] != 3).any():
        raise ValueError("read_ply: %s has faces that are not triangles" % path)
    return v[:, :3].copy(), (v[:, 3:].copy() if ncol == 6 else None), faces["v"].astype(np.uint32)


def fill_volume_brick_map(ni=8, nj=8, nk=15):
    """fillVolumeBrickMap (main.cpp:599-619): brick b -> (i, j, k), i fastest."""
    m = {}
    for b in range(ni * nj * nk):
        m[b] = (b % ni, (b // ni) % nj, b // (ni * nj))
    return m


class VolumeReader:
    """volume_renderer/VolumeReader.h:28-290.  `findSourceFile(brick, timestep)` returns a
    raw brick path; `brickMap` maps brick number -> (i, j, k).  `data` is the loaded volume
    (host numpy, like the reference's std::vector), `texture` the device copy that
    transferToGPU() creates in place of the GL 3-D texture."""

    def __init__(self, brick=None, grid=None, findFileFunct=None, bMap=None):
        self.brickDims = tuple(int(v) for v in brick) if brick is not None else (0, 0, 0)
        self.findSourceFile = findFileFunct or self._undefined
        self.brickMap = bMap
        self.data = None
        self.dataDims = (0, 0, 0)
        self.texture = None     # stands in for textureId
        self._tempBrick = None

    @staticmethod
    def _undefined(brick, time):
        raise RuntimeError("\n\nERROR! findSourceFile function not defined.\n")   # VolumeReader.h:62-64

    def _load_volume_from_binary_file(self, filename):                             # VolumeReader.h:244-289
        if not os.path.exists(filename):
            return False
        expected = self.brickDims[0] * self.brickDims[1] * self.brickDims[2]
        if os.path.getsize(filename) != expected:
            raise RuntimeError("File size does not match expected dataset size!")  # :258-260
        self._tempBrick = np.fromfile(filename, dtype=np.uint8)
        return self._tempBrick.size == expected

    def LoadBrickToTexture(self, brick, timestep, dealloc, toGPU=True):            # VolumeReader.h:91-107
        ok = self._load_volume_from_binary_file(self.findSourceFile(brick, timestep))
        self.data, self._tempBrick = self._tempBrick, self.data
        self.dataDims = self.brickDims
        if ok:
            if toGPU:
                self.transferToGPU(dealloc)
        else:
            print("ERROR! Texture load failure!")
        return ok

    def transferToGPU(self, dealloc=True):                                         # VolumeReader.h:114-138
        self.texture = torch.from_numpy(self.data).cuda()
        if dealloc:
            self.data = None
            self._tempBrick = None

    def LoadBricksToTexture(self, numBricks, I, J, K, timestep, dealloc, toGPU=True):  # VolumeReader.h:151-223
        X, Y, Z = self.brickDims
        bricks = np.zeros((numBricks, Z, Y, X), np.uint8)
        ijk = np.zeros((numBricks, 3), np.int64)
        for b in range(numBricks):
            ijk[b] = self.brickMap[b]
            if not self._load_volume_from_binary_file(self.findSourceFile(b, timestep)):
                print("Load error. Brick loading terminated.")
                return False
            bricks[b] = self._tempBrick.reshape(Z, Y, X)
        # placement (VolumeReader.h:184-205) runs on the device, 64-bit indices
        vol = assemble_bricks(torch.from_numpy(bricks).cuda(), self.brickDims, ijk, (I, J, K))
        self.dataDims = (I * X, J * Y, K * Z)
        self.texture = vol
        self.data = vol.cpu().numpy()
        if toGPU and dealloc:
            self.data = None
        return True


class UnitBrick:
    """volume_renderer/UnitBrick.h:17-119.  The proxy cube is implicit in the kernel's
    ray/box set-up; Draw() is one kernel launch over the frame."""

    VERTICES = np.array([[-.5, -.5, -.5], [.5, -.5, -.5], [.5, .5, -.5], [-.5, .5, -.5],
                         [-.5, -.5, .5], [.5, -.5, .5], [.5, .5, .5], [-.5, .5, .5]], np.float32)  # UnitBrick.h:54-61

    def __init__(self):
        self._bound = False
        self.volume = None
        self.dims = None

    def Setup(self):
        self._ready = True

    def Bind(self, volume=None, dims=None):
        self._bound = True
        if volume is not None:
            self.volume, self.dims = volume, dims

    def Unbind(self):
        self._bound = False

    def Delete(self):
        self.volume = None

    def Draw(self, cam, params, out=None, stream=None):
        if not self._bound or self.volume is None:
            raise VrError(-5, "UnitBrick.Draw without Bind(volume, dims)")
        return raycast(self.volume, self.dims, cam, params, out, stream)
