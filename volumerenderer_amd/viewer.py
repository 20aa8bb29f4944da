"""Headless mirror of the reference viewer's camera / key / mouse state machine
(volume_renderer/main.cpp:30-57 start values, :462-578 do_movement / key_callback / scroll_callback /
mouse_callback / reset): events come from the caller, frames from vr_raycast.  Same fields and
arithmetic (float32) as include/vrhip/Viewer.hpp."""
import math

import numpy as np

from . import _lib
from .render import (POOL_ENTRY, assemble_bricks, build_skip_grid_pool, default_camera, default_params, lod_pool_layout,
                     raycast, raycast_pool, raycast_pool_projection, raycast_pool_tf, raycast_pool_tf2d, raycast_pool_tf_shaded,
                     raycast_projection, raycast_tf, raycast_tf2d, raycast_tf_shaded, reslice, select_lod, use_skip_grid,
                     TransferFunction2D)

KEYS = ("UP", "DOWN", "LEFT", "RIGHT", "ENTER", "0", "1", "ESCAPE")
_f = np.float32

_DENSE_FRAMES = (raycast, raycast_tf, raycast_tf_shaded, raycast_projection, raycast_tf2d)
_POOL_FRAMES = (raycast_pool, raycast_pool_tf, raycast_pool_tf_shaded, raycast_pool_projection, raycast_pool_tf2d)


def _style(mode, tf, shading, projection):
    """How draw and draw_lod_pool draw a frame: (the mode of its params, the index of its call in _DENSE_FRAMES /
    _POOL_FRAMES, the arguments that call takes between params and out)."""
    if projection is not None:
        if tf is not None or shading is not None:
            raise ValueError("a projection takes neither a transfer function nor shading")
        if mode not in (_lib.RENDER_COMPOSITE, _lib.RENDER_PROJECTION):
            raise ValueError("a projection is drawn in RENDER_PROJECTION mode, not mode %r" % (mode,))
        return _lib.RENDER_PROJECTION, 3, (projection,)
    if isinstance(tf, TransferFunction2D):       # RENDER_SHADED lit or not: its taps reach two voxels (select_lod)
        if mode not in (_lib.RENDER_COMPOSITE, _lib.RENDER_SHADED):
            raise ValueError("a two-dimensional transfer function is drawn in RENDER_SHADED mode, not mode %r" % (mode,))
        return _lib.RENDER_SHADED, 4, (tf, shading)
    if shading is not None:
        if tf is None:
            raise ValueError("shading requires a transfer function (tf=)")
        return _lib.RENDER_SHADED, 2, (tf, shading)
    return (mode, 1, (tf,)) if tf is not None else (mode, 0, ())


class HeadlessViewer:
    def __init__(self, width=1600, height=1200):
        self.width, self.height = int(width), int(height)
        self.currIsoVal = _f(40.0)            # main.cpp:52
        self.deltaTime = _f(0.0)
        self.keys = {k: False for k in KEYS}
        self.firstMouse = True
        self.shouldClose = False
        self.reset()

    def reset(self):                          # main.cpp:568-578
        self.cameraPos = np.array([0.0, 0.0, -0.75], _f)
        self.cameraFront = np.array([0.0, 0.0, 1.0], _f)
        self.cameraUp = np.array([0.0, 1.0, 0.0], _f)
        self.yaw, self.pitch, self.fov = _f(0.0), _f(0.0), _f(50.0)
        self.lastX, self.lastY = self.width / 2.0, self.height / 2.0

    def key(self, k, press):                  # main.cpp:481-506
        if k == "ESCAPE" and press: self.shouldClose = True
        if k == "ENTER" and press: self.reset()
        if k == "0" and press: self.currIsoVal = max(_f(0.0), _f(self.currIsoVal - _f(5.0)))
        if k == "1" and press: self.currIsoVal = min(_f(255.0), _f(self.currIsoVal + _f(5.0)))
        self.keys[k] = bool(press)

    def scroll(self, yoffset):                # main.cpp:508-518
        if 1.0 <= self.fov <= 50.0: self.fov = _f(self.fov - _f(yoffset))
        if self.fov <= 1.0: self.fov = _f(1.0)
        if self.fov >= 50.0: self.fov = _f(50.0)

    def mouse(self, xpos, ypos, button1):     # main.cpp:525-566
        if not button1:
            self.firstMouse = True
            return
        if self.firstMouse:
            self.lastX, self.lastY, self.firstMouse = xpos, ypos, False
        xoffset, yoffset = xpos - self.lastX, self.lastY - ypos
        self.lastX, self.lastY = xpos, ypos
        self.pitch = _f(self.pitch + _f(yoffset)); self.yaw = _f(self.yaw + _f(xoffset))
        self.pitch = min(_f(89.0), max(_f(-89.0), self.pitch))
        d2r = _f(0.01745329251994329576923690768489)
        p, y = _f(self.pitch * d2r), _f(self.yaw * d2r)
        f = np.array([_f(math.cos(p)) * _f(math.cos(y)), _f(math.sin(p)), _f(math.sin(y))], _f)   # (sic) z without cos(pitch)
        n = _f(np.sqrt(_f(f[0] * f[0] + f[1] * f[1] + f[2] * f[2])))
        self.cameraFront = (f / n).astype(_f) if n > 0 else f

    def advance(self, dt):                    # main.cpp:382, :462-478
        self.deltaTime = _f(dt)
        sp = _f(_f(2.5) * self.deltaTime)
        r = np.cross(self.cameraFront, self.cameraUp).astype(_f)
        n = _f(np.sqrt(_f(np.dot(r, r))))
        if n > 0: r = (r / n).astype(_f)
        if self.keys["UP"]: self.cameraPos = (self.cameraPos + sp * self.cameraFront).astype(_f)
        if self.keys["DOWN"]: self.cameraPos = (self.cameraPos - sp * self.cameraFront).astype(_f)
        if self.keys["LEFT"]: self.cameraPos = (self.cameraPos - r * sp).astype(_f)
        if self.keys["RIGHT"]: self.cameraPos = (self.cameraPos + r * sp).astype(_f)

    def camera(self):
        cam = default_camera()
        cam.pos[:] = tuple(float(v) for v in self.cameraPos)
        cam.front[:] = tuple(float(v) for v in self.cameraFront)
        cam.up[:] = tuple(float(v) for v in self.cameraUp)
        cam.fov_deg = float(self.fov)
        return cam

    def draw(self, volume, dims, brick_dims=(256, 256, 128), mode=_lib.RENDER_COMPOSITE, out=None, tf=None, shading=None,
             projection=None):
        """One frame of `volume`: raycast, or raycast_tf through the TransferFunction `tf` (composite mode only).
        shading: a Shading (requires tf): the frame is drawn with raycast_tf_shaded in RENDER_SHADED mode.
        projection: a Projection (neither tf nor shading): drawn with raycast_projection in RENDER_PROJECTION mode.
        tf may be a TransferFunction2D, with or without shading: drawn with raycast_tf2d in RENDER_SHADED mode."""
        mode, call, extra = _style(mode, tf, shading, projection)
        P = default_params(self.width, self.height, brick_dims, mode, float(self.currIsoVal) / 255.0)
        return _DENSE_FRAMES[call](volume, dims, self.camera(), P, *extra, out)

    def draw_lod(self, bset, brick_ijk, grid, pixel_tolerance=1.0, mode=_lib.RENDER_COMPOSITE, out=None):
        """One frame from a BrickSet: select_lod for this frame's camera, decode_lod, assemble, ray-cast.  The bricks
        are decoded into a buffer this viewer owns and kept across frames: a brick culled in this frame keeps (and
        shows nowhere) whatever an earlier frame decoded into it.  Returns (frame, cuts)."""
        import torch
        bd = tuple(int(q) for q in bset.dims)
        g = tuple(int(q) for q in grid)
        info = bset.info(0)
        P = default_params(self.width, self.height, bd, mode, float(self.currIsoVal) / 255.0)
        cam = self.camera()
        cuts = select_lod(cam, P, bd, brick_ijk, g, info["orig_tree_depth"], info["max_tree_depth"], pixel_tolerance)
        n = bset.num_bricks * bset.voxels_per_brick
        if getattr(self, "_lodBricks", None) is None or self._lodBricks.numel() != n:
            self._lodBricks = torch.zeros(n, dtype=torch.uint8, device="cuda")
            self._lodVol = None
        bset.decode_lod(cuts, out=self._lodBricks)
        self._lodVol = assemble_bricks(self._lodBricks, bd, brick_ijk, g, out=self._lodVol)
        vol = self._lodVol
        dims = (g[0] * bd[0], g[1] * bd[1], g[2] * bd[2])
        return raycast(vol, dims, cam, P, out), cuts

    def draw_lod_pool(self, bset, brick_ijk, grid, pixel_tolerance=1.0, mode=_lib.RENDER_COMPOSITE, skip_cell=0, out=None,
                      tf=None, shading=None, projection=None):
        """draw_lod's frame (bit for bit) from a pool: select_lod, decode_lod_pool, raycast_pool -- no brick buffer and no
        assembled volume; each brick is stored at the resolution of its cut.  The pool is kept across frames and grows
        only when a frame needs more.  skip_cell > 0: a skip grid of that cell size is built from the pool for the frame.
        Power-of-two brick extents only.  tf: a TransferFunction, drawn with raycast_pool_tf; shading (requires tf): a
        Shading, drawn with raycast_pool_tf_shaded in RENDER_SHADED mode (select_lod included); projection (neither tf nor
        shading): a Projection, drawn with raycast_pool_projection in RENDER_PROJECTION mode.  A TransferFunction2D as tf, with
        or without shading: raycast_pool_tf2d in RENDER_SHADED mode (select_lod included).  Returns (frame, cuts)."""
        import torch
        mode, call, extra = _style(mode, tf, shading, projection)
        bd = tuple(int(q) for q in bset.dims)
        g = tuple(int(q) for q in grid)
        info = bset.info(0)
        P = default_params(self.width, self.height, bd, mode, float(self.currIsoVal) / 255.0)
        cam = self.camera()
        cuts = select_lod(cam, P, bd, brick_ijk, g, info["orig_tree_depth"], info["max_tree_depth"], pixel_tolerance)
        _, need = lod_pool_layout(bd, brick_ijk, g, cuts, info["orig_tree_depth"], info["max_tree_depth"])
        cells = g[0] * g[1] * g[2]
        if getattr(self, "_pool", None) is None or self._pool.numel() < max(need, 1):
            self._pool = None
            self._pool = torch.empty(max(need, 1), dtype=torch.uint8, device="cuda")
        if getattr(self, "_poolTable", None) is None or self._poolTable.numel() != cells * POOL_ENTRY.itemsize:
            self._poolTable = torch.empty(cells * POOL_ENTRY.itemsize, dtype=torch.uint8, device="cuda")
        bset.decode_lod_pool(cuts, brick_ijk, g, pool=self._pool, table=self._poolTable)
        if skip_cell > 0:
            sg = build_skip_grid_pool(self._pool, self._poolTable, bd, g, skip_cell)
            use_skip_grid(P, sg, skip_cell)
        return _POOL_FRAMES[call](self._pool, self._poolTable, bd, g, cam, P, *extra, out), cuts

    def draw_slice(self, volume, dims, plane, projection, out=None):
        """The slice `plane` (a SlicePlane) of `volume` through the Projection `projection`: reslice.  A slice has its
        own geometry: the viewer's camera and frame size play no part."""
        return reslice(volume, dims, plane, projection, out)

    @staticmethod
    def dump_ppm(path, rgba):
        """rgba: (H, W, 4) float array/tensor in [0,1] -> binary PPM (8-bit, like the framebuffer)."""
        a = rgba.detach().cpu().numpy() if hasattr(rgba, "detach") else np.asarray(rgba)
        h, w = a.shape[:2]
        px = np.rint(255.0 * np.clip(a[..., :3], 0.0, 1.0)).astype(np.uint8)
        with open(path, "wb") as f:
            f.write(b"P6\n%d %d\n255\n" % (w, h))
            f.write(px.tobytes())
