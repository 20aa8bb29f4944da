"""Host-side mirror of the reference's codec classes over the C ABI (include/vrhip.h).

  BrickSet       a batch of per-brick trees (one kd-tree per brick, batched launches)
  VolumeKdtree   same names / argument meaning as the reference class
                 (volume_renderer/VolumeKdtree_recover.h:51-175), a BrickSet of 1
  MidRangeTree   volume_renderer/MidRangeTree.h:51-271 (second stream + 4-bit packing)

PyTorch appears here only as plumbing: device buffers (torch.uint8 CUDA tensors),
streams.  All compute is in libvrhip.so; nothing here falls back to the CPU.
"""
import ctypes as C
import os

import numpy as np
import torch

from . import _lib
from ._lib import VrError, check


def _stream_ptr(stream=None):
    s = stream if stream is not None else torch.cuda.current_stream()
    return C.c_void_p(s.cuda_stream)


def _as_dev_u8(x):
    """numpy / torch, host or device -> contiguous CUDA uint8 tensor (the boundary
    hands over host buffers in the reference: std::vector<byte>&)."""
    if isinstance(x, np.ndarray):
        x = torch.from_numpy(np.ascontiguousarray(x, dtype=np.uint8))
    if not isinstance(x, torch.Tensor) or x.dtype != torch.uint8:
        raise TypeError("expected a uint8 numpy array or torch tensor")
    if not x.is_cuda:
        x = x.cuda()
    return x.contiguous()


class BrickSet:
    def __init__(self, num_bricks, dims, tolerance=6, max_epochs=5, variant=_lib.VARIANT_RECOVER, _handle=None):
        self._L = _lib.lib()
        self._h = C.c_void_p()
        if _handle is not None:
            self._h = _handle
        else:
            d = (C.c_int64 * 3)(*[int(v) for v in dims])
            check(self._L.vr_brickset_create(C.byref(self._h), int(num_bricks), d, int(tolerance), int(max_epochs),
                                             int(variant)), "vr_brickset_create")
        self.num_bricks = int(num_bricks)
        self.dims = tuple(int(v) for v in dims)
        self.voxels_per_brick = self.dims[0] * self.dims[1] * self.dims[2]
        self._keep = None

    def __del__(self):
        try:
            if self._h:
                self._L.vr_brickset_destroy(self._h)
                self._h = None
        except Exception:
            pass

    def set_error_tolerance(self, tol):
        check(self._L.vr_brickset_set_error_tolerance(self._h, int(tol)), "setErrorTolerance")

    def set_max_epochs(self, e):
        check(self._L.vr_brickset_set_max_epochs(self._h, int(e)), "setMaxEpochs")

    def set_compaction(self, on_build=True):
        """build() ends with the reference's contiguous stream (default) or leaves it to the first get_tree / save."""
        check(self._L.vr_brickset_set_compaction(self._h, 1 if on_build else 0), "vr_brickset_set_compaction")

    def set_switch(self, name, value=1):
        """Debugging switch of this set (vr_brickset_set_switch): which kernel serves the next calls.

        Names: "decode_walk", "decode_fine_v1", "decode_quad", "no_skip_blocks", "no_uniform_blocks",
        "no_uniform_decode", "est_exact_bounds", "est_old_schedule", "pyramid_boxes", "index_per_block" (include/vrhip.h)."""
        check(self._L.vr_brickset_set_switch(self._h, name.encode(), int(value)), "vr_brickset_set_switch(%s)" % name)

    def build(self, voxels, stream=None):
        v = _as_dev_u8(voxels)
        if v.numel() != self.num_bricks * self.voxels_per_brick:
            raise ValueError("voxel buffer has %d bytes, expected %d" % (v.numel(), self.num_bricks * self.voxels_per_brick))
        self._keep = v  # the launches are asynchronous: keep the input alive
        check(self._L.vr_brickset_build(self._h, C.c_void_p(v.data_ptr()), _stream_ptr(stream)), "vr_brickset_build")
        return self

    def info(self, brick=0):
        ti = _lib.TreeInfo()
        check(self._L.vr_brickset_info(self._h, int(brick), C.byref(ti)), "vr_brickset_info")
        return {k: getattr(ti, k) for k, _ in ti._fields_}

    def tree(self, brick=0):
        n = self.info(brick)["tree_bytes"]
        out = np.empty(n, np.uint8)
        check(self._L.vr_brickset_get_tree(self._h, int(brick), out.ctypes.data, n), "vr_brickset_get_tree")
        return out

    def distance_map(self, brick=0):
        n = self.info(brick)["max_tree_depth"] + 1
        out = np.empty(n, np.uint8)
        check(self._L.vr_brickset_get_distance_map(self._h, int(brick), out.ctypes.data, n), "get_distance_map")
        return out

    def tree_range(self, brick=0):
        n = self.info(brick)["tree_bytes"]
        out = np.empty(n, np.uint8)
        check(self._L.vr_brickset_get_tree_range(self._h, int(brick), out.ctypes.data, n), "get_tree_range")
        return out

    def distance_map_range(self, brick=0):
        n = self.info(brick)["max_tree_depth"] + 1
        out = np.empty(n, np.uint8)
        check(self._L.vr_brickset_get_distance_map_range(self._h, int(brick), out.ctypes.data, n), "get_distance_map_range")
        return out

    def packed4(self, brick=0):
        n = C.c_int64()
        check(self._L.vr_brickset_get_packed4(self._h, int(brick), None, 0, C.byref(n)), "get_packed4")
        out = np.empty(n.value, np.uint8)
        check(self._L.vr_brickset_get_packed4(self._h, int(brick), out.ctypes.data, n.value, C.byref(n)), "get_packed4")
        return out

    def decode(self, out=None, cut_depth=-1, stream=None):
        if out is None:
            out = torch.empty(self.num_bricks * self.voxels_per_brick, dtype=torch.uint8, device="cuda")
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                and out.numel() == self.num_bricks * self.voxels_per_brick):
            raise ValueError("bad output buffer")
        check(self._L.vr_brickset_decode(self._h, int(cut_depth), C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
              "vr_brickset_decode")
        return out

    def decode_lod(self, cuts, out=None, stream=None):
        """Per-brick progressive decode: cuts[b] = -1 leaves brick b's bytes of `out` untouched, 0 .. max_tree_depth
        decodes it exactly as decode(cut_depth=cuts[b]) would (vr_brickset_decode_lod)."""
        c = np.ascontiguousarray(np.asarray(cuts).reshape(-1), dtype=np.int32)
        if c.size != self.num_bricks:
            raise ValueError("decode_lod: %d cuts for %d bricks" % (c.size, self.num_bricks))
        if out is None:
            out = torch.empty(self.num_bricks * self.voxels_per_brick, dtype=torch.uint8, device="cuda")
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                and out.numel() == self.num_bricks * self.voxels_per_brick):
            raise ValueError("bad output buffer")
        check(self._L.vr_brickset_decode_lod(self._h, c.ctypes.data_as(C.POINTER(C.c_int32)), C.c_void_p(out.data_ptr()),
                                             _stream_ptr(stream)), "vr_brickset_decode_lod")
        return out

    def decode_lod_pool(self, cuts, brick_ijk, grid, pool=None, table=None, stream=None):
        """decode_lod into a pool that stores each brick at the resolution of its cut (vr_brickset_decode_lod_pool;
        layout: render.lod_pool_layout).  pool: a CUDA uint8 tensor of at least the layout's bytes (None: allocated);
        table: a CUDA uint8 tensor of 16 bytes per grid cell that receives the layout (None: allocated).  Power-of-two
        brick extents only.  Returns (pool, table)."""
        from .render import POOL_ENTRY, _check_buf, lod_pool_layout
        c = np.ascontiguousarray(np.asarray(cuts).reshape(-1), dtype=np.int32)
        if c.size != self.num_bricks:
            raise ValueError("decode_lod_pool: %d cuts for %d bricks" % (c.size, self.num_bricks))
        ijk = np.ascontiguousarray(brick_ijk, np.int64).reshape(-1, 3)
        if ijk.shape[0] != self.num_bricks:
            raise ValueError("decode_lod_pool: %d brick cells for %d bricks" % (ijk.shape[0], self.num_bricks))
        g = (C.c_int64 * 3)(*[int(q) for q in grid])
        dev = torch.device("cuda", torch.cuda.current_device())
        if pool is None or table is None:
            info = self.info(0)
            _, need = lod_pool_layout(self.dims, ijk, grid, c, info["orig_tree_depth"], info["max_tree_depth"])
            if pool is None:
                pool = torch.empty(max(need, 1), dtype=torch.uint8, device=dev)
            if table is None:
                table = torch.empty(g[0] * g[1] * g[2] * POOL_ENTRY.itemsize, dtype=torch.uint8, device=dev)
        if not isinstance(pool, torch.Tensor) or pool.numel() == 0:
            raise ValueError("pool must be a non-empty torch tensor")
        _check_buf(pool, "pool", torch.uint8, pool.numel(), pool.device)
        _check_buf(table, "table", torch.uint8, g[0] * g[1] * g[2] * POOL_ENTRY.itemsize, pool.device)
        check(self._L.vr_brickset_decode_lod_pool(self._h, c.ctypes.data_as(C.POINTER(C.c_int32)),
                                                  ijk.ctypes.data_as(C.POINTER(C.c_int64)), g, C.c_void_p(pool.data_ptr()),
                                                  pool.numel(), C.c_void_p(table.data_ptr()), _stream_ptr(stream)),
              "vr_brickset_decode_lod_pool")
        return pool, table

    def error_table(self, reference=None, cuts=None, scratch=None, stream=None):
        """What every cut of every brick costs in accuracy (vr_brickset_error_table; the rule is in vrhip.h).
        reference: the voxels to compare with, in build()'s layout -- the original volume or any decode; None = the
        set's own full-depth decode, against which the last row (cut max_tree_depth) is all zero.  cuts: (cut_lo, cut_hi),
        inclusive; None = every cut 0 .. max_tree_depth.  scratch: a CUDA uint8 tensor of num_bricks * voxels_per_brick
        bytes for the decodes (None: allocated); it is left with the decode at cut_hi.  Returns a BRICK_ERROR numpy
        array of shape (cut_hi - cut_lo + 1, num_bricks); the call synchronises the stream."""
        n = self.num_bricks * self.voxels_per_brick
        lo, hi = (0, self.info(0)["max_tree_depth"]) if cuts is None else (int(cuts[0]), int(cuts[1]))
        if hi < lo:
            raise ValueError("error_table: cuts (%d, %d)" % (lo, hi))
        ref = self.decode(stream=stream) if reference is None else _as_dev_u8(reference).reshape(-1)
        if ref.numel() != n:
            raise ValueError("reference has %d bytes, expected %d" % (ref.numel(), n))
        if scratch is None:
            scratch = torch.empty(n, dtype=torch.uint8, device=ref.device)
        if not (isinstance(scratch, torch.Tensor) and scratch.is_cuda and scratch.dtype == torch.uint8
                and scratch.is_contiguous() and scratch.numel() == n):
            raise ValueError("bad scratch buffer")
        table = np.zeros((hi - lo + 1, self.num_bricks), BRICK_ERROR)
        check(self._L.vr_brickset_error_table(self._h, C.c_void_p(ref.data_ptr()), C.c_void_p(scratch.data_ptr()), lo, hi,
                                              C.c_void_p(table.ctypes.data), _stream_ptr(stream)), "vr_brickset_error_table")
        return table

    def decode_range(self, out=None, cut_depth=-1, stream=None):
        """MidRangeTree sets: the half-range stream decoded like the mid stream (vr_brickset_decode_range)."""
        if out is None:
            out = torch.empty(self.num_bricks * self.voxels_per_brick, dtype=torch.uint8, device="cuda")
        if not (out.is_cuda and out.dtype == torch.uint8 and out.is_contiguous()
                and out.numel() == self.num_bricks * self.voxels_per_brick):
            raise ValueError("bad output buffer")
        check(self._L.vr_brickset_decode_range(self._h, int(cut_depth), C.c_void_p(out.data_ptr()), _stream_ptr(stream)),
              "vr_brickset_decode_range")
        return out

    def set_tree(self, brick, tree_bytes, num_active_nodes, distance_map):
        t = np.ascontiguousarray(tree_bytes, np.uint8)
        d = np.ascontiguousarray(distance_map, np.uint8)
        check(self._L.vr_brickset_set_tree(self._h, int(brick), t.ctypes.data, t.size, int(num_active_nodes),
                                           d.ctypes.data, d.size), "vr_brickset_set_tree")

    def set_trees(self, bricks, trees, num_active, dmaps, tables=None, stream=None):
        """Install many stored streams at once; the decode index is rebuilt on the GPU (vr_brickset_set_trees).
        bricks: brick numbers; trees, num_active, dmaps: per brick the packed stream (uint8), its token count and its
        distance map; tables: per brick (block_off, top_val) as stream_block_table returns them, or None to have them
        made on the host (slow).  Synchronises `stream` once."""
        n = len(bricks)
        if not (len(trees) == n and len(num_active) == n and len(dmaps) == n and (tables is None or len(tables) == n)):
            raise ValueError("set_trees: one tree, token count, map and table per brick")
        keep = []
        descs = (_lib.TreeDesc * n)()
        for i in range(n):
            t = np.ascontiguousarray(trees[i], np.uint8)
            d = np.ascontiguousarray(dmaps[i], np.uint8)
            keep += [t, d]
            descs[i].tree, descs[i].tree_bytes, descs[i].num_active = t.ctypes.data, t.size, int(num_active[i])
            descs[i].distance_map, descs[i].map_len = d.ctypes.data, d.size
            if tables is not None and tables[i] is not None:
                off = np.ascontiguousarray(tables[i][0], np.uint32)
                top = np.ascontiguousarray(tables[i][1], np.uint8)
                keep += [off, top]
                descs[i].block_off, descs[i].top_val = off.ctypes.data, top.ctypes.data
        b = np.ascontiguousarray(np.asarray(bricks).reshape(-1), dtype=np.int32)
        check(self._L.vr_brickset_set_trees(self._h, n, b.ctypes.data_as(C.POINTER(C.c_int32)), descs, _stream_ptr(stream)),
              "vr_brickset_set_trees")

    def save_set(self, path):
        """The whole set (one timestep) as one archive file (vr_brickset_save_set; layout in include/vrhip.h)."""
        check(self._L.vr_brickset_save_set(self._h, os.fsencode(path)), "vr_brickset_save_set")

    @classmethod
    def open_set(cls, path, stream=None):
        L = _lib.lib()
        h = C.c_void_p()
        check(L.vr_brickset_open_set(C.byref(h), os.fsencode(path), _stream_ptr(stream)), "vr_brickset_open_set")
        with open(path, "rb") as f:
            head = np.frombuffer(f.read(64), np.uint8)
        dims = head[16:40].view("<i8")
        return cls(int(head[40:44].view("<i4")[0]), tuple(int(v) for v in dims), _handle=h)

    def load_set(self, source, nbytes=None, stream=None):
        """The next timestep into this set: an archive file's path, or a uint8 host tensor / array that holds a file's
        bytes (16-byte aligned; pinned memory makes the copies asynchronous; nbytes: the file's size if the buffer is
        longer).  Synchronises `stream` once."""
        if isinstance(source, (str, bytes, os.PathLike)):
            check(self._L.vr_brickset_load_set(self._h, os.fsencode(source), _stream_ptr(stream)), "vr_brickset_load_set")
            return self
        if isinstance(source, torch.Tensor):
            if source.is_cuda or source.dtype != torch.uint8 or not source.is_contiguous():
                raise TypeError("load_set: a contiguous uint8 host tensor")
            ptr, size = source.data_ptr(), source.numel()
        else:
            source = np.ascontiguousarray(source, np.uint8)
            ptr, size = source.ctypes.data, source.size
        size = size if nbytes is None else int(nbytes)
        check(self._L.vr_brickset_load_set_memory(self._h, C.c_void_p(ptr), size, _stream_ptr(stream)),
              "vr_brickset_load_set_memory")
        return self

    def save(self, path, brick=0):
        check(self._L.vr_brickset_save(self._h, int(brick), os.fsencode(path)), "vr_brickset_save")

    @classmethod
    def open(cls, path, variant=_lib.VARIANT_RECOVER):
        L = _lib.lib()
        h = C.c_void_p()
        check(L.vr_brickset_open_variant(C.byref(h), os.fsencode(path), int(variant)), "vr_brickset_open")
        ti = _lib.TreeInfo()
        check(L.vr_brickset_info(h, 0, C.byref(ti)), "vr_brickset_info")
        return cls(1, (ti.X, ti.Y, ti.Z), _handle=h)

    def set_concurrency(self, level_loop_streams):
        """Brick ranges whose level loops run side by side inside one build (1 = off, 2 = default, <= 4): see vrhip.h."""
        check(self._L.vr_brickset_set_concurrency(self._h, int(level_loop_streams)), "set_concurrency")
        return self

    def last_timings(self):
        ms = (C.c_float * 5)()
        check(self._L.vr_brickset_last_timings(self._h, ms), "last_timings")
        return dict(zip(("BUILD", "COMPRESS", "PRUNE", "CONVERT", "DECODE"), [float(v) for v in ms]))


def stream_block_table(dims, tree, num_active, dmap):
    """(block_off uint32[nBlk], top_val uint8[2 nBlk]) of one packed stream: the seek table vr_brickset_set_trees and
    the archive take (vr_stream_block_table; host only, no device needed).  VrError(VR_ERR_FORMAT) for a stream the
    grammar does not produce."""
    d = (C.c_int64 * 3)(*[int(v) for v in dims])
    depth = sum(int(v).bit_length() - 1 for v in dims)
    n_blk = 1 << max(depth - 12, 0)
    t = np.ascontiguousarray(tree, np.uint8)
    m = np.ascontiguousarray(dmap, np.uint8)
    off, top = np.empty(n_blk, np.uint32), np.empty(2 * n_blk, np.uint8)
    check(_lib.lib().vr_stream_block_table(d, t.ctypes.data, t.size, int(num_active), m.ctypes.data, m.size,
                                           off.ctypes.data, top.ctypes.data), "vr_stream_block_table")
    return off, top


def measure_error(decoded, original, stream=None):
    """measureMaxError / measureMeanError (R.cpp:386-401) with the original passed explicitly."""
    a, b = _as_dev_u8(decoded), _as_dev_u8(original)
    mx, mean = C.c_int32(), C.c_double()
    check(_lib.lib().vr_measure_error(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.numel(),
                                      C.byref(mx), C.byref(mean), _stream_ptr(stream)), "vr_measure_error")
    return mx.value, mean.value


# vr_brick_error as numpy
BRICK_ERROR = np.dtype([("sum_abs", "<u8"), ("sum_sq", "<u8"), ("max_abs", "<u4"), ("num_diff", "<u4")])


def measure_error_bricks(decoded, reference, num_bricks, stream=None):
    """Per-brick error of two buffers of num_bricks equal bricks (vr_measure_error_bricks): a BRICK_ERROR numpy array of
    num_bricks entries, every field an exact integer.  Either buffer may start at any byte."""
    a, b = _as_dev_u8(decoded), _as_dev_u8(reference)
    nb = int(num_bricks)
    if nb < 1 or a.numel() != b.numel() or a.numel() == 0 or a.numel() % nb:
        raise ValueError("measure_error_bricks: %d and %d bytes for %d bricks" % (a.numel(), b.numel(), nb))
    out = np.zeros(nb, BRICK_ERROR)
    check(_lib.lib().vr_measure_error_bricks(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), nb, a.numel() // nb,
                                             C.c_void_p(out.ctypes.data), _stream_ptr(stream)), "vr_measure_error_bricks")
    return out


def query_error(decoded, original, stream=None):
    """queryError (R.cpp:404-411)."""
    a, b = _as_dev_u8(decoded), _as_dev_u8(original)
    out = torch.empty_like(a)
    check(_lib.lib().vr_query_error(C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()), a.numel(),
                                    C.c_void_p(out.data_ptr()), _stream_ptr(stream)), "vr_query_error")
    return out


class VolumeKdtree:
    """volume_renderer/VolumeKdtree_recover.h:51-175 -- same method names and argument meaning.

    Differences forced by the defects listed in SURVEY.md Appendix C: the input is
    not destroyed by build() (C-7: the error helpers need it); levelCut() below
    maxTreeDepth is a defined progressive cut rather than the reference's broken walk (C-4)."""
    _variant = _lib.VARIANT_RECOVER

    def __init__(self, inData=None, x=0, y=0, z=0):
        self.tolerance = 6      # R.h:92-93
        self.maxEpochs = 5
        self.X, self.Y, self.Z = int(x), int(y), int(z)
        self._data = _as_dev_u8(inData).reshape(-1) if inData is not None else None
        self._bs = None
        self._output = None

    def setErrorTolerance(self, errorTolerance):   # R.cpp:9-11
        self.tolerance = int(errorTolerance)

    def setMaxEpochs(self, epochs):                # R.cpp:13-15
        self.maxEpochs = int(epochs)

    def build(self, useThreads=True):              # R.cpp:17-140 (useThreads is meaningless on the GPU)
        if self._data is None:
            raise VrError(-5, "build() without data")
        self._bs = BrickSet(1, (self.X, self.Y, self.Z), self.tolerance, self.maxEpochs, self._variant)
        self._bs.build(self._data)
        return self

    def _need(self):
        if self._bs is None:
            raise VrError(-5, "no tree")
        return self._bs

    # public data members of the reference class
    @property
    def tree(self): return self._need().tree(0)
    @property
    def distanceMap(self): return self._need().distance_map(0)
    @property
    def numActiveNodes(self): return self._need().info(0)["num_active_nodes"]
    @property
    def origTreeDepth(self): return self._need().info(0)["orig_tree_depth"]
    @property
    def maxTreeDepth(self): return self._need().info(0)["max_tree_depth"]

    def levelCut(self, cutDepth=None, outData=None):   # R.cpp:726-835
        bs = self._need()
        self._output = bs.decode(outData, -1 if cutDepth is None else int(cutDepth))
        return self._output

    def measureMaxError(self):                     # R.cpp:386-392
        return measure_error(self._output, self._data)[0]

    def measureMeanError(self):                    # R.cpp:394-401
        return measure_error(self._output, self._data)[1]

    def queryError(self):                          # R.cpp:404-411
        return query_error(self._output, self._data)

    def save(self, filename):                      # R.cpp:521-552
        self._need().save(filename, 0)

    def open(self, filename):                      # R.cpp:554-594 / M.cpp:787-833
        self._bs = BrickSet.open(filename, self._variant)
        self.X, self.Y, self.Z = self._bs.dims
        return self


class MidRangeTree(VolumeKdtree):
    """volume_renderer/MidRangeTree.h:51-271: VolumeKdtree + half-range stream."""
    _variant = _lib.VARIANT_MIDRANGE

    @property
    def tree_range(self): return self._need().tree_range(0)
    @property
    def distanceMap_range(self): return self._need().distance_map_range(0)

    def convertToByteArray(self):                  # M.cpp:1095-1128
        return self._need().packed4(0)

    def levelCutRange(self, cutDepth=None, outData=None):
        """New (the reference never decodes tree_range): the half range per voxel at a cut depth."""
        return self._need().decode_range(outData, -1 if cutDepth is None else int(cutDepth))


class HashedKdtree(VolumeKdtree):
    """volume_renderer/HashedKdtree.h:26-227 -- the interface only; PARITY UNPINNED.

    The reference class cannot be run (heap overflow on the first level, HashedKdtree.cpp:138; collision handling
    seeded from std::random_device, :473), so there is nothing to compare with.  Callers get the same methods and
    members over the VolumeKdtree path with the class's own tolerance (4, HashedKdtree.h:79); the hash-table members
    exist and stay empty."""

    def __init__(self, inData=None, x=0, y=0, z=0):
        super().__init__(inData, x, y, z)
        self.tolerance = 4
        self.numCollisions = 0
        self.hashMask = 0
        self.queryDepth = 0

    @property
    def treeData(self): return self.tree
    @property
    def treeDepth(self): return self.maxTreeDepth

    def levelCut(self, cutDepth=None, outData=None):   # HashedKdtree.h:113
        self.queryDepth = self.treeDepth if cutDepth is None else int(cutDepth)
        return super().levelCut(cutDepth, outData)
