"""Multi-GPU host logic: one process per GPU over torch.distributed (backend "nccl" = RCCL
over xGMI on ROCm).

  * The codec shards with NO data-path collective: bricks (or whole timesteps) are dealt
    to ranks, every rank builds / decodes its own trees.
  * Rendering has one real exchange step: sort-last compositing of the per-rank partial
    (c, tau) images.  Direct send: the frame is cut into R row tiles, one grouped send/recv moves
    tile t of every rank's partial image to rank t (1080p: 33 MB per partial, 4.1 MB per
    peer at R = 8 -- latency-, not bandwidth-bound on the 7 x ~153 GB/s xGMI links), rank
    t composites its R partials per pixel in view order (vr_composite_slabs), and the
    finished tiles are gathered on rank 0.  A plain all-reduce cannot be used: "over" is
    associative but not commutative.

The combine step is injectable so that the exchange pattern can be exercised on CPU tensors
with the gloo backend (tests/test_distributed_cpu.py); on the GPU it is the C-ABI kernel.
"""
import ctypes as C

import torch
import torch.distributed as dist


def shard_range(n_items, rank, world):
    """Contiguous block partition [lo, hi) of n_items over world ranks (first ranks get the remainder)."""
    q, r = divmod(n_items, world)
    lo = rank * q + min(rank, r)
    return lo, lo + q + (1 if rank < r else 0)


def shard_bricks_by_slab(grid, rank, world, axis=2):
    """Bricks of an I x J x K grid owned by `rank` when the grid is cut into `world` slabs along
    `axis` (brick numbering of fillVolumeBrickMap, main.cpp:599-619: i fastest).  Returns
    (brick ids, (slab_lo, slab_hi))."""
    I, J, K = grid
    lo, hi = shard_range(grid[axis], rank, world)
    ids = []
    for b in range(I * J * K):
        ijk = (b % I, (b // I) % J, b // (I * J))
        if lo <= ijk[axis] < hi:
            ids.append(b)
    return ids, (lo, hi)


def tile_rows(height, world):
    """Row range of every rank's image tile."""
    return [shard_range(height, r, world) for r in range(world)]


def _gpu_slabs(fn, parts, *args):
    """The slab call `fn` on parts = [slabs][pixels][4]; args: what it takes between the pixel count and the output."""
    from . import _lib
    from .codec import _stream_ptr
    from ._lib import check
    out = torch.empty((parts.shape[1], 4), dtype=torch.float32, device=parts.device)
    check(getattr(_lib.lib(), fn)(C.c_void_p(parts.data_ptr()), parts.shape[0], parts.shape[1], *args,
                                  C.c_void_p(out.data_ptr()), _stream_ptr()), fn)
    return out


def _gpu_combine(parts, first_pixel, axis, cam, params):
    return _gpu_slabs("vr_composite_slabs", parts, int(first_pixel), int(axis), C.byref(cam), C.byref(params))


def _gpu_combine_tf(parts, first_pixel, axis, cam, params, tf):
    from .render import background_desc
    desc = background_desc(tf)
    return _gpu_slabs("vr_composite_slabs_tf", parts, int(first_pixel), int(axis), C.byref(cam), C.byref(params), C.byref(desc))


def _gpu_combine_proj(parts, proj):
    desc = proj.desc()
    return _gpu_slabs("vr_composite_slabs_proj", parts, C.byref(desc))


def _slab_cut(who, dims, axis, rank, world, halo):
    """The cut slab_params and slab_plane share: (dims, box_min, box_max, vol_origin, local_dims, (a0, a1)) of rank
    `rank`'s slab; the last rank's box_max is 2.0 (it owns the far face).  ValueError in the name of `who`."""
    dims = [int(q) for q in dims]
    if len(dims) != 3 or axis not in (0, 1, 2) or not 0 <= rank < world or halo < 0 or world > dims[axis]:
        raise ValueError("%s: axis %r, rank %r of %r, halo %r, extents %r" % (who, axis, rank, world, halo, dims))
    n = dims[axis]
    lo, hi = shard_range(n, rank, world)
    a0, a1 = max(0, lo - halo), min(n, hi + halo)
    bmin, bmax, org, local = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 0, 0], list(dims)
    bmin[axis] = lo / n
    bmax[axis] = hi / n if rank < world - 1 else 2.0
    org[axis] = a0
    local[axis] = a1 - a0
    return dims, bmin, bmax, org, tuple(local), (a0, a1)


def slab_params(params, dims, axis, rank, world, halo):
    """Rank `rank`'s slab when a volume of `dims` = (X, Y, Z) voxels is cut into `world` slabs along `axis`, stored with
    `halo` voxel layers beyond each cut (1 for the grey and the unlit marches and the projections, 2 for the lit one and
    for a two-dimensional transfer function, lit or not; vrhip.h).  Returns
    (P, local_dims, (a0, a1)): P = a copy of `params` with box_min / box_max (the last rank's box_max is 2.0: it owns
    the far face), vol_origin and global_dims set, local_dims the extents of the voxels [a0, a1) along `axis` that the
    rank has to hold."""
    dims, bmin, bmax, org, local, held = _slab_cut("slab_params", dims, axis, rank, world, halo)
    P = type(params).from_buffer_copy(params)
    if hasattr(params, "_keep_grid"):
        P._keep_grid = params._keep_grid
    P.box_min[:] = bmin
    P.box_max[:] = bmax
    P.vol_origin[:] = org
    P.global_dims[:] = dims
    return P, local, held


def slab_plane(plane, dims, axis, rank, world, halo=1):
    """slab_params' twin for a slice: rank `rank`'s copy of the SlicePlane `plane` when a volume of `dims` voxels is cut
    into `world` slabs along `axis`, stored with `halo` voxel layers beyond each cut (1, for both filters; vrhip.h).
    Returns (plane, local_dims, (a0, a1)) with box_min / box_max (the last rank's box_max is 2.0), vol_origin and
    global_dims set.  The partials of reslice_partial go through composite_sort_last_proj unchanged."""
    import copy
    dims, bmin, bmax, org, local, held = _slab_cut("slab_plane", dims, axis, rank, world, halo)
    p = copy.copy(plane)
    p.box_min, p.box_max, p.vol_origin, p.global_dims = tuple(bmin), tuple(bmax), tuple(org), tuple(dims)
    return p, local, held


def slab_voxels(dims, axis, rank, world, halo=1):
    """slab_params' twin for the voxel-space calls (render.histogram2d): rank `rank`'s slab when a volume of `dims`
    voxels is cut into `world` slabs along `axis`, stored with `halo` voxel layers beyond each cut (1: the central
    differences reach one voxel).  Returns (vol_origin, own_lo, own_hi, local_dims, (a0, a1)): the rank holds the
    voxels [a0, a1) along `axis` and owns [own_lo, own_hi) in global coordinates; the own boxes of the ranks tile the
    volume."""
    dims, _, _, org, local, held = _slab_cut("slab_voxels", dims, axis, rank, world, halo)
    lo, hi = [0, 0, 0], list(dims)
    lo[axis], hi[axis] = shard_range(dims[axis], rank, world)
    return tuple(org), tuple(lo), tuple(hi), local, held


def slab_cells(dims, axis, rank, world, cap=False, gradients=False):
    """slab_voxels' twin for the cell-space call (render.isosurface_mesh): rank `rank`'s slab when the CELLS of a volume
    of `dims` voxels are cut into `world` slabs along `axis`.  Along an axis of G voxels there are G - 1 cells from 0
    without cap and G + 1 cells from -1 with it; shard_range cuts them.  Returns (vol_origin, own_lo, own_hi,
    local_dims, (a0, a1)): the rank owns the cells own_lo <= c < own_hi (global cell coordinates) and holds the voxels
    [a0, a1) along `axis` -- every in-volume point of the closed point box [own_lo, own_hi], and one layer more on both
    sides with `gradients` (vrhip.h).  The own boxes of the ranks tile the cell range, so the ranks' meshes
    concatenate with no exchange (render.IsoMesh.concat); a rank beyond the number of cells owns an empty box."""
    dims = [int(q) for q in dims]
    if len(dims) != 3 or any(q < 1 for q in dims) or axis not in (0, 1, 2) or world < 1 or not 0 <= rank < world:
        raise ValueError("slab_cells: axis %r, rank %r of %r, extents %r" % (axis, rank, world, dims))
    n, grow = dims[axis], 1 if gradients else 0
    first, cells = (-1, n + 1) if cap else (0, n - 1)
    s0, s1 = shard_range(cells, rank, world)
    lo = [-1, -1, -1] if cap else [0, 0, 0]
    hi = list(dims) if cap else [q - 1 for q in dims]
    lo[axis], hi[axis] = first + s0, first + s1
    a0 = min(max(lo[axis] - grow, 0), n - 1)
    a1 = max(min(hi[axis] + grow, n - 1), a0) + 1
    org, local = [0, 0, 0], list(dims)
    org[axis], local[axis] = a0, a1 - a0
    return tuple(org), tuple(lo), tuple(hi), tuple(local), (a0, a1)


def histogram_all_reduce(hist, group=None):
    """The sum of every rank's histogram (any of render's tables: counts add exactly): an int64 all-reduce over `group`
    (None: the default group).  Without a process group -- torch.distributed not initialised -- it is the identity.
    hist: an integer numpy array or torch tensor; returns the same kind, shape and dtype."""
    import numpy as np
    is_np = not isinstance(hist, torch.Tensor)
    if not dist.is_initialized():
        return hist
    t = torch.from_numpy(np.ascontiguousarray(hist).astype(np.int64)) if is_np else hist.to(torch.int64).clone()
    if dist.get_backend(group) == "nccl":
        t = t.cuda()
    dist.all_reduce(t, op=dist.ReduceOp.SUM, group=group)
    if is_np:
        return t.cpu().numpy().astype(np.asarray(hist).dtype)
    return t.to(device=hist.device, dtype=hist.dtype)


_compositors = {}


def _compositor(group, world, rank, W, H):
    """The C-ABI compositor of (group, frame size): its RCCL communicator is created once from an ncclUniqueId that
    rank 0 asks the library for and the process group passes on."""
    key = (id(group), world, rank, W, H)
    h = _compositors.get(key)
    if h is None:
        from . import _lib
        from ._lib import check
        L = _lib.lib()
        uid = (C.c_uint8 * 128)()
        if world > 1:
            box = [None]
            if rank == 0:
                check(L.vr_rccl_unique_id(uid), "vr_rccl_unique_id")
                box[0] = bytes(uid)
            dist.broadcast_object_list(box, src=0, group=group)
            uid = (C.c_uint8 * 128).from_buffer_copy(box[0])
        h = C.c_void_p()
        check(L.vr_compositor_create(C.byref(h), uid, rank, world, W, H), "vr_compositor_create")
        _compositors[key] = h
    return h


def _check_image(t, what, shape=None):
    if t.dtype != torch.float32:
        raise ValueError("%s must be float32, not %s" % (what, t.dtype))
    if t.dim() != 3 or t.shape[2] != 4 or (shape is not None and tuple(t.shape) != shape):
        raise ValueError("%s must be shaped %s, not %s" % (what, shape or "(H, W, 4)", tuple(t.shape)))
    if not t.is_contiguous():
        raise ValueError("%s must be contiguous" % what)


def composite_sort_last(partial, cam, params, axis=2, group=None, combine=None, out=None):
    """partial: this rank's (c, tau, covered, 0) image [H][W][4] float32 (rank r holds slab r along
    `axis`).  Returns the finished RGBA frame [H][W][4] on rank 0 (None elsewhere).

    Device tensors take the C-ABI compositor (vr_compositor_composite: grouped RCCL send/recv, k_composite_slabs,
    gather -- what a C++ host calls); it reads `partial` (and writes `out`) through raw pointers, so anything but a
    contiguous float32 (H, W, 4) device tensor raises ValueError before any C call.  With an injected `combine` (the
    CPU tests: gloo, the oracle's combine) the same exchange runs over torch.distributed point-to-point operations."""
    return _sort_last("grey", None, partial, cam, params, axis, group, combine, out)


def composite_sort_last_tf(partial, cam, params, tf, axis=2, group=None, combine=None, out=None):
    """composite_sort_last for colour partials: partial = this rank's (C.r, C.g, C.b, T) image [H][W][4] float32 from
    raycast_tf_partial (unlit or lit) or raycast_tf2d_partial, tf the TransferFunction or TransferFunction2D whose
    background finishes the frame (nothing else of it is read).  The same exchange;
    device tensors take vr_compositor_composite_tf, an injected `combine(parts, first_pixel, axis, cam, params)` runs
    over torch.distributed point-to-point operations."""
    from .render import background_desc
    background_desc(tf)         # ValueError for anything but the two table classes
    return _sort_last("colour", tf, partial, cam, params, axis, group, combine, out)


def composite_sort_last_proj(partial, proj, group=None, combine=None, out=None):
    """composite_sort_last for projection partials: partial = this rank's (v, n, 0, 0) image [H][W][4] float32 from
    raycast_projection_partial (slab_params with halo=1), proj the Projection that finishes the frame.  The same
    exchange, without camera, axis or params: the combine has no view order.  Device tensors take
    vr_compositor_composite_proj; an injected `combine(parts, proj)` (parts: [world][pixels][4]) runs over
    torch.distributed point-to-point operations.  MAX and MIN frames equal the single-GPU frame bit for bit."""
    from .render import _check_projection
    _check_projection(proj, partial.device)        # a table goes to C as a raw pointer: it must live where the partial does
    return _sort_last("proj", proj, partial, None, None, 0, group, combine, out)


def _sort_last(kind, finish, partial, cam, params, axis, group, combine, out):
    """The exchange of the three calls.  kind: "grey" partials, "colour" partials, which `finish` (a TransferFunction)
    finishes, or "proj" partials, which `finish` (a Projection) combines and finishes without a view order."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if combine is None and partial.is_cuda:
        # the C ABI reads (and writes) dense float32 [H][W][4] through raw pointers: anything else is refused here
        _check_image(partial, "partial")
        H, W = partial.shape[0], partial.shape[1]
        if rank == 0 and out is not None:
            _check_image(out, "out", (H, W, 4))
            if out.device != partial.device:
                raise ValueError("out must be on %s, not %s" % (partial.device, out.device))
        from . import _lib
        from .codec import _stream_ptr
        from ._lib import check
        h = _compositor(group, world, rank, W, H)
        frame = None
        if rank == 0:
            frame = out if out is not None else torch.empty((H, W, 4), dtype=torch.float32, device=partial.device)
        src, dst = C.c_void_p(partial.data_ptr()), C.c_void_p(frame.data_ptr()) if rank == 0 else None
        if kind == "grey":
            check(_lib.lib().vr_compositor_composite(h, src, int(axis), C.byref(cam), C.byref(params), dst, _stream_ptr()),
                  "vr_compositor_composite")
        elif kind == "colour":
            from .render import background_desc
            desc = background_desc(finish)
            check(_lib.lib().vr_compositor_composite_tf(h, src, int(axis), C.byref(cam), C.byref(params), C.byref(desc), dst,
                                                        _stream_ptr()), "vr_compositor_composite_tf")
        else:
            desc = finish.desc()
            check(_lib.lib().vr_compositor_composite_proj(h, src, C.byref(desc), dst, _stream_ptr()),
                  "vr_compositor_composite_proj")
        return frame
    H, W = partial.shape[0], partial.shape[1]

    def tile(parts, first_pixel):
        """The finished pixels of a tile: the injected combine, else the kind's slab call."""
        if kind == "proj":
            return (combine or _gpu_combine_proj)(parts, finish)
        if combine is not None:
            return combine(parts, first_pixel, axis, cam, params)
        if kind == "grey":
            return _gpu_combine(parts, first_pixel, axis, cam, params)
        return _gpu_combine_tf(parts, first_pixel, axis, cam, params, finish)

    rows = tile_rows(H, world)
    if world == 1:
        return tile(partial.reshape(1, H * W, 4), 0).reshape(H, W, 4)
    # send tile t to rank t, receive my tile from everybody (slab order = rank order)
    send = [partial[lo:hi].reshape(-1, 4).contiguous() for lo, hi in rows]
    my_lo, my_hi = rows[rank]
    npix = (my_hi - my_lo) * W
    recv = [torch.empty((npix, 4), dtype=partial.dtype, device=partial.device) for _ in range(world)]
    recv[rank].copy_(send[rank])
    # grouped point-to-point = ncclGroupStart / ncclSend / ncclRecv / ncclGroupEnd on RCCL; unlike
    # all_to_all it also exists on gloo, which the CPU tests use
    ops = []
    for peer in range(world):
        if peer == rank:
            continue
        ops.append(dist.P2POp(dist.isend, send[peer], peer, group))
        ops.append(dist.P2POp(dist.irecv, recv[peer], peer, group))
    for req in dist.batch_isend_irecv(ops):
        req.wait()
    parts = torch.stack(recv, 0)
    done = tile(parts, my_lo * W)
    # gather the finished tiles on rank 0 (tiles may differ by one row: pad to the largest)
    max_rows = max(hi - lo for lo, hi in rows)
    padded = torch.zeros((max_rows * W, 4), dtype=done.dtype, device=done.device)
    padded[:npix] = done
    gathered = [torch.empty_like(padded) for _ in range(world)] if rank == 0 else None
    dist.gather(padded, gathered, dst=0, group=group)
    if rank != 0:
        return None
    frame = torch.empty((H, W, 4), dtype=done.dtype, device=done.device)
    for r, (lo, hi) in enumerate(rows):
        frame[lo:hi] = gathered[r][:(hi - lo) * W].reshape(hi - lo, W, 4)
    return frame
