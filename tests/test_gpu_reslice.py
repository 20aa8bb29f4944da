"""Slice views on the GPU (vr_reslice, vr_reslice_partial; the rule is in include/vrhip.h): known answers on axis-aligned
planes, partials and frames bit for bit against the float32 restatement of tests/refslice.py, the wave footprint switch,
slabs of 2 to 8 ranks along every axis against the single-GPU slice, vr_compositor_composite_proj through the loopback
transport, the viewer and the C++ example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refslice as RS  # noqa: E402
from test_gpu_compositor import DIMS, H, W, WORLDS, Ranks, build_loopback, check_log  # noqa: E402
from test_gpu_compositor import scene_volume as slab_volume  # noqa: E402
from test_gpu_transfer_function import smooth_table  # noqa: E402
from test_reslice_cpu import SCENE_DIMS, oblique_plane, scene_volume  # noqa: E402

pytestmark = pytest.mark.gpu
OPS = ("max", "min", "mean")
FILTERS = ("nearest", "linear")
BG = (0.2, 0.4, 0.6)


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def L(vr):
    from volumerenderer_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def LB(L, tmp_path_factory):
    """The loopback transport of test_gpu_compositor.py, loaded after libvrhip.so."""
    lb = C.CDLL(build_loopback(tmp_path_factory.mktemp("loopback_slice")))
    lb.lb_create.restype = C.c_void_p; lb.lb_create.argtypes = [C.c_int32, C.c_double]
    lb.lb_destroy.argtypes = [C.c_void_p]
    lb.lb_rank_ctx.restype = C.c_void_p; lb.lb_rank_ctx.argtypes = [C.c_void_p, C.c_int32]
    lb.lb_transport.restype = C.c_void_p
    lb.lb_log_size.argtypes = [C.c_void_p]
    lb.lb_log_entry.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    lb.lb_log_clear.argtypes = [C.c_void_p]
    lb.lb_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    return lb


def _dev(vol):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda().reshape(-1)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- 1. known answers --------------------------------------------------------------------------------------------------
def test_axis_aligned_slices_are_the_volume_planes(vr):
    """Power-of-two extents: the positions are exact and the fetch's weights are exactly 0, so both filters return the
    voxel itself: v == plane * float32(1/255) bit for bit and n == 1 everywhere."""
    vol = np.random.default_rng(41).integers(0, 256, (8, 16, 32), dtype=np.uint8)        # [Z][Y][X]: 32 x 16 x 8
    dims = (32, 16, 8)
    dvol = _dev(vol)
    k = np.float32(1 / 255)
    assert k == np.float32(1) / np.float32(255)
    for axis in (0, 1, 2):
        for index in (2, 5, 0, dims[axis] - 1):                 # both parities and both faces
            want = np.take(vol, index, 2 - axis).astype(np.float32) * k
            for flt in FILTERS:
                plane = vr.SlicePlane.axis_aligned(dims, axis, index, filter=flt)
                assert (plane.height, plane.width) == want.shape
                mirrored = vr.SlicePlane.axis_aligned(dims, axis, index, filter=flt)
                cu = int(np.nonzero(plane.du)[0][0])
                o = list(plane.origin)
                o[cu] = 1.0 - plane.origin[cu]                  # from the far edge, columns run backwards
                mirrored.origin, mirrored.du = tuple(o), tuple(-q for q in plane.du)
                for pl, w in ((plane, want), (mirrored, want[:, ::-1])):
                    for op in OPS:
                        part = _np(vr.reslice_partial(dvol, dims, pl, vr.Projection(op)))
                        assert np.array_equal(part[..., 0], w), (axis, index, flt, op)
                        assert (part[..., 1] == 1).all() and (part[..., 2:] == 0).all()
                    frame = _np(vr.reslice(dvol, dims, pl, vr.Projection("max")))
                    assert np.array_equal(frame[..., 0], w) and (frame[..., 3] == 1).all()


# ---- 2. bit for bit against the float32 restatement ----------------------------------------------------------------------
@pytest.mark.parametrize("size", [(72, 54), (7, 5), (65, 63)], ids=["72x54", "7x5", "65x63"])
@pytest.mark.parametrize("which", [0, 1, 2])
def test_oblique_slices_equal_the_float32_reference(vr, which, size):
    import torch
    vol = scene_volume()
    dvol = _dev(vol)
    lut = vr.transfer_function_table(smooth_table(np.random.default_rng(5)))
    empty_seen = False
    for layers in (1, 7):
        for flt in FILTERS:
            plane = oblique_plane(which, size[0], size[1], layers, flt)
            for op in OPS:
                grey = vr.Projection(op, background=BG)
                part = vr.reslice_partial(dvol, SCENE_DIMS, plane, grey)
                ref = RS.partial(vol, plane, grey.op)
                assert torch.equal(part.cpu(), torch.from_numpy(ref)), (which, size, layers, flt, op)
                n = ref[..., 1]
                assert (n > 0).any() and n.max() <= layers
                for proj in (grey, vr.Projection(op, (0.1, 0.9), BG, lut)):
                    frame = vr.reslice(dvol, SCENE_DIMS, plane, proj)
                    assert torch.equal(vr.composite_finish_proj(part, proj), frame), (which, size, layers, flt, op)
                    table = None if proj.lut is None else lut
                    want = RS.finish(ref, proj.op, proj.window, BG, table)
                    assert torch.equal(frame.cpu(), torch.from_numpy(want)), (which, size, layers, flt, op, table is not None)
                    if (n == 0).any():
                        empty_seen = True
                        got = _np(frame)[n == 0]
                        assert np.array_equal(got, np.broadcast_to(np.float32(BG + (0.0,)), got.shape))
    assert empty_seen == (which == 2)           # the third plane sticks out of the cube, the others do not


def test_wave_footprint_switch_changes_no_pixel(vr, L):
    """vr_debug_set("reslice_tile_w"): 8 x 8, 16 x 4 and 64 x 1 pixel tiles draw the same partial, edges included."""
    import torch
    vol = scene_volume()
    dvol = _dev(vol)
    try:
        for size in ((7, 5), (65, 63), (130, 3)):
            for flt in FILTERS:
                plane = oblique_plane(2, size[0], size[1], 7, flt)
                want = torch.from_numpy(RS.partial(vol, plane, RS.MEAN))
                for tw in (8, 16, 64):
                    assert L.vr_debug_set(b"reslice_tile_w", tw) == 0
                    out = torch.full((size[1] + 1, size[0], 4), -7.0, dtype=torch.float32, device="cuda")
                    vr.reslice_partial(dvol, SCENE_DIMS, plane, vr.Projection("mean"), out=out[:size[1]])
                    assert torch.equal(out[:size[1]].cpu(), want), (size, flt, tw)
                    assert (out[size[1]] == -7.0).all()             # nothing is written past the frame
        for bad in (0, 4, 32, 128, -8):
            assert L.vr_debug_set(b"reslice_tile_w", bad) == -1
    finally:
        assert L.vr_debug_set(b"reslice_tile_w", 16) == 0           # the library's default


# ---- 3. slabs ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volume():
    return slab_volume()


def slab_scene_plane(vr, axis, layers, flt):
    """An oblique W x H slice of the compositor scene whose layers are stacked (roughly) along `axis`, 0.04 apart: nine
    of them cross every slab boundary near the centre for 2 to 8 slabs."""
    right, down = {0: ((0.1, 1.0, 0.15), (-0.2, 0.05, 1.0)), 1: ((1.0, 0.1, 0.15), (0.05, -0.2, 1.0)),
                   2: ((1.0, 0.1, 0.15), (0.05, 1.0, -0.2))}[axis]
    return vr.SlicePlane.from_frame((0.5, 0.5, 0.5), right, down, W, H, 0.011, layers, 0.04, flt)


def _slab_partials(vr, vol, plane, axis, world, proj, halo=1):
    import torch
    from volumerenderer_amd import distributed as D
    parts = []
    for r in range(world):
        p, local, (a0, a1) = D.slab_plane(plane, DIMS, axis, r, world, halo)
        sl = [slice(None)] * 3
        sl[2 - axis] = slice(a0, a1)
        parts.append(vr.reslice_partial(_dev(vol[tuple(sl)]), local, p, proj).reshape(-1, 4))
    return torch.stack(parts, 0)


def _slabs(stack, proj):
    from volumerenderer_amd import distributed as D
    return D._gpu_combine_proj(stack.contiguous(), proj)


SLAB_CASES = [(wd, ax) for wd in WORLDS for ax in (0, 1, 2)]


@pytest.mark.parametrize("world,axis", SLAB_CASES, ids=["w%d-ax%d" % c for c in SLAB_CASES])
def test_slabs_equal_the_single_gpu_slice(vr, volume, world, axis):
    import torch
    dvol = _dev(volume)
    rng = np.random.default_rng(world * 3 + axis)
    u = 2.0 ** -24
    N = 9
    g = (N - 1) * u / (1 - (N - 1) * u)          # the bound of two summation orders (test_gpu_projection.py)
    told = shared = 0
    for layers in (1, N):
        for flt in FILTERS:
            plane = slab_scene_plane(vr, axis, layers, flt)
            for op in OPS:
                proj = vr.Projection(op)
                frame = vr.reslice(dvol, DIMS, plane, proj)
                part = vr.reslice_partial(dvol, DIMS, plane, proj).reshape(-1, 4)
                assert (part[:, 1] == layers).float().mean() > 0.5
                stack = _slab_partials(vr, volume, plane, axis, world, proj)
                shared += int(((stack[..., 1] > 0).sum(0) > 1).sum())
                orders = [list(range(world)), [int(k) for k in rng.permutation(world)], list(range(world - 1, -1, -1))]
                for order in orders:
                    acc = stack[order[0]].clone()
                    for k in order[1:]:
                        vr.composite_combine_proj(acc, stack[k].contiguous(), proj)
                    got = _slabs(stack[order], proj).reshape(H, W, 4)
                    assert torch.equal(acc[:, 1], part[:, 1]), (layers, flt, op, order)          # n is exact for every op
                    if op != "mean" or layers == 1:
                        assert torch.equal(acc, part), (layers, flt, op, order)
                        assert torch.equal(got, frame), (layers, flt, op, order)
                    else:
                        d = (got - frame).abs().max().item()
                        assert d <= 2 * g + 2 * u, (flt, order, d)
                if op == "max" and flt == "linear":
                    # one halo layer is needed: without it a slab's edge samples read clamped voxels
                    bare = _slabs(_slab_partials(vr, volume, plane, axis, world, proj, halo=0), proj).reshape(H, W, 4)
                    told += int(not torch.equal(bare, frame))
    assert shared > 0, "no pixel owns samples in more than one slab"
    assert told >= 1, "the scene cannot tell a missing halo layer"


# ---- 4. the compositor ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", WORLDS)
def test_compositor_exchange_of_slice_partials(vr, L, LB, volume, world):
    import torch
    from volumerenderer_amd import distributed as D
    for axis, op, layers, flt in ((world % 3, "max", 9, "linear"), ((world + 1) % 3, "min", 9, "nearest"),
                                  ((world + 2) % 3, "mean", 1, "linear")):
        plane = slab_scene_plane(vr, axis, layers, flt)
        proj = vr.Projection(op, (0.0, 0.8), BG)
        slabs, planes, subs = [], [], []
        for r in range(world):
            p, local, (a0, a1) = D.slab_plane(plane, DIMS, axis, r, world, 1)
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(a0, a1)
            slabs.append(_dev(volume[tuple(sl)]))
            planes.append(p.desc())
            subs.append((C.c_int64 * 3)(*local))
        parts = [torch.empty((H, W, 4), dtype=torch.float32, device="cuda") for _ in range(world)]
        frame = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        pd = proj.desc()
        ranks = Ranks(vr, L, LB, world, W, H)
        try:
            torch.cuda.synchronize()        # uploads and the NaN fill are on torch's stream, the ranks use their own

            def job(r):
                def go():
                    buf = C.c_void_p(parts[r].data_ptr())
                    dst = C.c_void_p(frame.data_ptr()) if r == 0 else None
                    return [L.vr_reslice_partial(C.c_void_p(slabs[r].data_ptr()), subs[r], C.byref(planes[r]), C.byref(pd), buf,
                                                 ranks.streams[r]),
                            L.vr_compositor_composite_proj(ranks.comps[r], buf, C.byref(pd), dst, ranks.streams[r])]
                return go

            rcs = ranks.run([job(r) for r in range(world)])
            ranks.sync()
            assert all(rc == 0 for x in rcs for rc in x), (rcs, ranks.errors())
            check_log(ranks.log(), world, W, H)
            assert ranks.errors() == ""
        finally:
            ranks.close()
        assert not torch.isnan(frame).any()
        stack = torch.stack([p.reshape(-1, 4) for p in parts], 0)
        assert int(((stack[..., 1] > 0).sum(0) > 1).sum()) > 0 or layers == 1
        assert torch.equal(_slabs(stack, proj).reshape(H, W, 4), frame), "exchange or tile offset bug"
        assert torch.equal(vr.reslice(_dev(volume), DIMS, plane, proj), frame), (world, axis, op)


# ---- 5. surfaces ---------------------------------------------------------------------------------------------------------
def test_python_wrappers_refuse_bad_device_buffers(vr):
    import torch
    vol = torch.zeros(64, dtype=torch.uint8, device="cuda")
    plane, proj = vr.SlicePlane.axis_aligned((4, 4, 4), 2, 1), vr.Projection()
    with pytest.raises(ValueError):
        vr.reslice(vol, (4, 4, 5), plane, proj)                                 # the size does not match
    with pytest.raises(ValueError):
        vr.reslice(vol, (4, 4, 4), plane, proj, out=torch.zeros((4, 4, 3), device="cuda"))
    with pytest.raises(ValueError):
        vr.reslice_partial(vol, (4, 4, 4), plane, proj, out=torch.zeros((4, 4, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        vr.reslice(vol, (4, 4, 4), plane, "max")
    with pytest.raises(ValueError):
        vr.reslice(vol, (4, 4, 4), plane, vr.Projection("max", lut=np.zeros((256, 4), np.float32), device="cpu"))
    out = torch.empty((4, 4, 4), dtype=torch.float32, device="cuda")
    assert vr.reslice(vol, (4, 4, 4), plane, proj, out=out) is out


def test_viewer_draw_slice(vr):
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    vol = scene_volume()
    dvol = _dev(vol)
    v = HeadlessViewer(120, 90)
    for plane in (vr.SlicePlane.axis_aligned(SCENE_DIMS, 1, 7, 2.0), oblique_plane(1, 50, 30, 4, "nearest")):
        proj = vr.Projection("mean", (0.0, 0.9), (0.0, 0.0, 0.1))
        frame = v.draw_slice(dvol, SCENE_DIMS, plane, proj)
        assert frame.shape == (plane.height, plane.width, 4)
        assert torch.equal(frame, vr.reslice(dvol, SCENE_DIMS, plane, proj)) and (frame[..., 3] > 0).any()


def _fnv1a64(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_example_hashes_equal_the_python_frames(vr, tmp_path):
    """examples/slice.cpp (g++ against Slice.hpp) draws the two slices Python draws: the same FNV-1a-64."""
    from test_reslice_cpu import compile_example
    exe = compile_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [l.split() for l in r.stdout.splitlines()]
    assert [l[:5] for l in lines] == [["slice", "48", "x", "40", "fnv1a64"], ["slice", "96", "x", "64", "fnv1a64"]], r.stdout
    X, Y, Z = 48, 40, 32
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    val = ((x * 5 + y * 3) ^ (z * 7)) & 255
    vol = np.where(val > 200, val, val // 16).astype(np.uint8)
    planes = [(vr.SlicePlane.axis_aligned((X, Y, Z), 2, 13), vr.Projection("max")),
              (vr.SlicePlane.from_frame((0.5, 0.5, 0.5), (1.0, 0.3, 0.2), (-0.2, 1.0, 0.4), 96, 64, 0.012, 5, 0.02),
               vr.Projection("max", background=(0.0, 0.0, 0.25)))]
    for (plane, proj), words in zip(planes, lines):
        frame = _np(vr.reslice(_dev(vol), (X, Y, Z), plane, proj))
        assert (frame[..., 3] > 0).mean() > 0.5
        assert int(words[5], 16) == _fnv1a64(frame.tobytes())
    assert (_np(vr.reslice(_dev(vol), (X, Y, Z), *planes[1]))[..., 3] == 0).any()       # the corners stick out
