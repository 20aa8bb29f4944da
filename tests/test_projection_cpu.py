"""Intensity projections (vr_raycast_projection & co.) without a GPU: the C struct, the argument checks of the eight new
entry points (VR_ERR_INVALID before VR_ERR_NO_DEVICE), the Python wrappers' ValueErrors, the float64 reference of
tests/refproject.py against closed forms and across slabs, vr_lod_select in projection mode,
distributed.composite_sort_last_proj over gloo with an injected NumPy combine, and examples/projection.cpp."""
import ctypes as C
import itertools
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refproject as RP  # noqa: E402
from refmarch import rays  # noqa: E402
from test_gpu_compositor import DIMS, STEPS, cameras, scene_volume, slab_setup  # noqa: E402

VR_ERR_INVALID, VR_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("vr_raycast_projection", "vr_raycast_pool_projection", "vr_raycast_projection_partial",
               "vr_raycast_pool_projection_partial", "vr_composite_combine_proj", "vr_composite_finish_proj",
               "vr_composite_slabs_proj", "vr_compositor_composite_proj")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def test_struct_layout_and_constants():
    from volumerenderer_amd import _lib
    T = _lib.Projection
    assert C.sizeof(T) == 32
    assert (T.lut_dev.offset, T.op.offset, T.window_lo.offset, T.window_hi.offset, T.background.offset) == (0, 8, 12, 16, 20)
    assert _lib.RENDER_PROJECTION == 4
    assert (_lib.PROJECT_MAX, _lib.PROJECT_MIN, _lib.PROJECT_MEAN) == (0, 1, 2)
    header = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    assert "VR_RENDER_PROJECTION = 4" in header
    assert "VR_PROJECT_MAX = 0, VR_PROJECT_MIN = 1, VR_PROJECT_MEAN = 2" in header


def test_symbols_exported_and_declared(L):
    from volumerenderer_amd import _lib
    header = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES and ("vr_status %s(" % name) in header, name


def _proj(lut=None, op=0, lo=0.0, hi=1.0, bg=(0.0, 0.0, 0.0)):
    from volumerenderer_amd import _lib
    p = _lib.Projection()
    p.lut_dev, p.op, p.window_lo, p.window_hi = lut, op, lo, hi
    p.background[:] = bg
    return p


def _bad_projections(B):
    """Every way a vr_projection can be wrong, one at a time."""
    inf, nan = math.inf, math.nan
    return [_proj(op=-1), _proj(op=3), _proj(lo=0.5, hi=0.5), _proj(lo=0.75, hi=0.25), _proj(lo=nan), _proj(hi=nan),
            _proj(lo=-inf), _proj(hi=inf), _proj(bg=(0.0, nan, 0.0)), _proj(bg=(inf, 0.0, 0.0)), _proj(bg=(0.0, 0.0, -inf)),
            _proj(lut=B.lut + 4), _proj(lut=B.lut + 8)]


@pytest.mark.parametrize("partial", [False, True])
def test_marches_reject_bad_arguments_before_the_device(L, partial):
    from test_transfer_function_cpu import _Bufs
    from volumerenderer_amd import render as R
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)
    I64 = C.c_int64 * 3
    fd = L.vr_raycast_projection_partial if partial else L.vr_raycast_projection
    fp = L.vr_raycast_pool_projection_partial if partial else L.vr_raycast_pool_projection
    try:
        def params(mode=4, **kw):
            P = R.default_params(8, 8, (4, 4, 4), mode)
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(P, k)[:] = v
                else:
                    setattr(P, k, v)
            return P

        def ref(x):
            return None if x is None else C.byref(x)

        def dense(**kw):
            a = dict(vol=B.vol, dims=I64(4, 4, 4), cam=R.default_camera(), P=params(), pj=_proj(), img=B.img)
            a.update(kw)
            return fd(a["vol"], a["dims"], ref(a["cam"]), ref(a["P"]), ref(a["pj"]), a["img"], None)

        def pool(**kw):
            a = dict(pool=B.vol, table=B.table, bd=I64(4, 4, 4), grid=I64(1, 1, 1), cam=R.default_camera(), P=params(),
                     pj=_proj(), img=B.img)
            a.update(kw)
            return fp(a["pool"], a["table"], a["bd"], a["grid"], ref(a["cam"]), ref(a["P"]), ref(a["pj"]), a["img"], None)

        # each null pointer in turn
        for k in ("vol", "dims", "cam", "P", "pj", "img"):
            assert dense(**{k: None}) == VR_ERR_INVALID, k
        for k in ("pool", "table", "bd", "grid", "cam", "P", "pj", "img"):
            assert pool(**{k: None}) == VR_ERR_INVALID, k
        # shared: the frame, the mode, max_samples, the projection
        shared = [{"P": params(width=0)}, {"P": params(height=-1)}, {"P": params(max_samples=-1)},
                  {"P": params(max_samples=(1 << 24) + 1)}]
        shared += [{"P": params(mode=m)} for m in (-1, 0, 1, 2, 3, 5)]
        shared += [{"pj": p} for p in _bad_projections(B)]
        for k, kw in enumerate(shared):
            assert dense(**kw) == VR_ERR_INVALID and pool(**kw) == VR_ERR_INVALID, (k, sorted(kw))
        for d in ((0, 4, 4), (4, -1, 4), (4, 4, 1 << 31)):
            assert dense(dims=I64(*d)) == VR_ERR_INVALID, d
        # the pool restrictions
        for kw in ({"bd": I64(4, 6, 4)}, {"bd": I64(0, 4, 4)}, {"grid": I64(1, 0, 1)}, {"grid": I64(1 << 29, 1, 1)},
                   {"P": params(vol_origin=(1, 0, 0))}, {"P": params(vol_origin=(0, 0, -1))},
                   {"P": params(global_dims=(8, 4, 4))}):
            assert pool(**kw) == VR_ERR_INVALID, sorted(kw)
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback
            for op in (0, 1, 2):
                assert dense(pj=_proj(op=op)) == VR_ERR_NO_DEVICE and pool(pj=_proj(op=op)) == VR_ERR_NO_DEVICE
            assert dense(pj=_proj(lut=B.lut, lo=0.1, hi=0.9, bg=(0.2, 0.4, 0.6))) == VR_ERR_NO_DEVICE
            assert dense(P=params(max_samples=1 << 24)) == VR_ERR_NO_DEVICE
            assert pool(P=params(global_dims=(4, 4, 4))) == VR_ERR_NO_DEVICE
    finally:
        B.free()


def test_combine_calls_reject_bad_arguments_before_the_device(L):
    from test_transfer_function_cpu import _Bufs
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)          # B.img: 8 x 8 pixels; B.lut (4 KiB) stands in for a second image of 8 x 8
    try:
        npx = 64
        for a in ((None, B.lut, npx, 0), (B.img, None, npx, 0), (B.img, B.lut, 0, 0), (B.img, B.lut, -3, 0),
                  (B.img, B.lut, npx, -1), (B.img, B.lut, npx, 3)):
            assert L.vr_composite_combine_proj(*a, None) == VR_ERR_INVALID, a
        ok = _proj()
        assert L.vr_composite_finish_proj(None, C.byref(ok), B.lut, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_proj(B.img, None, B.lut, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_proj(B.img, C.byref(ok), None, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_proj(B.img, C.byref(ok), B.lut, 0, None) == VR_ERR_INVALID
        assert L.vr_composite_slabs_proj(None, 1, npx, C.byref(ok), B.lut, None) == VR_ERR_INVALID
        assert L.vr_composite_slabs_proj(B.img, 0, npx, C.byref(ok), B.lut, None) == VR_ERR_INVALID
        assert L.vr_composite_slabs_proj(B.img, -1, npx, C.byref(ok), B.lut, None) == VR_ERR_INVALID
        assert L.vr_composite_slabs_proj(B.img, 1, 0, C.byref(ok), B.lut, None) == VR_ERR_INVALID
        assert L.vr_composite_slabs_proj(B.img, 1, npx, None, B.lut, None) == VR_ERR_INVALID
        assert L.vr_composite_slabs_proj(B.img, 1, npx, C.byref(ok), None, None) == VR_ERR_INVALID
        for bad in _bad_projections(B):
            assert L.vr_composite_finish_proj(B.img, C.byref(bad), B.lut, npx, None) == VR_ERR_INVALID
            assert L.vr_composite_slabs_proj(B.img, 1, npx, C.byref(bad), B.lut, None) == VR_ERR_INVALID
        # a null handle is refused before anything else
        assert L.vr_compositor_composite_proj(None, B.img, C.byref(ok), B.lut, None) == VR_ERR_INVALID
        if n.value == 0:
            for op in (0, 1, 2):
                assert L.vr_composite_combine_proj(B.img, B.lut, npx, op, None) == VR_ERR_NO_DEVICE
                assert L.vr_composite_finish_proj(B.img, C.byref(_proj(op=op)), B.lut, npx, None) == VR_ERR_NO_DEVICE
                assert L.vr_composite_slabs_proj(B.img, 1, npx, C.byref(_proj(op=op)), B.lut, None) == VR_ERR_NO_DEVICE
    finally:
        B.free()


# ---- Python wrappers -------------------------------------------------------------------------------------------------
def test_projection_rejects_bad_values():
    pytest.importorskip("torch")
    import volumerenderer_amd as vr
    from volumerenderer_amd import _lib
    P = vr.Projection
    for kw in ({"op": "median"}, {"op": 3}, {"op": -1}, {"op": None}, {"op": 1.0}, {"window": (0.5, 0.5)},
               {"window": (0.75, 0.25)}, {"window": (0.0, math.nan)}, {"window": (-math.inf, 1.0)}, {"window": (0.0,)},
               {"window": 1.0}, {"window": (1.0, 1.0 + 1e-12)}, {"background": (0.0, math.nan, 0.0)},
               {"background": (0.0, 0.0)}, {"lut": np.zeros((255, 4))}, {"lut": np.full((256, 4), 1.5)},
               {"lut": np.full((256, 4), np.nan)}):
        with pytest.raises(ValueError):
            P(device="cpu", **kw)
    p = P("mean", (0.25, 0.75), (0.1, 0.2, 0.3), np.zeros((256, 4), np.float32), device="cpu")
    d = p.desc()
    assert (d.op, d.window_lo, d.window_hi) == (_lib.PROJECT_MEAN, 0.25, 0.75) and d.lut_dev == p.lut.data_ptr()
    assert [round(v, 6) for v in d.background] == [0.1, 0.2, 0.3]
    d = P().desc()
    assert (d.op, d.window_lo, d.window_hi, tuple(d.background), d.lut_dev) == (0, 0.0, 1.0, (0.0, 0.0, 0.0), None)
    assert [P(op).op for op in ("max", "min", "mean", 0, 1, 2)] == [0, 1, 2, 0, 1, 2]


def test_python_wrappers_raise_before_any_c_call():
    """What can be refused without a device; a device tensor of the wrong dtype, a strided partial and a foreign `proj`
    are in test_gpu_projection.test_python_wrappers_refuse_bad_device_buffers."""
    torch = pytest.importorskip("torch")
    import volumerenderer_amd as vr
    from volumerenderer_amd import distributed as D
    from volumerenderer_amd import render as R
    for name in ("Projection", "raycast_projection", "raycast_pool_projection", "raycast_projection_partial",
                 "raycast_pool_projection_partial", "composite_combine_proj", "composite_finish_proj"):
        assert callable(getattr(vr, name)), name
    proj = R.Projection(device="cpu")
    host = torch.zeros((4, 4, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        R.composite_combine_proj(host, host, proj)              # not on the device
    with pytest.raises(ValueError):
        R.composite_finish_proj(host, proj)
    with pytest.raises(ValueError):
        R.composite_combine_proj(np.zeros((4, 4, 4), np.float32), host, proj)
    with pytest.raises(ValueError):
        D.composite_sort_last_proj(host, None)
    with pytest.raises(ValueError):
        D.composite_sort_last_proj(host, "max")


# ---- the float64 reference -------------------------------------------------------------------------------------------
CAM = ((0.02, -0.03, -3.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 6.0)      # far and narrow: every ray crosses z = 0 .. 1
STEP = (1 / 60.5,) * 3


@pytest.mark.parametrize("value", [0, 77, 255])
def test_reference_constant_volume(value):
    vol = np.full((12, 10, 14), value, np.uint8)
    pos, front, up, fov = CAM
    cov, vuv, g = rays(pos, front, up, fov, 24, 16)
    assert cov.all()
    for op in RP.OPS:
        v, n = RP.project(vol, cov, vuv, g, STEP, op)
        assert (n >= 58).all() and (n <= 62).all()
        img = RP.finish(v, n, op)
        assert np.abs(img[..., :3] - value / 255.0).max() < 1e-12 and (img[..., 3] == 1.0).all(), op


def test_reference_no_owned_sample_is_the_background():
    vol = np.full((8, 8, 8), 200, np.uint8)
    pos, front, up, fov = CAM
    cov, vuv, g = rays(pos, front, up, fov, 8, 8)
    bg = (0.25, 0.5, 0.75)
    for op in RP.OPS:
        v, n = RP.project(vol, cov, vuv, g, STEP, op, box_min=(2.0, 2.0, 2.0), box_max=(3.0, 3.0, 3.0))
        assert (n == 0).all() and (v == 0).all()
        for lut in (None, np.tile([0.9, 0.8, 0.7, 1.0], (256, 1))):
            img = RP.finish(v, n, op, background=bg, lut=lut)
            assert np.array_equal(img, np.broadcast_to(bg + (0.0,), img.shape))
    # a pixel the cube does not cover
    cov, vuv, g = rays((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 50.0, 16, 16)
    assert not cov.all() and cov.any()
    v, n = RP.project(vol, cov, vuv, g, STEP, RP.MAX)
    assert (n[~cov] == 0).all() and (n[cov] > 0).all()


def test_reference_window_and_lookup():
    v = np.array([0.0, 0.25, 0.5, 0.75, 1.0, 0.1, 0.9])
    n = np.ones_like(v)
    img = RP.finish(v, n, RP.MAX, window=(0.25, 0.75))
    assert np.allclose(img[:, 0], [0.0, 0.0, 0.5, 1.0, 1.0, 0.0, 1.0], atol=1e-15) and img[2, 0] == 0.5
    assert np.array_equal(RP.finish(v, n, RP.MIN)[:, 0], v)                 # the identity window
    assert np.array_equal(RP.finish(v * 4, n * 4, RP.MEAN)[:, 0], v)
    k = np.arange(256) / 255.0
    lut = np.stack([k, 1 - k, np.full(256, 0.5), k], -1)                    # linear: the lookup of w is w
    bg = np.array([0.2, 0.4, 0.6])
    img = RP.finish(v, n, RP.MAX, background=bg, lut=lut)
    want = np.concatenate([v[:, None] * np.stack([v, 1 - v, np.full_like(v, 0.5)], -1) + (1 - v)[:, None] * bg, v[:, None]], -1)
    assert np.abs(img - want).max() < 1e-12


@pytest.mark.parametrize("world", [2, 3, 5])
def test_reference_slabs_combine_to_the_whole_in_any_order(world):
    vol = scene_volume()
    step = tuple(1.0 / s for s in STEPS)
    w, h = 41, 31
    for axis in (0, 1, 2):
        cam = cameras(axis)[2]
        cov, vuv, g = rays(cam[1], cam[2], cam[3], cam[4], w, h)
        for op in RP.OPS:
            whole = np.stack(RP.project(vol, cov, vuv, g, step, op), -1)
            parts = [np.stack(RP.project(vol, cov, vuv, g, step, op, 300, *slab_setup(axis, world, r)[:2]), -1)
                     for r in range(world)]
            assert sum((p[..., 1] > 0).any() for p in parts) >= 2           # more than one slab is seen
            perms = list(itertools.permutations(range(world)))
            for perm in perms[::max(1, len(perms) // 6)]:
                got = RP.combine([parts[k] for k in perm], op)
                assert np.array_equal(got[..., 1], whole[..., 1]), (axis, op, perm)
                if op == RP.MEAN:
                    assert np.abs(got[..., 0] - whole[..., 0]).max() < 1e-10
                else:
                    assert np.array_equal(got[..., 0], whole[..., 0]), (axis, op, perm)


def test_reference_scene_leaves_enough_pixels():
    """What test_gpu_projection.py relies on for the random volumes: at most 5 % of the pixels of a camera are set aside
    by slack <= 1; the inside camera owns no sample on any ray and the oblique one has covered rays that own none."""
    from test_gpu_transfer_function import CAMERAS
    rng = np.random.default_rng(17)
    W, H, step = 72, 54, (1 / 96, 1 / 80, 1 / 64)
    for ci, (pos, front) in enumerate(CAMERAS):
        vol = rng.integers(0, 256, (24, 20, 28), dtype=np.uint8)
        vol[8:16] //= 8
        cov = rays(pos, front, (0, 1, 0), 50.0, W, H)[0]
        _, v, n, slack = RP.project_checked(vol, (pos, front, (0, 1, 0), 50.0), W, H, step, RP.MAX)
        assert (slack > 1).mean() >= 0.95, (ci, float((slack > 1).mean()))
        if ci == 2:
            assert cov.any() and (n == 0).all()
        if ci == 1:
            assert (cov & (n == 0)).any() and (n > 0).mean() > 0.5


# ---- vr_lod_select ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid,bd", [((3, 2, 5), (64, 32, 16)), ((8, 8, 15), (256, 256, 128)), ((1, 4, 2), (96, 80, 40))])
def test_select_lod_in_projection_mode_is_the_composite_cut(grid, bd):
    """Mode 4 takes the one-voxel grow of a trilinear fetch: the cuts of RENDER_COMPOSITE, for the cameras of
    test_lod_select.test_select_matches_numpy_rule."""
    from test_lod_select import _cam, _grid_ijk
    from volumerenderer_amd import _lib
    from volumerenderer_amd.render import default_params, select_lod
    ijk = _grid_ijk(grid)
    otd = int(round(math.log2(bd[0] * bd[1] * bd[2])))
    mtd = otd + 7
    culled = kept = 0
    for mode in (_lib.RENDER_COMPOSITE, _lib.RENDER_ISOSURFACE):
        rng = np.random.default_rng(1234 + sum(grid) + mode)
        for trial in range(40):
            where = trial % 3
            if where == 0:
                pos = rng.uniform(-0.45, 0.45, 3)
            elif where == 1:
                pos = rng.uniform(-2.0, 2.0, 3)
            else:
                pos = np.array([0.0, 0.0, 1.5]) + rng.uniform(-0.3, 0.3, 3)
            front = rng.normal(size=3)
            if where == 2:
                front[2] = abs(front[2]) + 0.5
            w, h = int(rng.integers(64, 1921)), int(rng.integers(64, 1081))
            cam = _cam(tuple(pos), tuple(front / np.linalg.norm(front)), fov=float(rng.uniform(10, 90)),
                       near=float(rng.uniform(0.01, 0.3)), far=float(rng.uniform(0.5, 100)))
            tol = float(rng.choice([0.25, 1.0, 4.0, 16.0]))
            cuts = {m: select_lod(cam, default_params(w, h, bd, m), bd, ijk, grid, otd, mtd, tol)
                    for m in (_lib.RENDER_COMPOSITE, _lib.RENDER_PROJECTION)}
            assert np.array_equal(cuts[_lib.RENDER_PROJECTION], cuts[_lib.RENDER_COMPOSITE]), trial
            culled += int((cuts[_lib.RENDER_PROJECTION] < 0).sum())
            kept += int((cuts[_lib.RENDER_PROJECTION] >= 0).sum())
    assert culled > 0 and kept > 0


# ---- composite_sort_last_proj over gloo --------------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_partials(world, w, h, op):
    """(v, n, 0, 0) per rank: about a third of the pixels own nothing on a rank."""
    rng = np.random.default_rng(200 + world + op)
    n = rng.integers(0, 40, (world, h, w)) * (rng.random((world, h, w)) > 0.35)
    v = rng.uniform(0.0, 1.0, (world, h, w)) * (n if op == RP.MEAN else 1)
    parts = np.zeros((world, h, w, 4), np.float32)
    parts[..., 0] = np.where(n > 0, v, 0.0)
    parts[..., 1] = n
    return parts


GLOO_WINDOW, GLOO_BG = (0.1, 0.9), (0.2, 0.4, 0.6)


def _numpy_combine(parts, proj):
    import torch
    p = parts.numpy().astype(np.float64)
    c = RP.combine(p[..., :2], proj.op)
    return torch.from_numpy(RP.finish(c[..., 0], c[..., 1], proj.op, proj.window, proj.background).astype(np.float32))


def _gloo_worker(rank, world, port, w, h, op, result_path):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from volumerenderer_amd import distributed as D
        from volumerenderer_amd import render as R
        proj = R.Projection(op, GLOO_WINDOW, GLOO_BG, device="cpu")
        part = torch.from_numpy(_gloo_partials(world, w, h, op)[rank])
        frame = D.composite_sort_last_proj(part, proj, combine=_numpy_combine)
        assert (frame is None) == (rank != 0)
        if rank == 0:
            np.save(result_path, frame.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world,op", [(2, RP.MAX), (3, RP.MIN), (3, RP.MEAN)])
def test_sort_last_proj_over_gloo_equals_the_combine_of_the_stacked_partials(world, op, tmp_path):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    w, h = 37, 23                           # uneven tiles
    out = str(tmp_path / "frame.npy")
    mp.spawn(_gloo_worker, args=(world, _free_port(), w, h, op, out), nprocs=world, join=True)
    got = np.load(out)
    parts = _gloo_partials(world, w, h, op).astype(np.float64)
    c = RP.combine(parts[..., :2], op)
    assert (c[..., 1] == 0).any() and (c[..., 1] > 0).any()
    want = RP.finish(c[..., 0], c[..., 1], op, GLOO_WINDOW, GLOO_BG).astype(np.float32)
    assert np.array_equal(got, want)


# ---- the C++ surface ---------------------------------------------------------------------------------------------------
def compile_example(out_dir):
    """examples/projection.cpp (vrhip::Projector) built with g++ against libvrhip.so; returns the program's path."""
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(str(out_dir), "projection")
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "projection.cpp"), "-L" + lib, "-lvrhip", "-Wl,-rpath," + lib,
                           "-o", exe])
    return exe


def test_cpp_example_compiles_and_is_loud_without_a_gpu(L, tmp_path):
    exe = compile_example(tmp_path)
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    r = subprocess.run([exe], capture_output=True, text=True)
    if n.value > 0:
        assert r.returncode == 0 and "fnv1a64" in r.stdout, r.stdout + r.stderr
    else:
        assert r.returncode != 0 and "no usable HIP device" in (r.stdout + r.stderr)
