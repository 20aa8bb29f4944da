"""Intensity projections on the GPU (vr_raycast_projection & co.; the rule is in include/vrhip.h): MIP, MinIP and the
mean along the ray against the float64 reference of tests/refproject.py; frames and partials bit-identical with and
without the skip grid and from the pool; finish(partial) == frame and pairwise folds ==
the slab call; slabs of 2 to 8 ranks along every axis equal to the single-GPU frame bit for bit (MAX, MIN) or within two
summation orders (MEAN); vr_compositor_composite_proj through the loopback transport of test_gpu_compositor.py; the
viewer and the C++ example."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refproject as RP  # noqa: E402
from test_gpu_compositor import DIMS, H, STEPS, W, WORLDS, Ranks, build_loopback, cameras, check_log, scene_volume  # noqa: E402
from test_gpu_transfer_function import BD, CAMERAS, GRID, _sparse_volume, pool_set, smooth_table  # noqa: E402,F401
from test_gpu_transfer_function import DIMS as POOL_DIMS  # noqa: E402

pytestmark = pytest.mark.gpu
TOL = 2e-3                          # the project's frame tolerance (test_gpu_compositor.TOL)
OPS = ("max", "min", "mean")


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
    lb = C.CDLL(build_loopback(tmp_path_factory.mktemp("loopback_proj")))
    lb.lb_create.restype = C.c_void_p; lb.lb_create.argtypes = [C.c_int32, C.c_double]
    lb.lb_destroy.argtypes = [C.c_void_p]
    lb.lb_rank_ctx.restype = C.c_void_p; lb.lb_rank_ctx.argtypes = [C.c_void_p, C.c_int32]
    lb.lb_transport.restype = C.c_void_p
    lb.lb_log_size.argtypes = [C.c_void_p]
    lb.lb_log_entry.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    lb.lb_log_clear.argtypes = [C.c_void_p]
    lb.lb_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    return lb


def _cam(vr, pos, front, fov=50.0, up=(0.0, 1.0, 0.0)):
    cam = vr.default_camera()
    f = np.array(front, float) / np.linalg.norm(front)
    cam.pos[:], cam.front[:], cam.up[:], cam.fov_deg = pos, tuple(float(v) for v in f), up, fov
    return cam


def _scene_cam(vr, cam):
    return _cam(vr, cam[1], cam[2], cam[4], cam[3])


def _dev(vol):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda().reshape(-1)


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _params(vr, w, h, steps, max_samples=300):
    from volumerenderer_amd import _lib
    P = vr.default_params(w, h, steps, _lib.RENDER_PROJECTION)
    P.max_samples = max_samples
    return P


# ---- against float64 -------------------------------------------------------------------------------------------------
def _random_scene(ci):
    """The volume of camera ci in test_gpu_transfer_function.test_random_volumes_match_float64_reference's scene."""
    rng = np.random.default_rng(17)
    vol = None
    for _ in range(ci + 1):
        vol = rng.integers(0, 256, (24, 20, 28), dtype=np.uint8)
        vol[8:16] //= 8
    return vol


SCENE_W, SCENE_H, SCENE_STEP = 72, 54, (1 / 96, 1 / 80, 1 / 64)


@pytest.mark.parametrize("ci", [0, 1])
def test_one_sample_per_ray_is_the_fetch(vr, ci):
    """max_samples = 1: MAX, MIN and MEAN all return the one fetched value, and n is 1 where it is owned."""
    pos, front = CAMERAS[ci]
    vol = _random_scene(ci)
    cam = _cam(vr, pos, front)
    P = _params(vr, SCENE_W, SCENE_H, (96, 80, 64), 1)
    ref, v, n, slack = RP.project_checked(vol, (pos, front, (0, 1, 0), 50.0), SCENE_W, SCENE_H, SCENE_STEP, RP.MAX,
                                          max_samples=1)
    sel = slack > 1
    assert sel.mean() >= 0.95 and (n[sel] == 1).mean() > 0.5 and set(np.unique(n)) <= {0.0, 1.0}
    parts = {}
    for op in OPS:
        proj = vr.Projection(op)
        part = _np(vr.raycast_projection_partial(_dev(vol), (28, 20, 24), cam, P, proj)).astype(np.float64)
        frame = _np(vr.raycast_projection(_dev(vol), (28, 20, 24), cam, P, proj)).astype(np.float64)
        assert np.array_equal(part[..., 1][sel], n[sel]) and (part[..., 2:] == 0).all()
        d = np.abs(part[..., 0] - v)[sel]
        print(ci, op, "one sample: max", d.max(), "median", np.median(d))
        assert d.max() <= TOL and np.median(d) < 1e-5
        d = np.abs(frame - ref)[sel]
        assert d.max() <= TOL and np.median(d) < 1e-5
        parts[op] = part
    assert np.array_equal(parts["max"], parts["min"]) and np.array_equal(parts["max"], parts["mean"])


@pytest.mark.parametrize("ci", [0, 1, 2])
def test_random_volumes_match_float64_reference(vr, ci):
    pos, front = CAMERAS[ci]
    vol = _random_scene(ci)
    cam = _cam(vr, pos, front)
    P = _params(vr, SCENE_W, SCENE_H, (96, 80, 64))
    rng = np.random.default_rng(5)
    lut = vr.transfer_function_table(smooth_table(rng))
    bg = (0.2, 0.4, 0.6)
    cases = [(op, (0.0, 1.0), None) for op in OPS] + [("max", (0.1, 0.9), lut)]
    for op, window, table in cases:
        proj = vr.Projection(op, window, bg, table)
        ref, v, n, slack = RP.project_checked(vol, (pos, front, (0, 1, 0), 50.0), SCENE_W, SCENE_H, SCENE_STEP, proj.op, window,
                                              bg, None if table is None else table.astype(np.float64))
        sel = slack > 1
        assert sel.mean() >= 0.95, (ci, float(sel.mean()))          # at most 5 % of the pixels are set aside
        got = _np(vr.raycast_projection(_dev(vol), (28, 20, 24), cam, P, proj)).astype(np.float64)
        part = _np(vr.raycast_projection_partial(_dev(vol), (28, 20, 24), cam, P, proj)).astype(np.float64)
        assert np.array_equal(part[..., 1][sel], n[sel]), (ci, op)    # the count is exact
        d = np.abs(got - ref)[sel]
        print(ci, op, "colour" if table is not None else "grey", "max", d.max(), "median", np.median(d))
        assert d.max() <= TOL and np.median(d) < 1e-5, (ci, op, float(d.max()), float(np.median(d)))
        if ci == 2:         # inside the cube: no ray owns a sample
            assert (n == 0).all() and np.array_equal(got, np.broadcast_to(np.float32(bg + (0.0,)), got.shape))
            assert (part == 0).all()
        else:
            assert (n[sel] > 0).mean() > 0.5 and (got[..., 3] > 0).mean() > 0.5
        if ci == 1:         # covered rays that own no sample are the background too
            from refmarch import rays
            cov = rays(pos, front, (0, 1, 0), 50.0, SCENE_W, SCENE_H)[0]
            empty = cov & (n == 0) & sel
            assert empty.any() and np.array_equal(got[empty], np.broadcast_to(np.float32(bg + (0.0,)), got[empty].shape))


# ---- the skip grid, the pool ----------------------------------------------------------------------
def _plateau_volume():
    """A ramp rising along z in plateaus of eight voxels (cells with equal bounds: the rule's first branch), each
    plateau's last layer a ramp along x (unequal bounds: the second)."""
    X, Y, Z = 96, 80, 72
    vol = np.empty((Z, Y, X), np.uint8)
    vol[:] = (20 + 24 * (np.arange(Z) // 8))[:, None, None]
    vol[7::8] = np.minimum(vol[7::8] + (np.arange(X) // 4)[None, None, :], 255)
    return vol


SKIP_CAMERAS = [CAMERAS[0], ((0.05, -0.1, 0.85), (0.0, 0.1, -1.0))]       # oblique from -z; from +z, down the ramp


@pytest.mark.parametrize("cell", [4, 8, 16])
@pytest.mark.parametrize("which", ["sparse", "plateaus"])
def test_skip_grid_bit_identical(vr, which, cell):
    import torch
    vol = _sparse_volume() if which == "sparse" else _plateau_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    grid = vr.build_skip_grid(dvol, (X, Y, Z), cell)
    for op in OPS:
        proj = vr.Projection(op, (0.05, 0.95), (0.3, 0.1, 0.0))
        for pos, front in SKIP_CAMERAS:
            cam = _cam(vr, pos, front)
            P = _params(vr, 160, 100, (256, 256, 128))
            frame = vr.raycast_projection(dvol, (X, Y, Z), cam, P, proj)
            part = vr.raycast_projection_partial(dvol, (X, Y, Z), cam, P, proj)
            assert (part[..., 1] > 100).float().mean() > 0.1           # long rays
            Pg = _params(vr, 160, 100, (256, 256, 128))
            vr.use_skip_grid(Pg, grid, cell)
            assert torch.equal(vr.raycast_projection(dvol, (X, Y, Z), cam, Pg, proj), frame), (op, pos)
            assert torch.equal(vr.raycast_projection_partial(dvol, (X, Y, Z), cam, Pg, proj), part), (op, pos)


def test_pool_equals_dense_and_skip_grid(vr, pool_set):  # noqa: F811
    import torch
    bs, ijk = pool_set
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    plans = [np.full(8, M, np.int32), np.array([M, D - 3, -1, D - 1, M - 1, -1, D - 6, M], np.int32)]
    for cuts in plans:
        buf = torch.zeros(bs.num_bricks * bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=buf)
        vol = vr.assemble_bricks(buf, BD, ijk, GRID)
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        for op in OPS:
            proj = vr.Projection(op, background=(0.1, 0.2, 0.3))
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front, 40.0)
                P = _params(vr, 96, 72, BD)
                want = vr.raycast_projection(vol, POOL_DIMS, cam, P, proj)
                wantp = vr.raycast_projection_partial(vol, POOL_DIMS, cam, P, proj)
                assert torch.equal(vr.raycast_pool_projection(pool, table, BD, GRID, cam, P, proj), want), (cuts, op, pos)
                assert torch.equal(vr.raycast_pool_projection_partial(pool, table, BD, GRID, cam, P, proj), wantp)
                for cell in (4, 8):
                    Pp = _params(vr, 96, 72, BD)
                    vr.use_skip_grid(Pp, vr.build_skip_grid_pool(pool, table, BD, GRID, cell), cell)
                    assert torch.equal(vr.raycast_pool_projection(pool, table, BD, GRID, cam, Pp, proj), want), (cuts, op, pos, cell)
                    assert torch.equal(vr.raycast_pool_projection_partial(pool, table, BD, GRID, cam, Pp, proj), wantp)


def test_pool_rejects_bad_params(vr, pool_set):  # noqa: F811
    bs, ijk = pool_set
    pool, table = bs.decode_lod_pool(np.full(8, bs.info(0)["max_tree_depth"], np.int32), ijk, GRID)
    proj = vr.Projection()
    P = _params(vr, 32, 32, BD)
    P.vol_origin[:] = (1, 0, 0)
    with pytest.raises(vr.VrError):
        vr.raycast_pool_projection(pool, table, BD, GRID, vr.default_camera(), P, proj)
    P = _params(vr, 32, 32, BD)
    P.global_dims[:] = (64, 64, 32)
    with pytest.raises(vr.VrError):
        vr.raycast_pool_projection_partial(pool, table, BD, GRID, vr.default_camera(), P, proj)
    with pytest.raises(vr.VrError):        # the compositor's mode
        vr.raycast_pool_projection(pool, table, BD, GRID, vr.default_camera(), vr.default_params(32, 32, BD), proj)
    with pytest.raises(ValueError):
        vr.raycast_pool_projection(pool, table, BD, GRID, vr.default_camera(), _params(vr, 32, 32, BD), None)


# ---- finish and folds ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volume():
    return scene_volume()


def _slabs(vr, stack, proj):
    from volumerenderer_amd import distributed as D
    return D._gpu_combine_proj(stack.contiguous(), proj)


def _slab_partials(vr, vol, axis, world, cam, proj, halo=1):
    """The stacked partials [world][H*W][4] of the slabs of test_gpu_compositor's scene, laid out by slab_params."""
    import torch
    from volumerenderer_amd import distributed as D
    base = _params(vr, W, H, STEPS)
    parts = []
    for r in range(world):
        P, local, (a0, a1) = D.slab_params(base, DIMS, axis, r, world, halo)
        sl = [slice(None)] * 3
        sl[2 - axis] = slice(a0, a1)
        parts.append(vr.raycast_projection_partial(_dev(vol[tuple(sl)]), local, cam, P, proj).reshape(-1, 4))
    return torch.stack(parts, 0)


def test_finish_of_the_partial_is_the_frame_and_folds_are_the_slab_call(vr, volume):
    import torch
    lut = vr.transfer_function_table(smooth_table(np.random.default_rng(6)))
    dvol = _dev(volume)
    for axis in (0, 2):
        for cam4 in cameras(axis):
            cam = _scene_cam(vr, cam4)
            for op, window, table in [(o, (0.0, 1.0), None) for o in OPS] + [("max", (0.02, 0.6), lut), ("mean", (0.0, 0.3), lut)]:
                proj = vr.Projection(op, window, (0.2, 0.4, 0.6), table)
                P = _params(vr, W, H, STEPS)
                frame = vr.raycast_projection(dvol, DIMS, cam, P, proj)
                part = vr.raycast_projection_partial(dvol, DIMS, cam, P, proj)
                assert (part[..., 1] > 0).any()
                assert torch.equal(vr.composite_finish_proj(part, proj), frame), (axis, cam4[0], op)
                assert torch.equal(_slabs(vr, part.reshape(1, -1, 4), proj).reshape(H, W, 4), frame)
                # pairwise folds in ascending order, then the finish: the slab call, MEAN included
                stack = _slab_partials(vr, volume, axis, 5, cam, proj)
                acc = stack[0].clone()
                for k in range(1, 5):
                    vr.composite_combine_proj(acc, stack[k].contiguous(), proj)
                assert torch.equal(vr.composite_finish_proj(acc, proj), _slabs(vr, stack, proj)), (axis, cam4[0], op)


# ---- slabs: exact across ranks -----------------------------------------------------------------------------------------
SLAB_CASES = [(wd, ax) for wd in WORLDS for ax in (0, 1, 2)]


@pytest.mark.parametrize("world,axis", SLAB_CASES, ids=["w%d-ax%d" % c for c in SLAB_CASES])
def test_slabs_equal_the_single_gpu_frame(vr, volume, world, axis):
    import torch
    dvol = _dev(volume)
    rng = np.random.default_rng(world * 3 + axis)
    u = 2.0 ** -24
    N = 300
    g = (N - 1) * u / (1 - (N - 1) * u)
    told = 0
    for cam4 in cameras(axis):
        cam = _scene_cam(vr, cam4)
        P = _params(vr, W, H, STEPS, N)
        for op in OPS:
            proj = vr.Projection(op)
            frame = vr.raycast_projection(dvol, DIMS, cam, P, proj)
            part = vr.raycast_projection_partial(dvol, DIMS, cam, P, proj).reshape(-1, 4)
            stack = _slab_partials(vr, volume, axis, world, cam, proj)
            assert int(((stack[..., 1] > 0).sum(0) > 1).sum()) > 0                # rays cross slabs
            orders = [list(range(world)), [int(k) for k in rng.permutation(world)], list(range(world - 1, -1, -1))]
            for order in orders:
                acc = stack[order[0]].clone()
                for k in order[1:]:
                    vr.composite_combine_proj(acc, stack[k].contiguous(), proj)
                got = _slabs(vr, stack[order], proj).reshape(H, W, 4)
                assert torch.equal(acc[:, 1], part[:, 1]), (cam4[0], op, order)           # n is exact for every op
                if op != "mean":
                    assert torch.equal(acc, part), (cam4[0], op, order)
                    assert torch.equal(got, frame), (cam4[0], op, order)
                else:
                    d = (got - frame).abs().max().item()
                    assert d <= 2 * g + 2 * u, (cam4[0], order, d)
            if op == "max":
                # one halo layer is needed: without it a slab's edge samples read clamped voxels
                bare = _slabs(vr, _slab_partials(vr, volume, axis, world, cam, proj, halo=0), proj).reshape(H, W, 4)
                told += int(not torch.equal(bare, frame))
    assert told >= 1, "the scene cannot tell a missing halo layer"


# ---- the compositor ----------------------------------------------------------------------------------------------------
def _render_ranks(vr, L, ranks, vol, axis, cam, proj, also_grey_and_tf=False):
    """Every rank: vr_raycast_projection_partial of its slab on its stream, then vr_compositor_composite_proj at once
    (also_grey_and_tf: a grey and a colour frame through the same handle first).  Returns (frames, stacked projection
    partials) after the streams are synchronised; frames are NaN beforehand."""
    import torch
    from volumerenderer_amd import distributed as D
    world, w, h = ranks.world, ranks.w, ranks.h
    base = _params(vr, w, h, STEPS)
    slabs, params, subs = [], [], []
    for r in range(world):
        P, local, (a0, a1) = D.slab_params(base, DIMS, axis, r, world, 1)
        sl = [slice(None)] * 3
        sl[2 - axis] = slice(a0, a1)
        slabs.append(_dev(vol[tuple(sl)]))
        params.append(P)
        subs.append((C.c_int64 * 3)(*local))
    kinds = (["grey", "tf"] if also_grey_and_tf else []) + ["proj"]
    parts = {k: [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(world)] for k in kinds}
    frames = {k: torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for k in kinds}
    tf = vr.TransferFunction(vr.transfer_function_table([(0, 0.1, 0.3, 0.9, 0.0), (255, 1.0, 0.9, 0.2, 0.9)]), 1 / 40,
                             (0.2, 0.4, 0.6))
    tfd, pd = tf.desc(), proj.desc()
    c = cam
    torch.cuda.synchronize()            # uploads and the NaN fills are on torch's stream, the ranks use their own

    def job(r):
        def go():
            rcs = []
            vp, dst = C.c_void_p(slabs[r].data_ptr()), (lambda k: C.c_void_p(frames[k].data_ptr()) if r == 0 else None)
            for k in kinds:
                P = type(params[r]).from_buffer_copy(params[r])
                buf = C.c_void_p(parts[k][r].data_ptr())
                if k == "grey":
                    P.mode = 2
                    rcs.append(L.vr_raycast(vp, subs[r], C.byref(c), C.byref(P), buf, ranks.streams[r]))
                    rcs.append(L.vr_compositor_composite(ranks.comps[r], buf, axis, C.byref(c), C.byref(P), dst(k), ranks.streams[r]))
                elif k == "tf":
                    P.mode = 0
                    rcs.append(L.vr_raycast_tf_partial(vp, subs[r], C.byref(c), C.byref(P), C.byref(tfd), None, buf, ranks.streams[r]))
                    rcs.append(L.vr_compositor_composite_tf(ranks.comps[r], buf, axis, C.byref(c), C.byref(P), C.byref(tfd), dst(k),
                                                            ranks.streams[r]))
                else:
                    rcs.append(L.vr_raycast_projection_partial(vp, subs[r], C.byref(c), C.byref(P), C.byref(pd), buf, ranks.streams[r]))
                    rcs.append(L.vr_compositor_composite_proj(ranks.comps[r], buf, C.byref(pd), dst(k), ranks.streams[r]))
            return rcs
        return go

    rcs = ranks.run([job(r) for r in range(world)])
    ranks.sync()
    assert all(rc == 0 for x in rcs for rc in x), (rcs, ranks.errors())
    stacks = {k: torch.stack([p.reshape(-1, 4) for p in parts[k]], 0) for k in kinds}
    return frames, stacks, tf


@pytest.mark.parametrize("world", WORLDS)
def test_compositor_exchange_proj(vr, L, LB, volume, world):
    import torch
    for axis, op in ((world % 3, "max"), ((world + 1) % 3, "min"), ((world + 2) % 3, "mean")):
        cam4 = cameras(axis)[2]
        cam = _scene_cam(vr, cam4)
        proj = vr.Projection(op, (0.0, 0.8), (0.2, 0.4, 0.6))
        ranks = Ranks(vr, L, LB, world, W, H)
        try:
            frames, stacks, _ = _render_ranks(vr, L, ranks, volume, axis, cam, proj)
            check_log(ranks.log(), world, W, H)
            assert ranks.errors() == ""
        finally:
            ranks.close()
        frame = frames["proj"]
        assert not torch.isnan(frame).any()
        assert torch.equal(_slabs(vr, stacks["proj"], proj).reshape(H, W, 4), frame), "exchange or tile offset bug"
        if op != "mean":
            P = _params(vr, W, H, STEPS)
            assert torch.equal(vr.raycast_projection(_dev(volume), DIMS, cam, P, proj), frame), (world, axis, op)


def test_compositor_handle_alternates_grey_colour_and_projection(vr, L, LB, volume):
    import torch
    from volumerenderer_amd import distributed as D
    world, axis = 3, 1
    cam4 = cameras(axis)[0]
    cam = _scene_cam(vr, cam4)
    proj = vr.Projection("max")
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        frames, stacks, tf = _render_ranks(vr, L, ranks, volume, axis, cam, proj, also_grey_and_tf=True)
        check_log(ranks.log(), world, W, H, frames=3)
        assert ranks.errors() == ""
    finally:
        ranks.close()
    P = vr.default_params(W, H, STEPS, 0)
    assert torch.equal(D._gpu_combine(stacks["grey"].contiguous(), 0, axis, cam, P).reshape(H, W, 4), frames["grey"])
    assert torch.equal(D._gpu_combine_tf(stacks["tf"].contiguous(), 0, axis, cam, P, tf).reshape(H, W, 4), frames["tf"])
    assert torch.equal(_slabs(vr, stacks["proj"], proj).reshape(H, W, 4), frames["proj"])
    assert torch.equal(vr.raycast_projection(_dev(volume), DIMS, cam, _params(vr, W, H, STEPS), proj), frames["proj"])


def test_compositor_proj_refuses_bad_calls_before_any_transport_call(vr, L, LB):
    import torch
    from volumerenderer_amd import _lib
    ranks = Ranks(vr, L, LB, 2, W, H)
    try:
        part = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
        ok = vr.Projection().desc()
        bad = _lib.Projection.from_buffer_copy(ok)
        bad.op = 3
        buf = C.c_void_p(part.data_ptr())
        assert L.vr_compositor_composite_proj(ranks.comps[0], None, C.byref(ok), buf, ranks.streams[0]) == -1
        assert L.vr_compositor_composite_proj(ranks.comps[0], buf, None, buf, ranks.streams[0]) == -1
        assert L.vr_compositor_composite_proj(ranks.comps[0], buf, C.byref(ok), None, ranks.streams[0]) == -1    # rank 0's frame
        assert L.vr_compositor_composite_proj(ranks.comps[1], buf, C.byref(bad), None, ranks.streams[1]) == -1
        assert ranks.log() == []
    finally:
        ranks.close()


def test_composite_sort_last_proj_single_process(vr, volume):
    """distributed.composite_sort_last_proj without a process group: world 1 through the C-ABI compositor."""
    import torch
    from volumerenderer_amd import distributed as D
    cam = _scene_cam(vr, cameras(2)[0])
    proj = vr.Projection("min", (0.0, 0.5))
    P = _params(vr, W, H, STEPS)
    part = vr.raycast_projection_partial(_dev(volume), DIMS, cam, P, proj)
    frame = D.composite_sort_last_proj(part, proj)
    assert torch.equal(frame, vr.raycast_projection(_dev(volume), DIMS, cam, P, proj))
    with pytest.raises(ValueError):
        D.composite_sort_last_proj(part.double(), proj)
    with pytest.raises(ValueError):
        D.composite_sort_last_proj(part.reshape(-1, 4), proj)


def test_python_wrappers_refuse_bad_device_buffers(vr):
    """The wrapper checks that need a device tensor to get past the first one: all raise before any C call."""
    import torch
    from volumerenderer_amd import distributed as D
    from volumerenderer_amd import render as R
    proj = R.Projection()
    dev = torch.zeros((4, 4, 4), dtype=torch.float32, device="cuda")
    with pytest.raises(ValueError):
        R.composite_combine_proj(dev, dev.double(), proj)                       # wrong dtype
    with pytest.raises(ValueError):
        R.composite_finish_proj(torch.zeros((4, 4, 8), device="cuda")[..., ::2], proj)      # a strided partial
    with pytest.raises(ValueError):
        R.composite_finish_proj(dev, "max")                                     # not a Projection
    with pytest.raises(ValueError):
        R.raycast_projection(torch.zeros(64, dtype=torch.uint8, device="cuda"), (4, 4, 4), R.default_camera(),
                             R.default_params(4, 4, (4, 4, 4), 4), None)
    host_lut = R.Projection("max", lut=np.zeros((256, 4), np.float32), device="cpu")         # a table in host memory
    with pytest.raises(ValueError):
        R.composite_finish_proj(dev, host_lut)
    with pytest.raises(ValueError):
        D.composite_sort_last_proj(dev, host_lut)


# ---- surfaces ------------------------------------------------------------------------------------------------------
def test_viewer_draw_with_and_without_projection(vr):
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    v = HeadlessViewer(120, 90)
    v.cameraPos = np.array([0.1, -0.05, -0.9], np.float32)
    proj = vr.Projection("max", (0.0, 0.9), (0.0, 0.0, 0.1))
    P = _params(vr, 120, 90, (256, 256, 128))
    P.iso_value = float(v.currIsoVal) / 255.0
    frame = v.draw(dvol, (X, Y, Z), projection=proj)
    assert torch.equal(frame, vr.raycast_projection(dvol, (X, Y, Z), v.camera(), P, proj))
    assert (frame[..., 3] > 0).float().mean() > 0.2
    P0 = vr.default_params(120, 90, (256, 256, 128), 0, float(v.currIsoVal) / 255.0)
    assert torch.equal(v.draw(dvol, (X, Y, Z), projection=None), vr.raycast(dvol, (X, Y, Z), v.camera(), P0))
    with pytest.raises(ValueError):
        v.draw(dvol, (X, Y, Z), projection=proj, tf=vr.TransferFunction(np.zeros((256, 4), np.float32)))
    with pytest.raises(ValueError):
        v.draw(dvol, (X, Y, Z), mode=1, projection=proj)


def test_viewer_draw_lod_pool_with_projection(vr, pool_set):  # noqa: F811
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    bs, ijk = pool_set
    v = HeadlessViewer(96, 72)
    v.cameraPos = np.array([0.05, 0.0, -1.2], np.float32)
    proj = vr.Projection("mean", (0.0, 0.25))
    for skip in (0, 8):
        frame, cuts = v.draw_lod_pool(bs, ijk, GRID, pixel_tolerance=2.0, skip_cell=skip, projection=proj)
        P = _params(vr, 96, 72, BD)
        P.iso_value = float(v.currIsoVal) / 255.0
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        assert torch.equal(frame, vr.raycast_pool_projection(pool, table, BD, GRID, v.camera(), P, proj)), skip
        plain, cuts0 = v.draw_lod_pool(bs, ijk, GRID, pixel_tolerance=2.0, skip_cell=skip)
        assert np.array_equal(cuts0, cuts)          # the projection's cuts are the compositor's
        P0 = vr.default_params(96, 72, BD, 0, float(v.currIsoVal) / 255.0)
        assert torch.equal(plain, vr.raycast_pool(pool, table, BD, GRID, v.camera(), P0)), skip


def _fnv1a64(data):
    h = 14695981039346656037
    for b in data:
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return h


def test_cpp_example_hash_equals_the_python_frame(vr, tmp_path):
    """examples/projection.cpp (g++ against Projection.hpp) draws the MIP Python draws: the same FNV-1a-64."""
    from test_projection_cpu import compile_example
    exe = compile_example(tmp_path)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    words = r.stdout.split()
    assert words[:5] == ["mip", "96", "x", "64", "fnv1a64"], r.stdout
    X, Y, Z = 48, 40, 32
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    v = ((x * 5 + y * 3) ^ (z * 7)) & 255
    vol = np.where(v > 200, v, v // 16).astype(np.uint8)
    cam = _cam(vr, (0.15, -0.1, -0.8), (0.0, 0.0, 1.0), 40.0)
    P = _params(vr, 96, 64, (X, Y, Z))
    P.iso_value = 0.0
    frame = _np(vr.raycast_projection(_dev(vol), (X, Y, Z), cam, P, vr.Projection("max")))
    assert (frame[..., 0] > 0.78).mean() > 0.3      # the bright structure shows
    assert int(words[5], 16) == _fnv1a64(frame.tobytes())
