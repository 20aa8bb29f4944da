"""Sort-last colour partials on the GPU: vr_raycast_tf_partial (unlit and lit), vr_composite_over_tf / _finish_tf /
_slabs_tf and vr_compositor_composite_tf, on ONE GPU through the loopback transport of test_gpu_compositor.py.

Exact (bit for bit):
  1. a full-box partial finished by vr_composite_finish_tf, and by vr_composite_slabs_tf with one slab, is the frame of
     vr_raycast_tf / vr_raycast_tf_shaded;
  2. the partial is identical with and without a skip grid, and the pool partial to the dense one;
  4. rank 0's frame from vr_compositor_composite_tf equals ONE vr_composite_slabs_tf over the stacked partials, and the
     transport log is the direct-send exchange (test_gpu_compositor.check_log);
  5. folding the slabs pairwise with vr_composite_over_tf in view order and finishing equals vr_composite_slabs_tf.
Against the float64 references (tests/reftf.py, tests/refshade.py) of the GLOBAL volume:
  6. each rank's partial; 7. the composited frame without early exit (two halo layers lit; one is not enough);
  8. the frame with every rank's early exit on; 9. the scene can tell a wrong order.
The scene and the float64 helpers live in test_sort_last_tf_cpu.py."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays, view_dir  # noqa: E402
from test_gpu_compositor import DIMS, H, STEPS, W, WORLDS, Ranks, build_loopback, cameras, check_log, scene_volume  # noqa: E402
from test_sort_last_tf_cpu import (BACKGROUND, EXACT_CAMERA, EXACT_CASES, OPACITY_UNIT, PARTIAL_FRAC, SENSE, SHADING,  # noqa: E402
                                   TF_POINTS, TOL, combine_tf64, compile_example, ref_partial, slab_setup_halo)

pytestmark = pytest.mark.gpu

# (8): every rank's early exit on, against the single-GPU frame with its early exit on.  Let p be the sample at which the
# single pass stops: the first with the frame's transmittance T_p < 0.01.  A rank's own transmittance is never below the
# frame's, so no rank has stopped before p: up to p both frames add the same samples (TOL covers their rounding).
# Behind p a channel receives T_p * x with x = sum of w_k c_k + T' * background, where the weights w_k and T' sum to at
# most 1 and colours and background lie in [0, 1]: x is in [0, 1] whatever subset of the samples behind p is taken -- the
# single pass takes none (x = background), the ranks take those before their own exits, the true frame takes all.  So
# both the true and each computed sum of everything behind p lie in [0, 0.01], and so do the transmittances.
EARLY_EXIT_BOUND = 0.01 + TOL


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
    lb = C.CDLL(build_loopback(tmp_path_factory.mktemp("loopback_tf")))
    lb.lb_create.restype = C.c_void_p; lb.lb_create.argtypes = [C.c_int32, C.c_double]
    lb.lb_destroy.argtypes = [C.c_void_p]
    lb.lb_rank_ctx.restype = C.c_void_p; lb.lb_rank_ctx.argtypes = [C.c_void_p, C.c_int32]
    lb.lb_transport.restype = C.c_void_p
    lb.lb_log_size.argtypes = [C.c_void_p]
    lb.lb_log_entry.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    lb.lb_log_clear.argtypes = [C.c_void_p]
    lb.lb_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    return lb


@pytest.fixture(scope="module")
def volume():
    return scene_volume()


@pytest.fixture(scope="module")
def lut(vr):
    return vr.transfer_function_table(TF_POINTS)


def _cam(vr, cam):
    c = vr.default_camera()
    c.pos[:] = cam[1]; c.front[:] = cam[2]; c.up[:] = cam[3]; c.fov_deg = cam[4]
    return c


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda().reshape(-1)


def _mode(lit):
    from volumerenderer_amd import _lib
    return _lib.RENDER_SHADED if lit else _lib.RENDER_COMPOSITE


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def _slabs_tf(vr, stack, first, axis, cam, P, tf):
    from volumerenderer_amd import distributed as D
    return D._gpu_combine_tf(stack.contiguous(), first, axis, cam, P, tf)


# ---- 1: the finished full-box partial is the frame ---------------------------------------------------------------------
@pytest.mark.parametrize("w,h,lit,no_exit,unit", EXACT_CASES,
                         ids=["%dx%d-%s-ne%d-u%d" % (c[0], c[1], "lit" if c[2] else "unlit", c[3], c[4] > 0) for c in EXACT_CASES])
def test_finished_partial_is_the_frame(vr, volume, lut, w, h, lit, no_exit, unit):
    tf = vr.TransferFunction(lut, unit, BACKGROUND)
    sh = vr.Shading(*SHADING) if lit else None
    cam = _cam(vr, EXACT_CAMERA)
    P = vr.default_params(w, h, STEPS, _mode(lit))
    P.no_early_exit = no_exit
    dvol = _dev(volume)
    frame = _np(vr.raycast_tf_shaded(dvol, DIMS, cam, P, tf, sh) if lit else vr.raycast_tf(dvol, DIMS, cam, P, tf))
    part = vr.raycast_tf_partial(dvol, DIMS, cam, P, tf, sh)
    p = _np(part)
    assert (frame[..., 3] > 0.05).any() and not np.isnan(p).any()
    assert np.array_equal(_np(vr.composite_finish_tf(part, tf)), frame)
    for axis in (0, 1, 2):
        one = _slabs_tf(vr, part.reshape(1, -1, 4), 0, axis, cam, P, tf)
        assert np.array_equal(_np(one).reshape(h, w, 4), frame), axis
    # the partial itself: alpha = 1 - T, and exactly (0, 0, 0, 1) where the cube is not in the pixel
    assert np.array_equal(np.float32(1) - p[..., 3], frame[..., 3])
    cov = rays(EXACT_CAMERA[1], EXACT_CAMERA[2], EXACT_CAMERA[3], EXACT_CAMERA[4], w, h)[0]
    assert np.array_equal(p[~cov], np.broadcast_to(np.float32([0, 0, 0, 1]), p[~cov].shape))


def test_uncovered_pixels_and_an_empty_box(vr, volume, lut):
    """A camera that sees past the cube, and a box no ray enters: (0, 0, 0, 1) exactly."""
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    cam = _cam(vr, ("wide", (0.0, 0.0, -1.2), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 110.0))
    P = vr.default_params(W, H, STEPS, 0)
    dvol = _dev(volume)
    cov = rays(cam.pos[:], cam.front[:], cam.up[:], 110.0, W, H)[0]
    assert (~cov).mean() > 0.2
    p = _np(vr.raycast_tf_partial(dvol, DIMS, cam, P, tf))
    assert np.array_equal(p[~cov], np.broadcast_to(np.float32([0, 0, 0, 1]), p[~cov].shape))
    assert (p[cov][:, 3] < 1).any()
    P.box_min[:] = (0.0, 0.0, 1.5)
    P.box_max[:] = (1.0, 1.0, 2.0)
    for sh in (None, vr.Shading(*SHADING)):
        P.mode = _mode(sh is not None)
        p = _np(vr.raycast_tf_partial(dvol, DIMS, cam, P, tf, sh))
        assert np.array_equal(p, np.broadcast_to(np.float32([0, 0, 0, 1]), p.shape))


# ---- 2: skip grid and pool ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lit", [False, True], ids=["unlit", "lit"])
def test_partial_identical_with_skip_grid_and_from_the_pool(vr, lut, lit):
    import torch
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    sh = vr.Shading(*SHADING) if lit else None
    bd, grid = (16, 16, 16), (2, 2, 2)
    dims = tuple(g * b for g, b in zip(grid, bd))
    vol = scene_volume(dims, seed=5)
    vol[:16, :16] = 0                        # empty bricks: the grid has something to skip
    dvol = _dev(vol)
    cam = _cam(vr, cameras(0)[1])
    P = vr.default_params(W, H, tuple(2 * d for d in dims), _mode(lit))
    plain = _np(vr.raycast_tf_partial(dvol, dims, cam, P, tf, sh))
    assert (plain[..., 3] < 0.9).mean() > 0.05
    G = vr.build_skip_grid(dvol, dims, 4)
    vr.use_skip_grid(P, G, 4)
    assert np.array_equal(_np(vr.raycast_tf_partial(dvol, dims, cam, P, tf, sh)), plain)
    vr.use_skip_grid(P, None)
    # the pool of the same volume at full resolution: one brick per grid cell, brick b at offset b * 16^3
    ijk = np.array([(b % 2, (b // 2) % 2, b // 4) for b in range(8)], np.int64)
    bricks = vr.disassemble_bricks(dvol, bd, ijk, grid)
    from volumerenderer_amd import _lib
    table = (_lib.PoolEntry * 8)()
    for b in range(8):
        table[b].offset = b * 16 ** 3
    dtab = torch.frombuffer(bytearray(bytes(table)), dtype=torch.uint8).cuda()
    pool = bricks.reshape(-1)
    got = _np(vr.raycast_pool_tf_partial(pool, dtab, bd, grid, cam, P, tf, sh))
    assert np.array_equal(got, plain)
    PG = vr.build_skip_grid_pool(pool, dtab, bd, grid, 4)
    vr.use_skip_grid(P, PG, 4)
    assert np.array_equal(_np(vr.raycast_pool_tf_partial(pool, dtab, bd, grid, cam, P, tf, sh)), plain)


# ---- the rank driver: host threads, a stream each, the loopback handles of test_gpu_compositor.Ranks ---------------------
def render_ranks(vr, L, ranks, vol, axis, cam, tf, shading, halo, no_exit=1):
    """Every rank: vr_raycast_tf_partial of its slab (with `halo` layers) into its partial buffer on its stream, then
    vr_compositor_composite_tf at once.  Returns (rank 0's frame, the stacked partials [world][H*W][4]) after the streams
    are synchronised; the frame is NaN beforehand."""
    import torch
    world, w, h = ranks.world, ranks.w, ranks.h
    lit = shading is not None
    slabs, params, subs = [], [], []
    for r in range(world):
        bmin, bmax, org, sub, sl = slab_setup_halo(axis, world, r, halo)
        P = vr.default_params(w, h, STEPS, _mode(lit))
        P.box_min[:] = bmin; P.box_max[:] = bmax; P.global_dims[:] = DIMS; P.vol_origin[:] = org
        P.no_early_exit = no_exit
        slabs.append(_dev(vol[sl]))
        params.append(P)
        subs.append((C.c_int64 * 3)(*sub))
    parts = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(world)]
    frame = torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda")
    desc = tf.desc()
    shd = shading.desc() if lit else None
    c = _cam(vr, cam)
    torch.cuda.synchronize()            # uploads and the NaN fill are on torch's stream, the ranks use their own

    def job(r):
        def go():
            a = L.vr_raycast_tf_partial(C.c_void_p(slabs[r].data_ptr()), subs[r], C.byref(c), C.byref(params[r]),
                                        C.byref(desc), C.byref(shd) if lit else None, C.c_void_p(parts[r].data_ptr()),
                                        ranks.streams[r])
            b = L.vr_compositor_composite_tf(ranks.comps[r], C.c_void_p(parts[r].data_ptr()), axis, C.byref(c),
                                             C.byref(params[r]), C.byref(desc),
                                             C.c_void_p(frame.data_ptr()) if r == 0 else None, ranks.streams[r])
            return a, b
        return go

    rcs = ranks.run([job(r) for r in range(world)])
    ranks.sync()
    assert all(rc == (0, 0) for rc in rcs), (rcs, ranks.errors())
    return frame.cpu().numpy(), torch.stack([p.reshape(-1, 4) for p in parts], 0)


def run_case(vr, L, LB, vol, world, axis, cam, tf, shading, halo, no_exit=1, log=True):
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        frame, stack = render_ranks(vr, L, ranks, vol, axis, cam, tf, shading, halo, no_exit)
        if log:
            if world > 1:
                check_log(ranks.log(), world, W, H)
            else:
                assert ranks.log() == []
        assert ranks.errors() == ""
    finally:
        ranks.close()
    assert not np.isnan(frame).any()
    return frame, stack


# ---- 4 and 5: the exchange is lossless; pairwise folds are the slab kernel ---------------------------------------------
CASES = [(wd, ax, cam[0]) for wd in WORLDS for ax in (0, 1, 2) for cam in cameras(ax)]


@pytest.mark.parametrize("world,axis,cam_name", CASES, ids=["w%d-ax%d-%s" % c for c in CASES])
def test_compositor_exchange_tf(vr, L, LB, volume, lut, world, axis, cam_name):
    import torch
    cam = [c for c in cameras(axis) if c[0] == cam_name][0]
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    frame, stack = run_case(vr, L, LB, volume, world, axis, cam, tf, None, 1)
    c = _cam(vr, cam)
    P = vr.default_params(W, H, STEPS, 0)
    one = _np(_slabs_tf(vr, stack, 0, axis, c, P, tf)).reshape(H, W, 4)
    assert np.array_equal(one, frame), "exchange or tile offset bug"
    asc = view_dir(cam, W, H, axis) >= 0
    assert (asc.any() and not asc.all()) == (cam_name in ("inside", "orbit30")), cam_name
    if cam_name in ("minus", "plus"):
        # 5. the view order is uniform over the frame: fold in that order with vr_composite_over_tf, then finish
        order = list(range(world)) if asc.all() else list(range(world - 1, -1, -1))
        acc = stack[order[0]].clone()
        for k in order[1:]:
            vr.composite_over_tf(acc, stack[k].contiguous())
        folded = _np(vr.composite_finish_tf(acc, tf)).reshape(H, W, 4)
        assert np.array_equal(folded, frame)
        del acc
    torch.cuda.synchronize()


def test_single_rank_needs_no_transport(vr, L, LB, volume, lut):
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    cam = cameras(2)[0]
    frame, stack = run_case(vr, L, LB, volume, 1, 2, cam, tf, None, 1)
    P = vr.default_params(W, H, STEPS, 0)
    P.no_early_exit = 1
    assert np.array_equal(frame, _np(vr.raycast_tf(_dev(volume), DIMS, _cam(vr, cam), P, tf)))


# ---- 6 to 9: against float64 -------------------------------------------------------------------------------------------
# The float64 references dominate the time of these (world + 1 marches per case, lit ones with 48 more fetches per
# sample), so they run on a subset of the exchange cases that still holds every world size, every axis and every camera
# kind (sign change inside the frame included) at least once unlit, and every axis and camera kind lit.
REF_CASES = [(2, 0, "minus", False), (2, 1, "orbit30", False), (3, 1, "inside", False), (3, 2, "plus", False),
             (5, 2, "inside", False), (5, 0, "plus", False), (8, 0, "inside", False), (8, 1, "minus", False),
             (8, 2, "minus", False), (2, 2, "inside", True), (3, 0, "plus", True), (5, 1, "orbit30", True),
             (8, 1, "inside", True), (3, 2, "minus", True), (5, 0, "inside", True)]


@pytest.mark.parametrize("world,axis,cam_name,lit", REF_CASES,
                         ids=["w%d-ax%d-%s-%s" % (c[0], c[1], c[2], "lit" if c[3] else "unlit") for c in REF_CASES])
def test_partials_and_frame_against_float64(vr, L, LB, volume, lut, world, axis, cam_name, lit):
    cam = [c for c in cameras(axis) if c[0] == cam_name][0]
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    sh = vr.Shading(*SHADING) if lit else None
    halo = 2 if lit else 1
    frame, stack = run_case(vr, L, LB, volume, world, axis, cam, tf, sh, halo, no_exit=1)
    frame = frame.astype(np.float64)
    parts = _np(stack).reshape(world, H, W, 4).astype(np.float64)
    lut64 = lut.astype(np.float64)
    ray = rays(cam[1], cam[2], cam[3], cam[4], W, H)
    # 6. every rank's partial against the float64 partial of the global volume restricted to its box
    ref_parts = np.stack([ref_partial(volume, lut64, ray, lit, *slab_setup_halo(axis, world, r, halo)[:2])
                          for r in range(world)])
    for r in range(world):
        d = np.abs(parts[r] - ref_parts[r])
        print("partial rank %d: share above TOL %.5f, median %.2e, max %.2e" % (r, (d > TOL).mean(), np.median(d), d.max()))
        assert (d > TOL).mean() <= PARTIAL_FRAC and np.median(d) < 1e-5, (r, float((d > TOL).mean()), float(np.median(d)))
    # 7. the frame against the float64 frame (order-free: the whole volume, no early exit) and the single pass
    full = ref_partial(volume, lut64, ray, lit)
    asc = view_dir(cam, W, H, axis) >= 0
    ref_frame = combine_tf64(full[None], asc)
    d = np.abs(frame - ref_frame)
    print("frame against float64: max %.2e, median %.2e" % (d.max(), np.median(d)))
    assert d.max() <= TOL, float(d.max())
    c = _cam(vr, cam)
    P = vr.default_params(W, H, STEPS, _mode(lit))
    P.no_early_exit = 1
    dvol = _dev(volume)
    single = _np(vr.raycast_tf_shaded(dvol, DIMS, c, P, tf, sh) if lit else vr.raycast_tf(dvol, DIMS, c, P, tf))
    d = np.abs(frame - single)
    print("frame against the single pass: max %.2e" % d.max())
    assert d.max() <= TOL, float(d.max())
    # 8. every rank's early exit on, against the single-GPU frame with its early exit on
    early, _ = run_case(vr, L, LB, volume, world, axis, cam, tf, sh, halo, no_exit=0, log=False)
    P.no_early_exit = 0
    single = _np(vr.raycast_tf_shaded(dvol, DIMS, c, P, tf, sh) if lit else vr.raycast_tf(dvol, DIMS, c, P, tf))
    d = np.abs(early.astype(np.float64) - single)
    print("early exit on, against the single pass: max %.2e" % d.max())
    assert d.max() <= EARLY_EXIT_BOUND, float(d.max())
    # 9. the scene can tell: the float64 partials combined in the reversed order
    assert np.abs(combine_tf64(ref_parts, asc) - ref_frame).max() < 1e-9
    moved = (np.abs(combine_tf64(ref_parts, ~asc) - ref_frame).max(-1) > SENSE).mean()
    assert moved >= 0.01, moved


def test_one_halo_layer_is_not_enough_when_lit(vr, L, LB, volume, lut):
    """A lit slab with ONE halo layer clamps the gradient's outer tap at its edge: the frame leaves the reference by
    more than TOL somewhere, and with two layers it does not (the test can tell)."""
    world, axis = 5, 2
    cam = cameras(axis)[0]
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    sh = vr.Shading(*SHADING)
    ray = rays(cam[1], cam[2], cam[3], cam[4], W, H)
    asc = view_dir(cam, W, H, axis) >= 0
    ref_frame = combine_tf64(ref_partial(volume, lut.astype(np.float64), ray, True)[None], asc)
    one, _ = run_case(vr, L, LB, volume, world, axis, cam, tf, sh, 1)
    two, _ = run_case(vr, L, LB, volume, world, axis, cam, tf, sh, 2)
    d1, d2 = np.abs(one - ref_frame).max(), np.abs(two - ref_frame).max()
    print("one halo layer: max %.2e; two: max %.2e" % (d1, d2))
    assert d2 <= TOL < d1, (float(d1), float(d2))


# ---- errors and the Python surface -------------------------------------------------------------------------------------
def test_compositor_tf_refuses_bad_calls_before_any_transport_call(vr, L, LB, lut):
    import torch
    world = 3
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        part = torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda")
        c = vr.default_camera()
        desc = vr.TransferFunction(lut, 0.0, BACKGROUND).desc()

        def call(r, P, axis=1, tf=desc, frame=True):
            return L.vr_compositor_composite_tf(ranks.comps[r], C.c_void_p(part.data_ptr()), axis, C.byref(c), C.byref(P),
                                                C.byref(tf) if tf is not None else None,
                                                C.c_void_p(out.data_ptr()) if frame else None, ranks.streams[r])
        for bad in ((W + 1, H), (W, H + 1)):
            for r in range(world):
                assert call(r, vr.default_params(bad[0], bad[1], STEPS, 0), frame=r == 0) == -1
        P = vr.default_params(W, H, STEPS, 0)
        assert call(0, P, frame=False) == -1         # rank 0 needs a frame
        assert call(1, P, axis=3, frame=False) == -1
        assert call(1, P, tf=None, frame=False) == -1
        nan = vr.TransferFunction(lut, 0.0, BACKGROUND).desc()
        nan.background[1] = float("nan")
        assert call(2, P, tf=nan, frame=False) == -1
        assert ranks.log() == []
    finally:
        ranks.close()


def test_python_surface(vr, volume, lut):
    import torch
    from volumerenderer_amd import distributed as D
    tf = vr.TransferFunction(lut, OPACITY_UNIT, BACKGROUND)
    cam = _cam(vr, cameras(2)[0])
    P = vr.default_params(W, H, STEPS, 0)
    dvol = _dev(volume)
    good = vr.raycast_tf_partial(dvol, DIMS, cam, P, tf)
    # buffer checks before any C call
    with pytest.raises(ValueError):
        vr.raycast_tf_partial(dvol, (DIMS[0] + 1,) + DIMS[1:], cam, P, tf)
    with pytest.raises(ValueError):
        vr.raycast_tf_partial(dvol, DIMS, cam, P, tf, out=torch.zeros((H, W, 3), device="cuda"))
    with pytest.raises(ValueError):
        vr.raycast_tf_partial(dvol, DIMS, cam, P, tf, out=torch.zeros((H, W, 4), dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError):
        vr.raycast_tf_partial(dvol, DIMS, cam, P, "not a table")
    with pytest.raises(ValueError):
        vr.raycast_tf_partial(dvol, DIMS, cam, P, tf, shading="not a shading")
    with pytest.raises(ValueError):
        vr.composite_over_tf(good, torch.zeros((H, W + 1, 4), device="cuda"))
    with pytest.raises(ValueError):
        vr.composite_over_tf(good.transpose(0, 1), good)
    with pytest.raises(ValueError):
        vr.composite_finish_tf(good, tf, out=torch.zeros((H, W, 4), dtype=torch.float16, device="cuda"))
    with pytest.raises(ValueError):
        vr.composite_finish_tf(good, None)
    # a mode that does not match the shading is the C call's VR_ERR_INVALID
    with pytest.raises(vr.VrError):
        vr.raycast_tf_partial(dvol, DIMS, cam, P, tf, vr.Shading(*SHADING))
    # composite_sort_last_tf on one rank: the finished partial
    for bad in (good.double(), torch.zeros((H, W, 3), device="cuda")):
        with pytest.raises(ValueError):
            D.composite_sort_last_tf(bad, cam, P, tf)
    frame = D.composite_sort_last_tf(good, cam, P, tf, axis=2)
    assert np.array_equal(_np(frame), _np(vr.raycast_tf(dvol, DIMS, cam, P, tf)))
    # slab_params drives a two-slab frame end to end
    base = vr.default_params(W, H, STEPS, 0)
    base.no_early_exit = 1
    parts = []
    for r in range(2):
        Pr, local, (a0, a1) = D.slab_params(base, DIMS, 2, r, 2, 1)
        parts.append(vr.raycast_tf_partial(_dev(volume[a0:a1]), local, cam, Pr, tf).reshape(-1, 4))
    two = _np(D._gpu_combine_tf(torch.stack(parts, 0), 0, 2, cam, base, tf)).reshape(H, W, 4)
    assert np.abs(two - _np(vr.raycast_tf(dvol, DIMS, cam, base, tf))).max() <= TOL


@pytest.mark.parametrize("style", ["unlit", "lit"])
def test_cpp_example_two_slabs_equal_the_single_pass(vr, tmp_path, style):
    """examples/sort_last_tf.cpp through vrhip::SortLastTf: it exits 0 when the two-slab frame is within 2e-3 of the
    single pass and the frame shows something."""
    import subprocess
    r = subprocess.run([compile_example(tmp_path)] + (["lit"] if style == "lit" else []), capture_output=True, text=True)
    print(r.stdout, r.stderr)
    assert r.returncode == 0 and "max difference" in r.stdout, r.stdout + r.stderr
