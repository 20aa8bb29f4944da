"""Sort-last colour partials without a GPU: the argument checks of the six new C entry points (VR_ERR_INVALID before
VR_ERR_NO_DEVICE), distributed.composite_sort_last_tf over gloo with an injected float64 combine, the Python wrappers'
ValueErrors, distributed.slab_params against the hand-built slabs of test_gpu_compositor, and the scene that
test_gpu_sort_last_tf.py renders (defined here so that both files and the float64 checks share it)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays, view_dir  # noqa: E402
from refshade import march_shaded  # noqa: E402
from reftf import march_tf  # noqa: E402
from test_gpu_compositor import DIMS, STEPS, cameras, f32, scene_volume, shard, slab_setup  # noqa: E402

VR_OK, VR_ERR_INVALID, VR_ERR_NO_DEVICE = 0, -1, -2
TOL = 2e-3
PARTIAL_FRAC = 0.005
SENSE = 0.02

# ---- the scene -------------------------------------------------------------------------------------------------------
# test_gpu_compositor.scene_volume: a blob of values up to ~28, lumps of 48..230, noise below 4.  The table is blue
# and thin over the blob (0.3 at most, transparent below 5 and in the band 44..70) and orange and opaque-ish over the
# lumps: a lump in front of the blob and the blob in front of a lump give different colours, so the order matters.
TF_POINTS = [(0, 0.1, 0.3, 0.9, 0.0), (5, 0.1, 0.3, 0.9, 0.0), (28, 0.15, 0.45, 0.95, 0.3), (44, 0.15, 0.45, 0.95, 0.0),
             (70, 0.9, 0.5, 0.1, 0.0), (130, 0.95, 0.55, 0.1, 0.85), (255, 1.0, 0.9, 0.2, 0.9)]
OPACITY_UNIT = 1.0 / 40.0
BACKGROUND = (0.2, 0.4, 0.6)
SHADING = (0.3, 0.7, 0.2, 32.0, (0.0, 0.0, 0.0), 1.0 / 255.0)     # ambient, diffuse, specular, shininess, light, grad_min
STEP = tuple(1.0 / s for s in STEPS)


def slab_setup_halo(axis, world, r, halo, dims=DIMS):
    """test_gpu_compositor.slab_setup with `halo` voxel layers on each side (1 unlit, 2 lit)."""
    n = dims[axis]
    lo, hi = shard(n, r, world)
    a0, a1 = max(0, lo - halo), min(n, hi + halo)
    bmin, bmax, org = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 0, 0]
    bmin[axis] = f32(lo / n)
    bmax[axis] = f32(hi / n) if r < world - 1 else 2.0
    org[axis] = a0
    sub = list(dims)
    sub[axis] = a1 - a0
    sl = [slice(None)] * 3
    sl[2 - axis] = slice(a0, a1)
    return bmin, bmax, org, sub, tuple(sl)


def ref_partial(vol, lut, ray, lit, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), early_exit=False, unit=OPACITY_UNIT):
    """The float64 colour partial (C.r, C.g, C.b, T) of the box: the references' finished frame over a black background
    is (C, 1 - T)."""
    cov, vuv, g = ray
    if lit:
        img = march_shaded(vol, cov, vuv, g, STEP, lut, SHADING, unit, (0.0, 0.0, 0.0), early_exit=early_exit,
                           box_min=box_min, box_max=box_max)[0]
    else:
        img = march_tf(vol, cov, vuv, g, STEP, lut, unit, (0.0, 0.0, 0.0), early_exit=early_exit, box_min=box_min,
                       box_max=box_max)[0]
    img[..., 3] = 1.0 - img[..., 3]
    return img


def combine_tf64(parts, ascending, background=BACKGROUND):
    """Float64 over-combine of [world][h][w][4] colour partials, slab order ascending where `ascending`, then
    (C + T background, 1 - T)."""
    n = parts.shape[0]
    Cc = np.zeros(parts.shape[1:3] + (3,))
    T = np.ones(parts.shape[1:3])
    for k in range(n):
        p = np.where(ascending[..., None], parts[k], parts[n - 1 - k])
        Cc = Cc + T[..., None] * p[..., :3]
        T = T * p[..., 3]
    out = np.empty(parts.shape[1:])
    out[..., :3] = Cc + T[..., None] * np.asarray(background, float)
    out[..., 3] = 1.0 - T
    return out


# the frames of check (1) and (3): every combination on a camera that sees the whole cube
EXACT_FRAMES = ((1, 1), (7, 5), (83, 61))
EXACT_CASES = [(w, h, lit, no_exit, unit) for (w, h) in EXACT_FRAMES for lit in (False, True) for no_exit in (0, 1)
               for unit in (0.0, OPACITY_UNIT)]
EXACT_CAMERA = cameras(2)[0]


# ---- the C entry points: VR_ERR_INVALID before VR_ERR_NO_DEVICE ---------------------------------------------------------
NEW_SYMBOLS = ("vr_raycast_tf_partial", "vr_raycast_pool_tf_partial", "vr_composite_over_tf", "vr_composite_finish_tf",
               "vr_composite_slabs_tf", "vr_compositor_composite_tf")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def test_symbols_exported_and_declared(L):
    from volumerenderer_amd import _lib
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrhip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES and ("vr_status %s(" % name) in header, name


def test_partial_marches_reject_bad_arguments_before_the_device(L):
    import math
    from test_transfer_function_cpu import _Bufs
    from volumerenderer_amd import _lib
    from volumerenderer_amd import render as R
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)
    try:
        cam = R.default_camera()
        dims = (C.c_int64 * 3)(4, 4, 4)
        bd, grid = (C.c_int64 * 3)(4, 4, 4), (C.c_int64 * 3)(1, 1, 1)

        def tf(lut=B.lut, unit=0.0, bg=(1.0, 1.0, 1.0)):
            t = _lib.TransferFunctionDesc()
            t.lut_dev, t.opacity_unit = lut, unit
            t.background[:] = bg
            return t

        def sh(**kw):
            d = R.Shading().desc()
            for k, v in kw.items():
                if k == "light_dir":
                    d.light_dir[:] = v
                else:
                    setattr(d, k, v)
            return d

        def params(mode=0, w=8, h=8):
            return R.default_params(w, h, (4, 4, 4), mode)

        def dense(vol=B.vol, d=dims, c=cam, P=None, t=None, s=None, img=B.img, mode=None):
            P = P or params(mode if mode is not None else (3 if s is not None else 0))
            t = tf() if t is None else t
            return L.vr_raycast_tf_partial(vol, d, C.byref(c) if c is not None else None, C.byref(P) if P != "null" else None,
                                           C.byref(t) if t != "null" else None, C.byref(s) if s is not None else None, img,
                                           None)

        def pool(p=B.vol, tab=B.table, b=bd, g=grid, c=cam, P=None, t=None, s=None, img=B.img, mode=None):
            P = P or params(mode if mode is not None else (3 if s is not None else 0))
            t = tf() if t is None else t
            return L.vr_raycast_pool_tf_partial(p, tab, b, g, C.byref(c) if c is not None else None,
                                                C.byref(P) if P != "null" else None, C.byref(t) if t != "null" else None,
                                                C.byref(s) if s is not None else None, img, None)

        for lit in (None, sh()):
            # each null pointer in turn
            for kw in ({"vol": None}, {"d": None}, {"c": None}, {"P": "null"}, {"t": "null"}, {"img": None}):
                assert dense(s=lit, **kw) == VR_ERR_INVALID, kw
            for kw in ({"p": None}, {"tab": None}, {"b": None}, {"g": None}, {"c": None}, {"P": "null"}, {"t": "null"},
                       {"img": None}):
                assert pool(s=lit, **kw) == VR_ERR_INVALID, kw
            # bad extents / frame
            assert dense(s=lit, d=(C.c_int64 * 3)(4, 0, 4)) == VR_ERR_INVALID
            assert dense(s=lit, d=(C.c_int64 * 3)(4, 1 << 31, 4)) == VR_ERR_INVALID
            assert pool(s=lit, b=(C.c_int64 * 3)(4, 6, 4)) == VR_ERR_INVALID
            assert pool(s=lit, g=(C.c_int64 * 3)(1, 0, 1)) == VR_ERR_INVALID
            m = 3 if lit is not None else 0
            for w, h in ((0, 8), (8, 0), (-1, 8)):
                assert dense(s=lit, P=params(m, w, h)) == VR_ERR_INVALID and pool(s=lit, P=params(m, w, h)) == VR_ERR_INVALID
            P = params(m)
            P.max_samples = -1
            assert dense(s=lit, P=P) == VR_ERR_INVALID and pool(s=lit, P=P) == VR_ERR_INVALID
            P = params(m)
            P.vol_origin[:] = (1, 0, 0)
            assert pool(s=lit, P=P) == VR_ERR_INVALID          # a pool is the whole volume
            # a mode that does not match `shading`
            for mode in (0, 1, 2, 3, 4, -1):
                if mode != m:
                    assert dense(s=lit, mode=mode) == VR_ERR_INVALID and pool(s=lit, mode=mode) == VR_ERR_INVALID, mode
            # bad table
            for t in (tf(lut=None), tf(lut=B.lut + 4), tf(unit=-1e-6), tf(unit=math.inf), tf(unit=math.nan),
                      tf(bg=(1.0, math.nan, 1.0)), tf(bg=(math.inf, 0.0, 0.0))):
                assert dense(s=lit, t=t) == VR_ERR_INVALID and pool(s=lit, t=t) == VR_ERR_INVALID
        # bad lighting
        for bad in (sh(ambient=-0.1), sh(diffuse=math.nan), sh(specular=math.inf), sh(shininess=-1.0), sh(grad_min=-1e-9),
                    sh(light_dir=(0.0, math.nan, 0.0))):
            assert dense(s=bad) == VR_ERR_INVALID and pool(s=bad) == VR_ERR_INVALID
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback
            assert dense() == VR_ERR_NO_DEVICE and pool() == VR_ERR_NO_DEVICE
            assert dense(s=sh()) == VR_ERR_NO_DEVICE and pool(s=sh()) == VR_ERR_NO_DEVICE
    finally:
        B.free()


def test_combine_calls_reject_bad_arguments_before_the_device(L):
    import math
    from test_transfer_function_cpu import _Bufs
    from volumerenderer_amd import _lib
    from volumerenderer_amd import render as R
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)          # B.img: 8 x 8 pixels; B.lut (4 KiB) stands in for a second image of 8 x 8
    try:
        cam, P = R.default_camera(), R.default_params(8, 8, (4, 4, 4))

        def tf(bg=(0.5, 0.5, 0.5), lut=None):
            t = _lib.TransferFunctionDesc()
            t.lut_dev, t.opacity_unit = lut, 0.0
            t.background[:] = bg
            return t

        npx = 64
        assert L.vr_composite_over_tf(None, B.lut, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_over_tf(B.img, None, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_over_tf(B.img, B.lut, 0, None) == VR_ERR_INVALID
        assert L.vr_composite_over_tf(B.img, B.lut, -3, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_tf(None, C.byref(tf()), B.lut, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_tf(B.img, None, B.lut, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_tf(B.img, C.byref(tf()), None, npx, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_tf(B.img, C.byref(tf()), B.lut, 0, None) == VR_ERR_INVALID
        assert L.vr_composite_finish_tf(B.img, C.byref(tf(bg=(0.0, math.nan, 0.0))), B.lut, npx, None) == VR_ERR_INVALID

        def slabs(parts=B.img, ns=1, npix=npx, first=0, axis=2, c=cam, p=P, t=tf(), out=B.lut):
            return L.vr_composite_slabs_tf(parts, ns, npix, first, axis, C.byref(c) if c is not None else None,
                                           C.byref(p) if p is not None else None, C.byref(t) if t is not None else None,
                                           out, None)

        for kw in ({"parts": None}, {"c": None}, {"p": None}, {"t": None}, {"out": None}, {"ns": 0}, {"ns": -1}, {"npix": 0},
                   {"first": -1}, {"axis": -1}, {"axis": 3}, {"first": 1}, {"npix": 65}, {"p": R.default_params(0, 8, (4, 4, 4))},
                   {"p": R.default_params(8, 0, (4, 4, 4))}, {"t": tf(bg=(math.inf, 0.0, 0.0))}):
            assert slabs(**kw) == VR_ERR_INVALID, kw
        # a null handle is refused before anything else
        assert L.vr_compositor_composite_tf(None, B.img, 2, C.byref(cam), C.byref(P), C.byref(tf()), B.lut, None) == VR_ERR_INVALID
        if n.value == 0:
            # valid arguments (a null lut_dev is allowed here) reach the device check
            assert L.vr_composite_over_tf(B.img, B.lut, npx, None) == VR_ERR_NO_DEVICE
            assert L.vr_composite_finish_tf(B.img, C.byref(tf()), B.lut, npx, None) == VR_ERR_NO_DEVICE
            assert slabs() == VR_ERR_NO_DEVICE
    finally:
        B.free()


# ---- Python wrappers -------------------------------------------------------------------------------------------------
def test_python_combine_wrappers_raise_before_any_c_call():
    torch = pytest.importorskip("torch")
    import volumerenderer_amd as vr
    from volumerenderer_amd import render as R
    for name in ("raycast_tf_partial", "raycast_pool_tf_partial", "composite_over_tf", "composite_finish_tf"):
        assert callable(getattr(vr, name))
    tf = R.TransferFunction(R.transfer_function_table(TF_POINTS), device="cpu")
    host = torch.zeros((4, 4, 4), dtype=torch.float32)
    with pytest.raises(ValueError):
        R.composite_over_tf(host, host)                 # not on the device
    with pytest.raises(ValueError):
        R.composite_finish_tf(host, tf)
    with pytest.raises(ValueError):
        R.composite_over_tf(np.zeros((4, 4, 4), np.float32), host)
    from volumerenderer_amd import distributed as D
    with pytest.raises(ValueError):
        D.composite_sort_last_tf(host, R.default_camera(), R.default_params(4, 4, (4, 4, 4)), tf=None)


# ---- slab_params -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_slab_params_equals_the_hand_built_slabs(world):
    from volumerenderer_amd import distributed as D
    from volumerenderer_amd import render as R
    base = R.default_params(83, 61, STEPS, 0)
    base.no_early_exit = 1
    for axis in (0, 1, 2):
        for r in range(world):
            bmin, bmax, org, sub, sl = slab_setup(axis, world, r, DIMS)
            P, local, (a0, a1) = D.slab_params(base, DIMS, axis, r, world, 1)
            assert list(P.box_min) == bmin and list(P.box_max) == bmax, (axis, r)
            assert list(P.vol_origin) == org and list(P.global_dims) == list(DIMS) and list(local) == sub
            assert sl[2 - axis] == slice(a0, a1)
            assert (P.width, P.height, P.no_early_exit, P.mode, P.max_samples) == (83, 61, 1, 0, base.max_samples)
            assert list(P.step_size) == list(base.step_size)
            # two layers: the same box, a wider store
            P2, local2, (b0, b1) = D.slab_params(base, DIMS, axis, r, world, 2)
            want = slab_setup_halo(axis, world, r, 2)
            assert list(P2.box_min) == want[0] and list(P2.box_max) == want[1] and list(P2.vol_origin) == want[2]
            assert list(local2) == want[3] and want[4][2 - axis] == slice(b0, b1)
    assert list(base.box_max) == [1.0, 1.0, 1.0] and list(base.global_dims) == [0, 0, 0]      # the argument is not touched
    for bad in ((3, 0, 2, 1), (2, 2, 2, 1), (2, -1, 2, 1), (2, 0, 2, -1), (2, 0, 40, 1)):
        with pytest.raises(ValueError):
            D.slab_params(base, DIMS, *bad)


# ---- composite_sort_last_tf over gloo ----------------------------------------------------------------------------------
def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _gloo_partials(world, w, h):
    rng = np.random.default_rng(100 + world)
    parts = rng.uniform(0.0, 1.0, (world, h, w, 4))
    parts[..., :3] *= (1.0 - parts[..., 3:])        # premultiplied colours of an opacity 1 - T
    return parts.astype(np.float32)


GLOO_CAM = cameras(2)[2]           # "inside": the view order changes sign inside the frame


def _numpy_combine(w, h, axis):
    """combine(parts, first_pixel, ...) in float64 NumPy: the pixel's order from refmarch.view_dir."""
    import torch
    asc_full = (view_dir(GLOO_CAM, w, h, axis) >= 0).reshape(-1)

    def combine(parts, first_pixel, axis_, cam_, params_):
        p = parts.numpy().astype(np.float64)
        asc = asc_full[first_pixel:first_pixel + p.shape[1]]
        return torch.from_numpy(combine_tf64(p[:, None], asc[None])[0].astype(np.float32))
    return combine


def _gloo_worker(rank, world, port, w, h, result_path):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from volumerenderer_amd import distributed as D
        from volumerenderer_amd import render as R
        tf = R.TransferFunction(R.transfer_function_table(TF_POINTS), OPACITY_UNIT, BACKGROUND, device="cpu")
        cam = R.default_camera()
        cam.pos[:] = GLOO_CAM[1]; cam.front[:] = GLOO_CAM[2]; cam.up[:] = GLOO_CAM[3]; cam.fov_deg = GLOO_CAM[4]
        P = R.default_params(w, h, STEPS, 0)
        part = torch.from_numpy(_gloo_partials(world, w, h)[rank])
        frame = D.composite_sort_last_tf(part, cam, P, tf, axis=2, combine=_numpy_combine(w, h, 2))
        assert (frame is None) == (rank != 0)
        if rank == 0:
            np.save(result_path, frame.numpy())
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_sort_last_tf_over_gloo_equals_the_combine_of_the_stacked_partials(world, tmp_path):
    pytest.importorskip("torch")
    import torch.multiprocessing as mp
    w, h = 37, 23                           # uneven tiles
    out = str(tmp_path / "frame.npy")
    mp.spawn(_gloo_worker, args=(world, _free_port(), w, h, out), nprocs=world, join=True)
    got = np.load(out)
    asc = view_dir(GLOO_CAM, w, h, 2) >= 0
    assert asc.any() and not asc.all()      # both orders occur in the frame
    want = combine_tf64(_gloo_partials(world, w, h).astype(np.float64), asc).astype(np.float32)
    assert np.array_equal(got, want)


# ---- the scene of test_gpu_sort_last_tf.py, in float64 -----------------------------------------------------------------
def test_float64_partials_compose_to_the_frame_and_order_matters():
    """Combining the float64 partials of the slabs in view order is the frame (to rounding); reversed it is not."""
    from volumerenderer_amd.render import transfer_function_table
    lut = transfer_function_table(TF_POINTS).astype(np.float64)
    vol = scene_volume()
    w, h, world, axis = 83, 61, 3, 1
    for lit in (False, True):
        cam = cameras(axis)[2 if lit else 0]
        ray = rays(cam[1], cam[2], cam[3], cam[4], w, h)
        parts = np.stack([ref_partial(vol, lut, ray, lit, *slab_setup(axis, world, r)[:2]) for r in range(world)])
        full = ref_partial(vol, lut, ray, lit)
        asc = view_dir(cam, w, h, axis) >= 0
        assert np.abs(combine_tf64(parts, asc) - combine_tf64(full[None], asc)).max() < 1e-12
        moved = (np.abs(combine_tf64(parts, ~asc) - combine_tf64(parts, asc)).max(-1) > SENSE).mean()
        assert moved >= 0.01, moved
        empty = ~ray[0]
        assert np.array_equal(parts[:, empty], np.broadcast_to([0.0, 0.0, 0.0, 1.0], parts[:, empty].shape))


@pytest.mark.parametrize("world,axis,cam_k", [(8, 0, 0), (5, 1, 2), (3, 2, 1)])
def test_float32_positions_stay_inside_the_partial_share(world, axis, cam_k):
    """The bound of check (6) before it is relied on: with the march's positions accumulated in float32 (what the
    kernel does) a sample within rounding of a slab plane may change owner; the share of partial channels this moves by
    more than TOL stays within PARTIAL_FRAC for the scene."""
    from volumerenderer_amd.render import transfer_function_table
    lut = transfer_function_table(TF_POINTS).astype(np.float64)
    vol = scene_volume()
    w, h = 83, 61
    cam = cameras(axis)[cam_k]
    cov, vuv, g = rays(cam[1], cam[2], cam[3], cam[4], w, h)
    for r in range(world):
        bmin, bmax = slab_setup(axis, world, r)[:2]
        p64 = ref_partial(vol, lut, (cov, vuv, g), False, bmin, bmax)
        p32 = ref_partial32(vol, lut, (cov, vuv, g), bmin, bmax)
        d = np.abs(p32 - p64)
        assert (d > TOL).mean() <= PARTIAL_FRAC and np.median(d) < 1e-5, (r, float((d > TOL).mean()), float(d.max()))


def ref_partial32(vol, lut, ray, box_min, box_max, max_samples=300):
    """ref_partial (unlit, no early exit) with the kernel's position arithmetic: st = float32(g * step) and
    pos = float32(pos + st), compared with the float32 box; the sample and the compositing stay float64."""
    from refmarch import inside, tex3d
    from reftf import lookup
    cov, vuv, g = ray
    st = (g.astype(np.float32) * np.asarray(STEP, np.float32)).astype(np.float32)
    L = np.linalg.norm(st.astype(np.float64), axis=-1)
    ex = L / OPACITY_UNIT
    bmin, bmax = np.asarray(box_min, np.float32), np.asarray(box_max, np.float32)
    pos = vuv.astype(np.float32)
    live = cov.copy()
    Cc = np.zeros(cov.shape + (3,))
    T = np.ones(cov.shape)
    for _ in range(max_samples):
        pos = (pos + st).astype(np.float32)
        live = live & inside(pos.astype(np.float64))
        if not live.any():
            break
        take = live & ((pos >= bmin) & (pos < bmax)).all(-1)
        s = np.where(take, tex3d(vol, np.where(take[..., None], pos.astype(np.float64), 0.5)), 0.0)
        e = lookup(lut, s)
        a = np.where(take, 1.0 - (1.0 - e[..., 3]) ** ex, 0.0)
        Cc = Cc + (T * a)[..., None] * e[..., :3]
        T = T * (1.0 - a)
    return np.concatenate([Cc, T[..., None]], -1)


# ---- the C++ surface ---------------------------------------------------------------------------------------------------
def compile_example(out_dir):
    """examples/sort_last_tf.cpp (vrhip::SortLastTf) built with g++ against libvrhip.so; returns the program's path."""
    import subprocess
    import __graft_entry__ as g
    g.build()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = os.path.join(str(out_dir), "sort_last_tf")
    lib = os.path.join(root, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(root, "include"),
                           os.path.join(root, "examples", "sort_last_tf.cpp"), "-L" + lib, "-lvrhip", "-Wl,-rpath," + lib,
                           "-o", exe])
    return exe


def test_cpp_example_compiles_and_is_loud_without_a_gpu(L, tmp_path):
    import subprocess
    exe = compile_example(tmp_path)
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    r = subprocess.run([exe], capture_output=True, text=True)
    if n.value > 0:
        assert r.returncode == 0, r.stdout + r.stderr
    else:
        assert r.returncode != 0 and "no usable HIP device" in (r.stdout + r.stderr)
