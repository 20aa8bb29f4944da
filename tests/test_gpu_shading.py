"""vr_raycast_tf_shaded / vr_raycast_pool_tf_shaded on the GPU: ambient-only frames equal vr_raycast_tf's bit for bit,
a closed form on a ramp, pixel by pixel against the float64 reference of tests/refshade.py, frames bit-identical with
and without the skip grid, pool against dense, a slab with two halo layers, unaligned volumes and tiny extents, and the
Python / C++ viewer surfaces."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays  # noqa: E402
from refshade import march_shaded_checked  # noqa: E402
from test_gpu_transfer_function import BD, CAMERAS, DIMS, GRID, _cam, _dev, _sparse_volume, _tables, smooth_table  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _params(vr, W, H, bd):
    from volumerenderer_amd import _lib
    return vr.default_params(W, H, bd, _lib.RENDER_SHADED)


def smooth_volume(rng, shape, n=6):
    """A sum of Gaussians, rounded to uint8: smooth, with gradients of a few grey levels per voxel."""
    Z, Y, X = shape
    zz, yy, xx = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(Y) + 0.5) / Y, (np.arange(X) + 0.5) / X, indexing="ij")
    v = np.zeros(shape)
    for _ in range(n):
        c = rng.uniform(0.15, 0.85, 3)
        s = rng.uniform(0.12, 0.3)
        v += rng.uniform(60, 160) * np.exp(-((xx - c[0]) ** 2 + (yy - c[1]) ** 2 + (zz - c[2]) ** 2) / (2 * s * s))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _pool_set(vr):
    full = _sparse_volume()[:64, :64, 16:80].copy()
    ijk = np.array([(i, j, k) for k in range(2) for j in range(2) for i in range(2)], np.int64)
    bricks = np.stack([full[k * 32:(k + 1) * 32, j * 32:(j + 1) * 32, i * 32:(i + 1) * 32] for i, j, k in ijk])
    bs = vr.BrickSet(8, BD, 1, 2)
    bs.build(bricks.copy())
    return bs, ijk


@pytest.fixture(scope="module")
def pool_set(vr):
    return _pool_set(vr)


# 1 ----------------------------------------------------------------------------------------------------------------------
def test_ambient_only_is_bit_identical_to_raycast_tf(vr, pool_set):
    import torch
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    amb = [vr.Shading(1.0, 0.0, 0.0, 16.0), vr.Shading(1.0, 0.0, 0.0, 0.0, (1, -2, 0.5), 0.0)]
    for ti, lut in enumerate(_tables(vr)):
        for unit, early in ((0.0, 0), (0.0, 1), (1 / 90, 0), (1 / 90, 1)):
            tf = vr.TransferFunction(lut, unit, (0.3, 0.1, 0.0))
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front)
                P = vr.default_params(120, 80, (256, 256, 128))
                P.no_early_exit = early
                want = vr.raycast_tf(dvol, (X, Y, Z), cam, P, tf)
                P.mode = 3
                for sh in amb:
                    assert torch.equal(vr.raycast_tf_shaded(dvol, (X, Y, Z), cam, P, tf, sh), want), (ti, unit, early, pos)
    bs, ijk = pool_set
    M, D = bs.info(0)["max_tree_depth"], bs.info(0)["orig_tree_depth"]
    pool, table = bs.decode_lod_pool(np.array([M, D - 3, -1, D - 1, M - 1, -1, D - 6, M], np.int32), ijk, GRID)
    for ti, lut in enumerate(_tables(vr)):
        for early in (0, 1):
            tf = vr.TransferFunction(lut, 1 / 70 if ti % 2 else 0.0)
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front, 40.0)
                P = vr.default_params(96, 72, BD)
                P.no_early_exit = early
                want = vr.raycast_pool_tf(pool, table, BD, GRID, cam, P, tf)
                P.mode = 3
                got = vr.raycast_pool_tf_shaded(pool, table, BD, GRID, cam, P, tf, amb[ti % 2])
                assert torch.equal(got, want), (ti, early, pos)


# 2 ----------------------------------------------------------------------------------------------------------------------
def test_ramp_seen_along_its_gradient_under_the_head_light(vr):
    """A ramp along z seen along z: N = +-z, V = -z, so cd = ch = 1 and c = e.rgb (ka + kd) + ks, one sample per ray."""
    X, Y, Z = 16, 16, 64
    vol = np.broadcast_to((3 * np.arange(Z)).astype(np.uint8)[:, None, None], (Z, Y, X)).copy()
    k = np.arange(256) / 255.0
    lut = np.stack([k, 1 - k, np.full(256, 0.25), np.full(256, 0.5)], -1)
    tf = vr.TransferFunction(lut, background=(0.0, 0.0, 0.0))
    sh = vr.Shading(0.2, 0.5, 0.1, 20.0)
    W, H = 32, 32
    cam = _cam(vr, (0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 6.0)
    P = _params(vr, W, H, (X, Y, Z))
    P.max_samples = 1
    got = vr.raycast_tf_shaded(_dev(vol), (X, Y, Z), cam, P, tf, sh).cpu().numpy().astype(np.float64)
    cov, vuv, g = rays((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), (0, 1, 0), 6.0, W, H)
    p = vuv + g * np.array([1 / X, 1 / Y, 1 / Z])
    s = 3 * (p[..., 2] * Z - 0.5) / 255.0
    e = np.stack([s, 1 - s, np.full_like(s, 0.25)], -1)
    # N = (0, 0, +-1), L = H = V = -g: cd = ch = |g_z|
    cz = np.abs(g[..., 2])[..., None]
    want = 0.5 * np.minimum(1.0, e * (0.2 + 0.5 * cz) + 0.1 * cz ** 20)
    assert cov.all()
    assert np.abs(got[..., :3] - want).max() < 1e-4
    assert np.abs(got[..., 3] - 0.5).max() < 1e-6


# 3 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("light,unit,early", [((0, 0, 0), 0.0, True), ((0, 0, 0), 1 / 40, False),
                                              ((0.4, 1.0, -0.6), 0.0, False), ((0.4, 1.0, -0.6), 1 / 40, True)])
def test_smooth_volumes_match_float64_reference(vr, light, unit, early):
    rng = np.random.default_rng(31 + int(unit * 1000) + 2 * early + int(light[1]))
    checked = 0
    for ci, (pos, front) in enumerate(CAMERAS):
        vol = smooth_volume(rng, (24, 20, 28))
        lut = vr.transfer_function_table(smooth_table(rng, 0.5))
        bg = tuple(rng.uniform(0, 1, 3))
        tf = vr.TransferFunction(lut, unit, bg)
        shp = (float(rng.uniform(0.1, 0.4)), float(rng.uniform(0.3, 0.8)), float(rng.uniform(0.0, 0.4)),
               float(rng.choice([1.0, 8.0, 32.0])), light, 1 / 255)
        sh = vr.Shading(*shp)
        W, H = 72, 54
        step = (1 / 96, 1 / 80, 1 / 64)
        P = _params(vr, W, H, (96, 80, 64))
        P.no_early_exit = 0 if early else 1
        got = vr.raycast_tf_shaded(_dev(vol), (28, 20, 24), _cam(vr, pos, front), P, tf, sh).cpu().numpy().astype(np.float64)
        f32 = np.float32
        shp32 = tuple(float(f32(v)) for v in shp[:4]) + (light, float(f32(shp[5])))
        ref, slack = march_shaded_checked(vol, (pos, front, (0, 1, 0), 50.0), W, H, step, lut, shp32, unit, bg,
                                          early_exit=early)
        sel = slack > 1
        assert sel.mean() > 0.75, (ci, float(sel.mean()))
        d = np.abs(got - ref)[sel]
        assert d.max() <= 2e-3, (ci, float(d.max()), float((d > 2e-3).mean()))
        checked += int(sel.sum())
        assert ci == 2 or (ref[..., 3] > 0.05).mean() > 0.3
    assert checked > 3 * 0.75 * 72 * 54


# 4 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [4, 8, 16])
def test_skip_grid_frames_bit_identical(vr, cell):
    import torch
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    grid = vr.build_skip_grid(dvol, (X, Y, Z), cell)
    for ti, lut in enumerate(_tables(vr)[:2]):          # transparent on a low range; on a band
        for unit, early in ((0.0, 0), (1 / 90, 1)):
            tf = vr.TransferFunction(lut, unit, (0.3, 0.1, 0.0))
            sh = vr.Shading(light_dir=(0.3, -1.0, 0.2)) if ti else vr.Shading()
            for pos, front in CAMERAS + [((0, 0, -0.75), (0, 0, 1))]:
                cam = _cam(vr, pos, front)
                P = _params(vr, 160, 100, (256, 256, 128))
                P.no_early_exit = early
                plain = vr.raycast_tf_shaded(dvol, (X, Y, Z), cam, P, tf, sh)
                vr.use_skip_grid(P, grid, cell)
                assert torch.equal(plain, vr.raycast_tf_shaded(dvol, (X, Y, Z), cam, P, tf, sh)), (cell, ti, unit, pos)


# 5 ----------------------------------------------------------------------------------------------------------------------
def test_pool_equals_dense(vr, pool_set):
    import torch
    bs, ijk = pool_set
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    plans = [np.full(8, M, np.int32), np.array([M, D - 3, -1, D - 1, M - 1, -1, D - 6, M], np.int32)]
    shown = 0
    for cuts in plans:
        buf = torch.zeros(bs.num_bricks * bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=buf)
        vol = vr.assemble_bricks(buf, BD, ijk, GRID)
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        for ti, lut in enumerate(_tables(vr)[:3]):
            tf = vr.TransferFunction(lut, 1 / 70 if ti % 2 else 0.0)
            sh = vr.Shading(0.2, 0.6, 0.3, 12.0, (0, 0, 0) if ti % 2 else (1, 1, -1))
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front, 40.0)
                P = _params(vr, 96, 72, BD)
                want = vr.raycast_tf_shaded(vol, DIMS, cam, P, tf, sh)
                assert torch.equal(vr.raycast_pool_tf_shaded(pool, table, BD, GRID, cam, P, tf, sh), want), (cuts, ti, pos)
                Pp = _params(vr, 96, 72, BD)
                vr.use_skip_grid(Pp, vr.build_skip_grid_pool(pool, table, BD, GRID, 8), 8)
                assert torch.equal(vr.raycast_pool_tf_shaded(pool, table, BD, GRID, cam, Pp, tf, sh), want), (cuts, ti, pos)
                shown += int(bool((want[..., 3] > 0).any()))
    assert shown >= 8


# 6 ----------------------------------------------------------------------------------------------------------------------
def test_slab_with_two_halo_layers_equals_full_volume_in_its_box(vr):
    import torch
    rng = np.random.default_rng(12)
    X, Y, Z = 40, 36, 48
    vol = smooth_volume(rng, (Z, Y, X))
    vol = (vol.astype(np.int64) + rng.integers(0, 20, vol.shape)).clip(0, 255).astype(np.uint8)
    tf = vr.TransferFunction(vr.transfer_function_table(smooth_table(rng, 0.4)), 1 / 50, (0.1, 0.2, 0.3))
    sh = vr.Shading(0.25, 0.6, 0.3, 16.0, (0.2, 0.5, -1.0))
    dfull = _dev(vol)
    for z0, z1 in ((0, 16), (16, 32), (32, 48), (10, 29)):
        lo, hi = max(z0 - 2, 0), min(z1 + 2, Z)
        slab = _dev(vol[lo:hi])
        for pos, front in CAMERAS:
            cam = _cam(vr, pos, front)
            for early in (0, 1):
                P = _params(vr, 64, 48, (X, Y, Z))
                P.no_early_exit = early
                P.box_min[:] = (0.0, 0.0, z0 / Z)
                P.box_max[:] = (1.0, 1.0, z1 / Z)
                want = vr.raycast_tf_shaded(dfull, (X, Y, Z), cam, P, tf, sh)
                P.global_dims[:] = (X, Y, Z)
                P.vol_origin[:] = (0, 0, lo)
                got = vr.raycast_tf_shaded(slab, (X, Y, hi - lo), cam, P, tf, sh)
                assert torch.equal(got, want), (z0, z1, pos, early)


# 7 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims", [(1, 9, 7), (9, 1, 7), (9, 7, 1), (2, 2, 2), (3, 5, 2), (17, 13, 11), (1, 1, 1)])
def test_unaligned_volumes_and_tiny_extents(vr, dims):
    """Volumes at byte offsets 1..15 inside a larger allocation and extents of 1, 2 and odd sizes: the dword / word row
    loads and the byte loads of the clamped edges against the reference, and the pool of the same volume."""
    import torch
    X, Y, Z = dims
    rng = np.random.default_rng(X * 100 + Y * 10 + Z)
    vol = smooth_volume(rng, (Z, Y, X), 3) if min(dims) > 2 else rng.integers(0, 256, (Z, Y, X), dtype=np.uint8)
    lut = vr.transfer_function_table(smooth_table(rng, 0.5))
    tf = vr.TransferFunction(lut, 0.0, (0.2, 0.3, 0.4))
    shp = (0.3, 0.6, 0.2, 8.0, (0.5, 0.7, -0.4), 1 / 255)
    sh = vr.Shading(*shp)
    W, H = 40, 30
    step = (1 / 24, 1 / 20, 1 / 28)
    cam = ((0.6, 0.45, -0.9), (-0.55, -0.4, 1.0))
    P = _params(vr, W, H, (24, 20, 28))
    flat = vol.reshape(-1)
    base = torch.zeros(flat.size + 64, dtype=torch.uint8, device="cuda")
    first = None
    for off in range(1, 16):
        v = base[off:off + flat.size]
        v.copy_(torch.from_numpy(flat))
        img = vr.raycast_tf_shaded(v, dims, _cam(vr, *cam), P, tf, sh)
        if first is None:
            first = img
            got = img.cpu().numpy().astype(np.float64)
            f32 = np.float32
            shp32 = tuple(float(f32(q)) for q in shp[:4]) + (shp[4], float(f32(shp[5])))
            ref, slack = march_shaded_checked(vol, (cam[0], cam[1], (0, 1, 0), 50.0), W, H, step, lut, shp32, 0.0,
                                              (0.2, 0.3, 0.4))
            sel = slack > 1
            assert sel.mean() > 0.5
            assert np.abs(got - ref)[sel].max() <= 2e-3
        else:
            assert torch.equal(img, first), off
    # the pool of the volume padded into one brick of power-of-two extents (at least 2): dense against pool
    bd = tuple(max(2, 1 << int(np.ceil(np.log2(q)))) for q in dims)
    padded = np.zeros((bd[2], bd[1], bd[0]), np.uint8)
    padded[:Z, :Y, :X] = vol
    bs = vr.BrickSet(1, bd, 1, 2)
    bs.build(padded[None].copy())
    ijk = np.zeros((1, 3), np.int64)
    M = bs.info(0)["max_tree_depth"]
    buf = torch.zeros(bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
    bs.decode_lod(np.array([M], np.int32), out=buf)
    pool, table = bs.decode_lod_pool(np.array([M], np.int32), ijk, (1, 1, 1))
    want = vr.raycast_tf_shaded(buf, bd, _cam(vr, *cam), P, tf, sh)
    assert torch.equal(vr.raycast_pool_tf_shaded(pool, table, bd, (1, 1, 1), _cam(vr, *cam), P, tf, sh), want)


def test_pool_across_brick_faces_with_small_bricks(vr):
    """Bricks of 16 x 4 x 8 voxels: every gradient neighbourhood spans 4 voxels in y, so it crosses a brick face (the
    per-voxel pool path)."""
    import torch
    rng = np.random.default_rng(77)
    bd, grid = (16, 4, 8), (2, 5, 2)
    X, Y, Z = bd[0] * grid[0], bd[1] * grid[1], bd[2] * grid[2]
    vol = smooth_volume(rng, (Z, Y, X), 4)
    ijk = np.array([(i, j, k) for k in range(grid[2]) for j in range(grid[1]) for i in range(grid[0])], np.int64)
    bricks = np.stack([vol[k * bd[2]:(k + 1) * bd[2], j * bd[1]:(j + 1) * bd[1], i * bd[0]:(i + 1) * bd[0]] for i, j, k in ijk])
    bs = vr.BrickSet(len(ijk), bd, 1, 2)
    bs.build(bricks.copy())
    M = bs.info(0)["max_tree_depth"]
    cuts = np.full(len(ijk), M, np.int32)
    cuts[::7] = -1
    buf = torch.zeros(bs.num_bricks * bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
    bs.decode_lod(cuts, out=buf)
    dense = vr.assemble_bricks(buf, bd, ijk, grid)
    pool, table = bs.decode_lod_pool(cuts, ijk, grid)
    tf = vr.TransferFunction(vr.transfer_function_table(smooth_table(rng, 0.5)))
    for pos, front in CAMERAS:
        P = _params(vr, 64, 48, bd)
        cam = _cam(vr, pos, front)
        want = vr.raycast_tf_shaded(dense, (X, Y, Z), cam, P, tf, vr.Shading())
        assert torch.equal(vr.raycast_pool_tf_shaded(pool, table, bd, grid, cam, P, tf, vr.Shading()), want), pos


# 8 ----------------------------------------------------------------------------------------------------------------------
def test_viewer_draw_with_and_without_shading(vr, pool_set):
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    tf = vr.TransferFunction.from_points([(0, 0, 0, 0, 0), (60, 0.2, 0.4, 1.0, 0.0), (200, 1.0, 0.3, 0.1, 0.6)], 1 / 128)
    sh = vr.Shading()
    v = HeadlessViewer(120, 90)
    v.cameraPos = np.array([0.1, -0.05, -0.9], np.float32)
    P = _params(vr, 120, 90, (256, 256, 128))
    P.iso_value = float(v.currIsoVal) / 255.0
    assert torch.equal(v.draw(dvol, (X, Y, Z), tf=tf, shading=sh), vr.raycast_tf_shaded(dvol, (X, Y, Z), v.camera(), P, tf, sh))
    P0 = vr.default_params(120, 90, (256, 256, 128), 0, float(v.currIsoVal) / 255.0)
    assert torch.equal(v.draw(dvol, (X, Y, Z), tf=tf, shading=None), vr.raycast_tf(dvol, (X, Y, Z), v.camera(), P0, tf))
    assert torch.equal(v.draw(dvol, (X, Y, Z)), vr.raycast(dvol, (X, Y, Z), v.camera(), P0))
    with pytest.raises(ValueError):
        v.draw(dvol, (X, Y, Z), shading=sh)
    bs, ijk = pool_set
    v = HeadlessViewer(96, 72)
    v.cameraPos = np.array([0.05, 0.0, -1.2], np.float32)
    for skip in (0, 8):
        frame, cuts = v.draw_lod_pool(bs, ijk, GRID, pixel_tolerance=2.0, skip_cell=skip, tf=tf, shading=sh)
        P = _params(vr, 96, 72, BD)
        P.iso_value = float(v.currIsoVal) / 255.0
        info = bs.info(0)
        assert np.array_equal(cuts, vr.select_lod(v.camera(), P, BD, ijk, GRID, info["orig_tree_depth"],
                                                  info["max_tree_depth"], 2.0))
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        assert torch.equal(frame, vr.raycast_pool_tf_shaded(pool, table, BD, GRID, v.camera(), P, tf, sh)), skip


def test_cpp_example_frame_equals_python(vr, tmp_path):
    """examples/shaded_volume.cpp (g++ against Viewer.hpp and TransferFunction.hpp) draws the frame Python draws."""
    from volumerenderer_amd.viewer import HeadlessViewer
    lib = os.path.join(ROOT, "volumerenderer_amd")
    exe = str(tmp_path / "shaded_volume")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "shaded_volume.cpp"), "-L" + lib, "-lvrhip",
                           "-Wl,-rpath," + lib, "-o", exe])
    out = str(tmp_path / "frame.f32")
    subprocess.check_call([exe, "render", out], timeout=120)
    got = np.fromfile(out, np.float32).reshape(64, 96, 4)
    X, Y, Z = 48, 40, 32
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    d2 = ((xx - 0.5 * X) / X) ** 2 + ((yy - 0.5 * Y) / Y) ** 2 + ((zz - 0.5 * Z) / Z) ** 2
    vol = np.rint(230.0 * np.exp(-8.0 * d2)).astype(np.uint8)
    tf = vr.TransferFunction.from_points([(0, 0.0, 0.0, 0.0, 0.0), (60, 0.9, 0.5, 0.1, 0.0), (120, 0.9, 0.6, 0.2, 0.3),
                                          (200, 1.0, 1.0, 1.0, 0.9)], 1 / 64, (0.2, 0.2, 0.25))
    sh = vr.Shading(light_dir=(0.5, 1.0, -0.5))
    v = HeadlessViewer(96, 64)
    v.cameraPos = np.array([0.15, -0.1, -0.8], np.float32)
    v.fov = 40.0
    want = v.draw(_dev(vol), (X, Y, Z), brick_dims=(X, Y, Z), tf=tf, shading=sh).cpu().numpy()
    assert np.array_equal(got, want)
    assert (want[..., 3] > 0.05).mean() > 0.1
