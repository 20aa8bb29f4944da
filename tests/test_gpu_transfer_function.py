"""vr_raycast_tf / vr_raycast_pool_tf on the GPU: the lookup in closed form, pixel by pixel against the float64
reference of tests/reftf.py, frames bit-identical with and without the skip grid, pool against dense, clip box and
sub-volume, and the Python / C++ viewer surfaces."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays  # noqa: E402
from reftf import march_tf_checked  # noqa: E402

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


def _cam(vr, pos, front, fov=50.0):
    cam = vr.default_camera()
    f = np.array(front, float) / np.linalg.norm(front)
    cam.pos[:], cam.front[:], cam.fov_deg = pos, tuple(float(v) for v in f), fov
    return cam


def _dev(vol):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda().reshape(-1)


def smooth_table(rng, alpha_max=1.0):
    """Random control points every 51 grey levels: each channel moves by at most 1 per 51 levels (slope <= 5 per unit
    of scalar)."""
    vals = np.arange(0, 256, 51)
    pts = [(int(v),) + tuple(rng.uniform(0, 1, 3)) + (float(rng.uniform(0, alpha_max)),) for v in vals]
    return pts


def test_one_sample_per_ray_is_the_lookup(vr):
    """max_samples = 1 over a ramp along x with the table (k/255, 1 - k/255, 0.5, k/255): the lookup of a linear table is
    the sample itself, so the pixel is (s (s, 1 - s, 0.5) + (1 - s) bg, s) with s the ramp at the first position."""
    X, Y, Z = 64, 16, 16
    vol = np.broadcast_to((4 * np.arange(X)).astype(np.uint8), (Z, Y, X)).copy()
    k = np.arange(256) / 255.0
    tf = vr.TransferFunction(np.stack([k, 1 - k, np.full(256, 0.5), k], -1), background=(0.2, 0.4, 0.6))
    W, H = 80, 60
    pos, front = (0.1, 0.05, -1.2), (-0.05, 0.0, 1.0)
    cam = _cam(vr, pos, front, 30.0)
    P = vr.default_params(W, H, (X, Y, Z))
    P.max_samples = 1
    got = vr.raycast_tf(_dev(vol), (X, Y, Z), cam, P, tf).cpu().numpy().astype(np.float64)
    cov, vuv, g = rays(pos, front, (0, 1, 0), 30.0, W, H)
    p = vuv + g * np.array([1 / X, 1 / Y, 1 / Z])
    xf = p[..., 0] * X - 0.5
    s = 4 * xf / 255.0
    ok = cov & (xf > 0.01) & (xf < X - 1.01) & ((p > 0.01) & (p < 0.99)).all(-1)
    assert ok.sum() > 0.5 * W * H
    bg = np.array([0.2, 0.4, 0.6])
    want = np.concatenate([s[..., None] * np.stack([s, 1 - s, np.full_like(s, 0.5)], -1) + (1 - s)[..., None] * bg,
                           s[..., None]], -1)
    assert np.abs(got[ok] - want[ok]).max() < 1e-4
    assert np.array_equal(got[~cov], np.broadcast_to([0.2, 0.4, 0.6, 0.0], got[~cov].shape).astype(np.float32))


CAMERAS = [((0.7, 0.5, -0.8), (-0.6, -0.45, 0.9)),          # outside
           ((-0.9, 0.3, 0.2), (1.0, -0.25, 0.15)),           # oblique
           ((0.1, 0.05, 0.1), (0.3, 0.2, -1.0))]             # inside the cube


@pytest.mark.parametrize("unit,early", [(0.0, True), (0.0, False), (1 / 40, True), (1 / 40, False)])
def test_random_volumes_match_float64_reference(vr, unit, early):
    rng = np.random.default_rng(17 + int(unit * 1000) + early)
    checked = 0
    for ci, (pos, front) in enumerate(CAMERAS):
        vol = rng.integers(0, 256, (24, 20, 28), dtype=np.uint8)
        vol[8:16] //= 8                                     # a dim slab: long rays
        lut = vr.transfer_function_table(smooth_table(rng, 0.5))
        bg = tuple(rng.uniform(0, 1, 3))
        tf = vr.TransferFunction(lut, unit, bg)
        W, H = 72, 54
        step = (1 / 96, 1 / 80, 1 / 64)
        P = vr.default_params(W, H, (96, 80, 64))
        P.no_early_exit = 0 if early else 1
        got = vr.raycast_tf(_dev(vol), (28, 20, 24), _cam(vr, pos, front), P, tf).cpu().numpy().astype(np.float64)
        ref, slack = march_tf_checked(vol, (pos, front, (0, 1, 0), 50.0), W, H, step, lut, unit, bg,
                                      early_exit=early)
        sel = slack > 1
        assert sel.mean() > 0.8, (ci, float(sel.mean()))
        d = np.abs(got - ref)[sel]
        assert (d > 2e-3).mean() <= 0.0, (ci, float((d > 2e-3).mean()), float(d.max()))
        assert np.median(d) < 1e-5
        checked += int(sel.sum())
        # the frame shows something (a camera inside the cube starts at the exit face, as in vr_raycast: nothing)
        assert ci == 2 or (ref[..., 3] > 0.05).mean() > 0.3
    assert checked > 3 * 0.8 * 72 * 54


def _tables(vr):
    """Transparent on a low range, on a middle band, nowhere, everywhere."""
    rng = np.random.default_rng(4)
    lut = [vr.transfer_function_table(smooth_table(rng, 0.6)) for _ in range(4)]
    lut[0][:90, 3] = 0.0
    lut[1][100:160, 3] = 0.0
    lut[2][:, 3] = np.maximum(lut[2][:, 3], 0.05)
    lut[3][:, 3] = 0.0
    return lut


def _sparse_volume():
    rng = np.random.default_rng(8)
    X, Y, Z = 96, 80, 72
    vol = np.zeros((Z, Y, X), np.uint8)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    r = np.sqrt((xx - 40) ** 2 + (yy - 38) ** 2 + (zz - 30) ** 2)
    vol[r < 22] = (230 - 6 * r[r < 22]).astype(np.uint8)
    vol[50:60, 10:30, 60:90] = rng.integers(0, 256, (10, 20, 30))
    vol[5:9, :, :] = 3
    return vol


@pytest.mark.parametrize("cell", [4, 8, 16])
def test_skip_grid_frames_bit_identical_dense(vr, cell):
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    grid = vr.build_skip_grid(dvol, (X, Y, Z), cell)
    for ti, lut in enumerate(_tables(vr)):
        for unit, early in ((0.0, 0), (1 / 90, 1)):
            tf = vr.TransferFunction(lut, unit, (0.3, 0.1, 0.0))
            for pos, front in CAMERAS + [((0, 0, -0.75), (0, 0, 1))]:
                cam = _cam(vr, pos, front)
                P = vr.default_params(160, 100, (256, 256, 128))
                P.no_early_exit = early
                plain = vr.raycast_tf(dvol, (X, Y, Z), cam, P, tf)
                vr.use_skip_grid(P, grid, cell)
                skipped = vr.raycast_tf(dvol, (X, Y, Z), cam, P, tf)
                import torch
                assert torch.equal(plain, skipped), (cell, ti, unit, pos)


# ---- the level-of-detail pool ----------------------------------------------------------------------------------------
GRID, BD, DIMS = (2, 2, 2), (32, 32, 32), (64, 64, 64)


@pytest.fixture(scope="module")
def pool_set(vr):
    full = _sparse_volume()[:64, :64, 16:80].copy()
    ijk = np.array([(i, j, k) for k in range(2) for j in range(2) for i in range(2)], np.int64)
    bricks = np.stack([full[k * 32:(k + 1) * 32, j * 32:(j + 1) * 32, i * 32:(i + 1) * 32] for i, j, k in ijk])
    bs = vr.BrickSet(8, BD, 1, 2)
    bs.build(bricks.copy())
    return bs, ijk


def test_pool_equals_dense_and_skip_grid(vr, pool_set):
    import torch
    bs, ijk = pool_set
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    plans = [np.full(8, M, np.int32), np.array([M, D - 3, -1, D - 1, M - 1, -1, D - 6, M], np.int32)]
    luts = _tables(vr)
    shown = 0
    for cuts in plans:
        buf = torch.zeros(bs.num_bricks * bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=buf)
        vol = vr.assemble_bricks(buf, BD, ijk, GRID)
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        for ti, lut in enumerate(luts):
            tf = vr.TransferFunction(lut, 1 / 70 if ti % 2 else 0.0, (1.0, 1.0, 1.0))
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front, 40.0)
                P = vr.default_params(96, 72, BD)
                want = vr.raycast_tf(vol, DIMS, cam, P, tf)
                got = vr.raycast_pool_tf(pool, table, BD, GRID, cam, P, tf)
                assert torch.equal(got, want), (cuts, ti, pos)
                for cell in (4, 8, 16):
                    Pd, Pp = vr.default_params(96, 72, BD), vr.default_params(96, 72, BD)
                    vr.use_skip_grid(Pd, vr.build_skip_grid(vol, DIMS, cell), cell)
                    vr.use_skip_grid(Pp, vr.build_skip_grid_pool(pool, table, BD, GRID, cell), cell)
                    assert torch.equal(vr.raycast_tf(vol, DIMS, cam, Pd, tf), want), (cuts, ti, pos, cell)
                    assert torch.equal(vr.raycast_pool_tf(pool, table, BD, GRID, cam, Pp, tf), want), (cuts, ti, pos, cell)
                shown += int(bool((want[..., 3] > 0).any()))
    assert shown >= 8


def test_pool_rejects_bad_params(vr, pool_set):
    bs, ijk = pool_set
    pool, table = bs.decode_lod_pool(np.full(8, bs.info(0)["max_tree_depth"], np.int32), ijk, GRID)
    tf = vr.TransferFunction(np.zeros((256, 4), np.float32))
    P = vr.default_params(32, 32, BD)
    P.vol_origin[:] = (1, 0, 0)
    with pytest.raises(vr.VrError):
        vr.raycast_pool_tf(pool, table, BD, GRID, vr.default_camera(), P, tf)
    P = vr.default_params(32, 32, BD, 1)
    with pytest.raises(vr.VrError):
        vr.raycast_pool_tf(pool, table, BD, GRID, vr.default_camera(), P, tf)
    with pytest.raises(ValueError):
        vr.raycast_pool_tf(pool, table, BD, GRID, vr.default_camera(), vr.default_params(32, 32, BD), None)


# ---- clip box and sub-volume ---------------------------------------------------------------------------------------
def test_slab_with_halo_equals_full_volume_in_its_box(vr):
    import torch
    rng = np.random.default_rng(12)
    X, Y, Z = 40, 36, 48
    vol = rng.integers(0, 256, (Z, Y, X), dtype=np.uint8)
    tf = vr.TransferFunction(vr.transfer_function_table(smooth_table(rng, 0.4)), 1 / 50, (0.1, 0.2, 0.3))
    dfull = _dev(vol)
    for z0, z1 in ((0, 16), (16, 32), (32, 48), (10, 29)):
        lo, hi = max(z0 - 1, 0), min(z1 + 1, Z)
        slab = _dev(vol[lo:hi])
        for pos, front in CAMERAS:
            cam = _cam(vr, pos, front)
            for early in (0, 1):
                P = vr.default_params(64, 48, (X, Y, Z))
                P.no_early_exit = early
                P.box_min[:] = (0.0, 0.0, z0 / Z)
                P.box_max[:] = (1.0, 1.0, z1 / Z)
                want = vr.raycast_tf(dfull, (X, Y, Z), cam, P, tf)
                P.global_dims[:] = (X, Y, Z)
                P.vol_origin[:] = (0, 0, lo)
                got = vr.raycast_tf(slab, (X, Y, hi - lo), cam, P, tf)
                assert torch.equal(got, want), (z0, z1, pos, early)


def test_empty_box_and_transparent_table_give_the_background(vr):
    import torch
    rng = np.random.default_rng(2)
    vol = rng.integers(0, 256, (16, 16, 16), dtype=np.uint8)
    bg = (0.25, 0.5, 0.75)
    want = torch.tensor([0.25, 0.5, 0.75, 0.0], dtype=torch.float32, device="cuda").expand(48, 64, 4)
    full = vr.transfer_function_table([(0, 1, 0, 0, 1.0), (255, 0, 1, 0, 1.0)])
    for pos, front in CAMERAS:
        cam = _cam(vr, pos, front)
        P = vr.default_params(64, 48, (16, 16, 16))
        P.box_min[:] = (2.0, 2.0, 2.0)
        P.box_max[:] = (3.0, 3.0, 3.0)
        assert torch.equal(vr.raycast_tf(_dev(vol), (16, 16, 16), cam, P, vr.TransferFunction(full, 0.0, bg)), want)
        P = vr.default_params(64, 48, (16, 16, 16))
        for unit in (0.0, 0.1):
            assert torch.equal(vr.raycast_tf(_dev(vol), (16, 16, 16), cam, P,
                                             vr.TransferFunction(np.zeros((256, 4)), unit, bg)), want)


def test_rejects_other_modes_and_foreign_tables(vr):
    vol = _dev(np.zeros((8, 8, 8), np.uint8))
    tf = vr.TransferFunction(np.zeros((256, 4)))
    for mode in (1, 2):
        with pytest.raises(vr.VrError):
            vr.raycast_tf(vol, (8, 8, 8), vr.default_camera(), vr.default_params(16, 16, (8, 8, 8), mode), tf)
    with pytest.raises(ValueError):
        vr.raycast_tf(vol, (8, 8, 8), vr.default_camera(), vr.default_params(16, 16, (8, 8, 8)), np.zeros((256, 4)))


# ---- surfaces ------------------------------------------------------------------------------------------------------
def test_viewer_draw_with_and_without_tf(vr):
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    tf = vr.TransferFunction.from_points([(0, 0, 0, 0, 0), (60, 0.2, 0.4, 1.0, 0.0), (200, 1.0, 0.3, 0.1, 0.6)], 1 / 128)
    v = HeadlessViewer(120, 90)
    v.cameraPos = np.array([0.1, -0.05, -0.9], np.float32)
    P = vr.default_params(120, 90, (256, 256, 128), 0, float(v.currIsoVal) / 255.0)
    assert torch.equal(v.draw(dvol, (X, Y, Z), tf=tf), vr.raycast_tf(dvol, (X, Y, Z), v.camera(), P, tf))
    assert torch.equal(v.draw(dvol, (X, Y, Z)), vr.raycast(dvol, (X, Y, Z), v.camera(), P))


def test_viewer_draw_lod_pool_with_tf(vr, pool_set):
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    bs, ijk = pool_set
    tf = vr.TransferFunction(_tables(vr)[0], 1 / 64)
    v = HeadlessViewer(96, 72)
    v.cameraPos = np.array([0.05, 0.0, -1.2], np.float32)
    for skip in (0, 8):
        frame, cuts = v.draw_lod_pool(bs, ijk, GRID, pixel_tolerance=2.0, skip_cell=skip, tf=tf)
        P = vr.default_params(96, 72, BD, 0, float(v.currIsoVal) / 255.0)
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        assert torch.equal(frame, vr.raycast_pool_tf(pool, table, BD, GRID, v.camera(), P, tf)), skip
        plain, _ = v.draw_lod_pool(bs, ijk, GRID, pixel_tolerance=2.0, skip_cell=skip)
        assert torch.equal(plain, vr.raycast_pool(pool, table, BD, GRID, v.camera(), P)), skip


def test_cpp_example_frame_equals_python(vr, tmp_path):
    """examples/transfer_function.cpp (g++ against Viewer.hpp and TransferFunction.hpp) draws the frame Python draws."""
    from test_transfer_function_cpu import EXAMPLE_POINTS, _compile_example
    from volumerenderer_amd.viewer import HeadlessViewer
    exe = _compile_example(tmp_path)
    out = tmp_path / "frame.bin"
    r = subprocess.run([exe, "render", str(out)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    got = np.fromfile(str(out), np.float32).reshape(64, 96, 4)
    X, Y, Z = 48, 40, 32
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    vol = (((x * 5 + y * 3) ^ (z * 7)) & 255).astype(np.uint8)
    v = HeadlessViewer(96, 64)
    v.cameraPos = np.array([0.15, -0.1, -0.8], np.float32)
    v.fov = np.float32(40.0)
    tf = vr.TransferFunction.from_points(EXAMPLE_POINTS, 1.0 / 64.0, (0.2, 0.2, 0.25))
    want = v.draw(_dev(vol), (X, Y, Z), brick_dims=(X, Y, Z), tf=tf).cpu().numpy()
    assert np.array_equal(got, want)
    assert (want[..., 3] > 0.1).mean() > 0.2
