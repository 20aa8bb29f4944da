"""vr_raycast_tf2d & co. on the GPU: a table of equal rows draws the one-dimensional kernels' frames and partials bit for
bit, a closed form on a ramp, pixel by pixel against the float64 reference of tests/reftf2d.py, a saturated top row,
frames bit-identical with and without the skip grid (and the column summary itself), pool against dense, slabs with
two halo layers (and one, which is not enough), unaligned volumes and tiny extents, two slab partials folded, and the
Python / C++ viewer surfaces."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays  # noqa: E402
from reftf2d import march_tf2d_checked  # noqa: E402
from test_gpu_shading import _pool_set, smooth_volume  # noqa: E402
from test_gpu_transfer_function import BD, CAMERAS, DIMS, GRID, _cam, _dev, _sparse_volume, _tables, smooth_table  # noqa: E402
from test_sort_last_tf_cpu import TOL  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADED = 3


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def pool_set(vr):
    return _pool_set(vr)


def _params(vr, W, H, bd, mode=SHADED):
    return vr.default_params(W, H, bd, mode)


def _equal_rows(lut, rows):
    return np.ascontiguousarray(np.broadcast_to(lut, (rows, 256, 4)))


# 1 ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [2, 3, 111])
def test_equal_rows_draw_the_one_dimensional_kernels_bit_for_bit(vr, pool_set, rows):
    """eB - eA is exactly 0, so e = eA + h * 0 = eA: vr_raycast_tf (shading None), vr_raycast_tf_shaded (a shading) and
    vr_raycast_tf_partial, dense and pool, for two values of grad_scale."""
    import torch
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    shadings = [None, vr.Shading(0.25, 0.6, 0.3, 16.0, (0.2, 0.5, -1.0))]
    bg = (0.3, 0.1, 0.0)
    for ti, lut in enumerate(_tables(vr)):
        for unit, early in ((0.0, 0), (0.0, 1), (1 / 90, 0), (1 / 90, 1)):
            tf1 = vr.TransferFunction(lut, unit, bg)
            tf2s = [vr.TransferFunction2D(_equal_rows(lut, rows), gs, unit, bg) for gs in (127.5 * (rows - 1) / 110, 900.0)]
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front)
                for sh in shadings:
                    P1 = _params(vr, 120, 80, (256, 256, 128), SHADED if sh else 0)
                    P2 = _params(vr, 120, 80, (256, 256, 128))
                    P1.no_early_exit = P2.no_early_exit = early
                    frame = vr.raycast_tf_shaded(dvol, (X, Y, Z), cam, P1, tf1, sh) if sh else vr.raycast_tf(dvol, (X, Y, Z), cam, P1, tf1)
                    part = vr.raycast_tf_partial(dvol, (X, Y, Z), cam, P1, tf1, sh)
                    for tf2 in tf2s:
                        what = (rows, ti, unit, early, pos, sh is not None, tf2.grad_scale)
                        assert torch.equal(vr.raycast_tf2d(dvol, (X, Y, Z), cam, P2, tf2, sh), frame), what
                        assert torch.equal(vr.raycast_tf2d_partial(dvol, (X, Y, Z), cam, P2, tf2, sh), part), what
    # the 2 x 2 x 2 set of 32^3 bricks with mixed and culled cuts
    bs, ijk = pool_set
    M, D = bs.info(0)["max_tree_depth"], bs.info(0)["orig_tree_depth"]
    pool, table = bs.decode_lod_pool(np.array([M, D - 3, -1, D - 1, M - 1, -1, D - 6, M], np.int32), ijk, GRID)
    shown = 0
    for ti, lut in enumerate(_tables(vr)):
        unit = 1 / 70 if ti % 2 else 0.0
        tf1 = vr.TransferFunction(lut, unit)
        tf2 = vr.TransferFunction2D(_equal_rows(lut, rows), (None, 2000.0)[ti % 2], unit)
        for early in (0, 1):
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front, 40.0)
                for sh in shadings:
                    P1 = _params(vr, 96, 72, BD, SHADED if sh else 0)
                    P2 = _params(vr, 96, 72, BD)
                    P1.no_early_exit = P2.no_early_exit = early
                    if sh:
                        frame = vr.raycast_pool_tf_shaded(pool, table, BD, GRID, cam, P1, tf1, sh)
                    else:
                        frame = vr.raycast_pool_tf(pool, table, BD, GRID, cam, P1, tf1)
                    part = vr.raycast_pool_tf_partial(pool, table, BD, GRID, cam, P1, tf1, sh)
                    what = (rows, ti, early, pos, sh is not None)
                    assert torch.equal(vr.raycast_pool_tf2d(pool, table, BD, GRID, cam, P2, tf2, sh), frame), what
                    assert torch.equal(vr.raycast_pool_tf2d_partial(pool, table, BD, GRID, cam, P2, tf2, sh), part), what
                    shown += int(bool((frame[..., 3] > 0).any()))
    assert shown >= 16


# 2 ----------------------------------------------------------------------------------------------------------------------
def test_ramp_seen_along_its_gradient_reads_row_one_and_a_half(vr):
    """A ramp of 3 grey levels per voxel along z seen along z, one sample per ray: y = 1.5 at grad_scale 127.5, so with an
    alpha that depends on the row alone (a[j] = j / 110) the pixel's alpha is 1.5 / 110 and its colour the value lookup.
    The z step is 8.25 voxels, so that the one sample lies near voxel 7.75: next to the face the clamped neighbour of
    the first voxel layer halves its central difference."""
    X, Y, Z = 16, 16, 64
    vol = np.broadcast_to((3 * np.arange(Z)).astype(np.uint8)[:, None, None], (Z, Y, X)).copy()
    k = np.arange(256) / 255.0
    lut = np.empty((111, 256, 4))
    lut[:, :, :3] = np.stack([k, 1 - k, np.full(256, 0.25)], -1)[None]
    lut[:, :, 3] = (np.arange(111) / 110.0)[:, None]
    tf = vr.TransferFunction2D(lut, background=(0.0, 0.0, 0.0))
    assert tf.grad_scale == 127.5
    W, H = 32, 32
    cam = _cam(vr, (0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 6.0)
    P = _params(vr, W, H, (X, Y, Z))
    P.step_size[2] = 8.25 / Z
    P.max_samples = 1
    got = vr.raycast_tf2d(_dev(vol), (X, Y, Z), cam, P, tf).cpu().numpy().astype(np.float64)
    cov, vuv, g = rays((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), (0, 1, 0), 6.0, W, H)
    p = vuv + g * np.array([1 / X, 1 / Y, 8.25 / Z])
    zf = p[..., 2] * Z - 0.5
    assert cov.all() and zf.min() > 7.7 and zf.max() < 7.76
    s = 3 * zf / 255.0
    a = 1.5 / 110
    want = a * np.stack([s, 1 - s, np.full_like(s, 0.25)], -1)
    print("ramp: colour %.3g alpha %.3g" % (np.abs(got[..., :3] - want).max(), np.abs(got[..., 3] - a).max()))
    assert np.abs(got[..., :3] - want).max() < 1e-4
    assert np.abs(got[..., 3] - a).max() < 1e-6


# 3 ----------------------------------------------------------------------------------------------------------------------
SMOOTH_CASES = [(lit, unit, early) for lit in (False, True) for unit in (0.0, 1 / 40) for early in (True, False)]
SMOOTH_SCALE = 1000.0       # gradients of a few grey levels per voxel (m about 0.01) spread over the first dozens of rows


def table_5_to_111(vr, rng, alpha_max=0.5):
    """smooth_table control points in each of 5 rows, interpolated linearly (float64) to 111 rows."""
    ctrl = np.stack([vr.transfer_function_table(smooth_table(rng, alpha_max)) for _ in range(5)]).astype(np.float64)
    y = np.arange(111) * 4 / 110.0
    j = np.minimum(np.floor(y).astype(int), 3)
    h = (y - j)[:, None, None]
    return (ctrl[j] + h * (ctrl[j + 1] - ctrl[j])).astype(np.float32)


def smooth_case(vr, lit, unit, early, ci):
    """The volume, table, background and lighting of camera ci of a case; a generator per case, as the lit marcher's test."""
    rng = np.random.default_rng(100 + 37 * ci + 8 * lit + 4 * int(unit > 0) + 2 * early)
    vol = smooth_volume(rng, (24, 20, 28))
    lut = table_5_to_111(vr, rng)
    bg = tuple(rng.uniform(0, 1, 3))
    light = ((0, 0, 0), (0.4, 1.0, -0.6))[ci % 2]
    shp = (float(rng.uniform(0.1, 0.4)), float(rng.uniform(0.3, 0.8)), float(rng.uniform(0.0, 0.4)),
           float(rng.choice([1.0, 8.0, 32.0])), light, 1 / 255) if lit else None
    return vol, lut, bg, shp


def smooth_reference(vol, lut, bg, shp, unit, early, ci):
    pos, front = CAMERAS[ci]
    f32 = np.float32
    shp32 = tuple(float(f32(v)) for v in shp[:4]) + (shp[4], float(f32(shp[5]))) if shp else None
    return march_tf2d_checked(vol, (pos, front, (0, 1, 0), 50.0), 72, 54, (1 / 96, 1 / 80, 1 / 64), lut, SMOOTH_SCALE, shp32,
                              unit, bg, early_exit=early)


@pytest.mark.parametrize("lit,unit,early", SMOOTH_CASES)
def test_smooth_volumes_match_float64_reference(vr, lit, unit, early):
    """Within 2e-3 wherever the reference's slack exceeds 1, the bound of both one-dimensional marchers: the table's
    slope per row (control rows 27.5 rows apart) times the float32 error of y = m * 1000 (about 1e-4 rows) adds some
    1e-5.  Shares of compared pixels from a CPU run of the reference alone, cameras 0 / 1 / 2 (the third, inside the
    cube, starts at its exit face and sees nothing), per case in SMOOTH_CASES' order:
    0.951 0.944 1.000 | 0.998 0.996 1.000 | 0.880 0.840 1.000 | 0.998 0.996 1.000 |
    0.972 0.954 1.000 | 0.996 0.981 1.000 | 0.862 0.908 1.000 | 0.988 0.996 1.000."""
    checked = 0
    for ci, (pos, front) in enumerate(CAMERAS):
        vol, lut, bg, shp = smooth_case(vr, lit, unit, early, ci)
        tf = vr.TransferFunction2D(lut, SMOOTH_SCALE, unit, bg)
        P = _params(vr, 72, 54, (96, 80, 64))
        P.no_early_exit = 0 if early else 1
        got = vr.raycast_tf2d(_dev(vol), (28, 20, 24), _cam(vr, pos, front), P, tf, vr.Shading(*shp) if lit else None)
        got = got.cpu().numpy().astype(np.float64)
        ref, slack = smooth_reference(vol, lut, bg, shp, unit, early, ci)
        sel = slack > 1
        d = np.abs(got - ref)[sel]
        print("smooth lit %d unit %.3f early %d camera %d: share %.3f max %.3g" % (lit, unit, early, ci, sel.mean(), d.max()))
        assert sel.mean() > 0.75, (ci, float(sel.mean()))
        assert d.max() <= 2e-3, (ci, float(d.max()), float((d > 2e-3).mean()))
        checked += int(sel.sum())
        assert ci == 2 or (ref[..., 3] > 0.05).mean() > 0.3
    assert checked > 3 * 0.75 * 72 * 54


# 4 ----------------------------------------------------------------------------------------------------------------------
def test_a_grad_scale_that_saturates_reads_the_top_row(vr):
    """grad_scale = 1e30 on a random volume: every sample with a gradient clamps to y = rows - 1 (m * grad_scale may be
    +inf).  With the two top rows equal, e is the top row's entry exactly: vr_raycast_tf's frame through that row."""
    import torch
    rng = np.random.default_rng(23)
    vol = rng.integers(0, 256, (24, 20, 28), dtype=np.uint8)
    vol[8:16] //= 8
    top = vr.transfer_function_table(smooth_table(rng, 0.5))
    lut = rng.uniform(0, 1, (6, 256, 4)).astype(np.float32)
    lut[4] = lut[5] = top
    tf2 = vr.TransferFunction2D(lut, 1e30, 1 / 40, (0.2, 0.5, 0.7))
    tf1 = vr.TransferFunction(top, 1 / 40, (0.2, 0.5, 0.7))
    for pos, front in CAMERAS:
        cam = _cam(vr, pos, front)
        want = vr.raycast_tf(_dev(vol), (28, 20, 24), cam, _params(vr, 72, 54, (96, 80, 64), 0), tf1)
        assert torch.equal(vr.raycast_tf2d(_dev(vol), (28, 20, 24), cam, _params(vr, 72, 54, (96, 80, 64)), tf2), want), pos
    # and a general table against the reference (h = 1 in the top interval)
    lut[4] = vr.transfer_function_table(smooth_table(rng, 0.5))
    tf2 = vr.TransferFunction2D(lut, 1e30, 0.0, (0.2, 0.5, 0.7))
    pos, front = CAMERAS[0]
    got = vr.raycast_tf2d(_dev(vol), (28, 20, 24), _cam(vr, pos, front), _params(vr, 72, 54, (96, 80, 64)), tf2)
    ref, slack = march_tf2d_checked(vol, (pos, front, (0, 1, 0), 50.0), 72, 54, (1 / 96, 1 / 80, 1 / 64), lut, 1e30, None, 0.0,
                                    (0.2, 0.5, 0.7))
    sel = slack > 1
    assert sel.mean() > 0.8
    assert np.abs(got.cpu().numpy() - ref)[sel].max() <= 2e-3


def _columns_reference(lut):
    opaque = (np.asarray(lut)[:, :, 3] != 0).any(0)
    out, nxt = np.empty(256, np.int64), 256
    for k in range(255, -1, -1):
        nxt = k if opaque[k] else nxt
        out[k] = nxt
    return out


def _skip_tables(vr):
    """(transparent on a low range in every row, transparent in row 0 only), 7 rows each."""
    rng = np.random.default_rng(6)
    low = np.stack([vr.transfer_function_table(smooth_table(rng, 0.6)) for _ in range(7)])
    low[:, :, 3] = np.maximum(low[:, :, 3], 0.02)
    low[:, :90, 3] = 0.0
    low[3, :120, 3] = 0.0                                   # one row clear further up: the others decide
    row0 = np.stack([vr.transfer_function_table(smooth_table(rng, 0.6)) for _ in range(7)])
    row0[:, :, 3] = np.maximum(row0[:, :, 3], 0.02)
    row0[0, :, 3] = 0.0
    return low, row0


def test_column_summary(vr):
    low, row0 = _skip_tables(vr)
    band = low.copy()
    band[:, 200:, 3] = 0.0
    band[5, 230, 3] = 0.5                                    # one row alone keeps a column
    for lut in (low, row0, band, np.zeros((2, 256, 4), np.float32), np.ones((256, 256, 4), np.float32)):
        tf = vr.TransferFunction2D(lut)
        assert np.array_equal(tf.columns.cpu().numpy().astype(np.int64), _columns_reference(lut))
    assert np.array_equal(vr.TransferFunction2D(row0).columns.cpu().numpy(), np.arange(256))      # nothing may be skipped


@pytest.mark.parametrize("cell", [4, 8, 16])
def test_skip_grid_frames_bit_identical(vr, cell):
    import torch
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    grid = vr.build_skip_grid(dvol, (X, Y, Z), cell)
    for ti, lut in enumerate(_skip_tables(vr)):
        for unit, early in ((0.0, 0), (1 / 90, 1)):
            tf = vr.TransferFunction2D(lut, 127.5, unit, (0.3, 0.1, 0.0))
            for sh in (None, vr.Shading(light_dir=(0.3, -1.0, 0.2))):
                for pos, front in CAMERAS + [((0, 0, -0.75), (0, 0, 1))]:
                    cam = _cam(vr, pos, front)
                    P = _params(vr, 160, 100, (256, 256, 128))
                    P.no_early_exit = early
                    plain = vr.raycast_tf2d(dvol, (X, Y, Z), cam, P, tf, sh)
                    part = vr.raycast_tf2d_partial(dvol, (X, Y, Z), cam, P, tf, sh)
                    vr.use_skip_grid(P, grid, cell)
                    assert torch.equal(plain, vr.raycast_tf2d(dvol, (X, Y, Z), cam, P, tf, sh)), (cell, ti, unit, pos)
                    assert torch.equal(part, vr.raycast_tf2d_partial(dvol, (X, Y, Z), cam, P, tf, sh)), (cell, ti, unit, pos)
                    # row 0 alone is transparent: the sphere's shell (gradient 6 per voxel) still shows
                    assert ti == 0 or pos[2] > 0 or bool((plain[..., 3] > 0.1).any())


def test_pool_equals_dense_and_the_finished_partial_is_the_frame(vr, pool_set):
    import torch
    bs, ijk = pool_set
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    plans = [np.full(8, M, np.int32), np.array([M, D - 3, -1, D - 1, M - 1, -1, D - 6, M], np.int32)]
    low, row0 = _skip_tables(vr)
    shown = 0
    for cuts in plans:
        buf = torch.zeros(bs.num_bricks * bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=buf)
        vol = vr.assemble_bricks(buf, BD, ijk, GRID)
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        for ti, lut in enumerate((low, row0)):
            tf = vr.TransferFunction2D(lut, 300.0, 1 / 70 if ti else 0.0, (0.1, 0.2, 0.3))
            sh = (None, vr.Shading(0.2, 0.6, 0.3, 12.0, (1, 1, -1)))[ti]
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front, 40.0)
                P = _params(vr, 96, 72, BD)
                want = vr.raycast_tf2d(vol, DIMS, cam, P, tf, sh)
                assert torch.equal(vr.raycast_pool_tf2d(pool, table, BD, GRID, cam, P, tf, sh), want), (cuts, ti, pos)
                part = vr.raycast_tf2d_partial(vol, DIMS, cam, P, tf, sh)
                assert torch.equal(vr.composite_finish_tf(part, tf), want), (cuts, ti, pos)
                Pp = _params(vr, 96, 72, BD)
                vr.use_skip_grid(Pp, vr.build_skip_grid_pool(pool, table, BD, GRID, 8), 8)
                assert torch.equal(vr.raycast_pool_tf2d(pool, table, BD, GRID, cam, Pp, tf, sh), want), (cuts, ti, pos)
                assert torch.equal(vr.raycast_pool_tf2d_partial(pool, table, BD, GRID, cam, Pp, tf, sh), part), (cuts, ti, pos)
                shown += int(bool((want[..., 3] > 0).any()))
    assert shown >= 8


def _noisy_volume(rng, X, Y, Z):
    vol = smooth_volume(rng, (Z, Y, X))
    return (vol.astype(np.int64) + rng.integers(0, 20, vol.shape)).clip(0, 255).astype(np.uint8)


def test_slab_with_two_halo_layers_equals_full_volume_and_one_is_not_enough(vr):
    """Unlit too: the row needs the gradient, whose taps reach one voxel beyond the trilinear taps."""
    import torch
    rng = np.random.default_rng(12)
    X, Y, Z = 40, 36, 48
    vol = _noisy_volume(rng, X, Y, Z)
    tf = vr.TransferFunction2D(table_5_to_111(vr, rng, 0.4), 1000.0, 1 / 50, (0.1, 0.2, 0.3))
    dfull = _dev(vol)
    differs = 0
    for sh in (None, vr.Shading(0.25, 0.6, 0.3, 16.0, (0.2, 0.5, -1.0))):
        for z0, z1 in ((0, 16), (16, 32), (32, 48), (10, 29)):
            for pos, front in CAMERAS:
                cam = _cam(vr, pos, front)
                for early in (0, 1):
                    P = _params(vr, 64, 48, (X, Y, Z))
                    P.no_early_exit = early
                    P.box_min[:] = (0.0, 0.0, z0 / Z)
                    P.box_max[:] = (1.0, 1.0, z1 / Z)
                    want = vr.raycast_tf2d(dfull, (X, Y, Z), cam, P, tf, sh)
                    P.global_dims[:] = (X, Y, Z)
                    for halo in (2, 1):
                        lo, hi = max(z0 - halo, 0), min(z1 + halo, Z)
                        P.vol_origin[:] = (0, 0, lo)
                        got = vr.raycast_tf2d(_dev(vol[lo:hi]), (X, Y, hi - lo), cam, P, tf, sh)
                        if halo == 2:
                            assert torch.equal(got, want), (z0, z1, pos, early, sh is not None)
                        elif sh is None and (z0, z1) == (16, 32) and early == 0:
                            differs += int(not torch.equal(got, want))
    assert differs >= 2         # the interior slab, seen from outside: its border samples read other rows


@pytest.mark.parametrize("dims", [(1, 9, 7), (9, 1, 7), (9, 7, 1), (2, 2, 2), (3, 5, 2), (17, 13, 11), (1, 1, 1)])
def test_unaligned_volumes_and_tiny_extents(vr, dims):
    """Volumes at byte offsets 1..15 inside a larger allocation and extents of 1, 2 and odd sizes, against the reference,
    and the pool of the same volume."""
    import torch
    X, Y, Z = dims
    rng = np.random.default_rng(X * 100 + Y * 10 + Z)
    vol = smooth_volume(rng, (Z, Y, X), 3) if min(dims) > 2 else rng.integers(0, 256, (Z, Y, X), dtype=np.uint8)
    lut = table_5_to_111(vr, rng)
    scale = 1000.0 if min(dims) > 2 else 127.5
    tf = vr.TransferFunction2D(lut, scale, 0.0, (0.2, 0.3, 0.4))
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
        img = vr.raycast_tf2d(v, dims, _cam(vr, *cam), P, tf)
        if first is None:
            first = img
            got = img.cpu().numpy().astype(np.float64)
            ref, slack = march_tf2d_checked(vol, (cam[0], cam[1], (0, 1, 0), 50.0), W, H, step, lut, scale, None, 0.0,
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
    want = vr.raycast_tf2d(buf, bd, _cam(vr, *cam), P, tf)
    assert torch.equal(vr.raycast_pool_tf2d(pool, table, bd, (1, 1, 1), _cam(vr, *cam), P, tf), want)


def test_two_slab_partials_folded_equal_the_frame(vr):
    """slab_params(..., halo=2) drives a two-slab frame end to end through vr_composite_slabs_tf, no_early_exit, within
    the sort-last tests' bound; composite_sort_last_tf takes the two-dimensional table for its background."""
    import torch
    from volumerenderer_amd import distributed as D
    rng = np.random.default_rng(41)
    X, Y, Z = 40, 36, 48
    vol = _noisy_volume(rng, X, Y, Z)
    tf = vr.TransferFunction2D(table_5_to_111(vr, rng, 0.3), 1000.0, 1 / 40, (0.2, 0.4, 0.6))
    W, H = 64, 48
    for sh in (None, vr.Shading()):
        for pos, front in CAMERAS[:2]:
            cam = _cam(vr, pos, front)
            base = _params(vr, W, H, (X, Y, Z))
            base.no_early_exit = 1
            want = vr.raycast_tf2d(_dev(vol), (X, Y, Z), cam, base, tf, sh)
            parts = []
            for r in range(2):
                Pr, local, (a0, a1) = D.slab_params(base, (X, Y, Z), 2, r, 2, halo=2)
                parts.append(vr.raycast_tf2d_partial(_dev(vol[a0:a1]), local, cam, Pr, tf, sh).reshape(-1, 4))
            two = D._gpu_combine_tf(torch.stack(parts, 0), 0, 2, cam, base, tf).reshape(H, W, 4)
            d = float((two - want).abs().max())
            print("two slabs lit %d: max %.3g" % (sh is not None, d))
            assert d <= TOL
            assert bool((want[..., 3] > 0.05).any())
            full = vr.raycast_tf2d_partial(_dev(vol), (X, Y, Z), cam, base, tf, sh)
            assert torch.equal(D.composite_sort_last_tf(full, cam, base, tf, axis=2), want)
    with pytest.raises(ValueError):
        D.composite_sort_last_tf(full, cam, base, "not a table")


def test_python_surface_checks(vr):
    import torch
    vol = _dev(np.zeros((4, 4, 4), np.uint8))
    tf2 = vr.TransferFunction2D(np.zeros((2, 256, 4), np.float32))
    tf1 = vr.TransferFunction(np.zeros((256, 4), np.float32))
    cam = vr.default_camera()
    P = _params(vr, 8, 8, (4, 4, 4))
    assert vr.raycast_tf2d(vol, (4, 4, 4), cam, P, tf2).shape == (8, 8, 4)
    with pytest.raises(ValueError):
        vr.raycast_tf2d(vol, (4, 4, 4), cam, P, tf1)
    with pytest.raises(ValueError):
        vr.raycast_tf2d(vol, (4, 4, 4), cam, P, tf2, shading="no")
    with pytest.raises(ValueError):
        vr.raycast_tf2d(vol, (4, 4, 5), cam, P, tf2)
    with pytest.raises(ValueError):
        vr.raycast_tf2d(vol, (4, 4, 4), cam, P, tf2, out=torch.zeros((8, 8, 3), device="cuda"))
    with pytest.raises(vr.VrError):                             # RENDER_SHADED only, lit or not
        vr.raycast_tf2d(vol, (4, 4, 4), cam, _params(vr, 8, 8, (4, 4, 4), 0), tf2)
    # a host table is built without a launch and refused by every frame call before the C call
    host = vr.TransferFunction2D(np.zeros((2, 256, 4), np.float32), device="cpu")
    assert not host.lut.is_cuda and not host.columns.is_cuda
    for call in (vr.raycast_tf2d, vr.raycast_tf2d_partial):
        with pytest.raises(ValueError):
            call(vol, (4, 4, 4), cam, P, host)
    assert torch.equal(vr.composite_finish_tf(vr.raycast_tf2d_partial(vol, (4, 4, 4), cam, P, tf2), host),
                       vr.raycast_tf2d(vol, (4, 4, 4), cam, P, tf2))        # only the background is read
    sep = vr.TransferFunction2D.from_separable(np.full((256, 4), 0.5, np.float32), [0.0, 0.5, 1.0])
    assert sep.rows == 3 and sep.grad_scale == 127.5 * 2 / 110
    assert np.array_equal(sep.lut[:, 7, 3].cpu().numpy(), np.array([0.0, 0.25, 0.5], np.float32))


# the viewer ---------------------------------------------------------------------------------------------------------------
def test_viewer_draw_and_draw_lod_pool(vr, pool_set):
    import torch
    from volumerenderer_amd.viewer import HeadlessViewer
    vol = _sparse_volume()
    Z, Y, X = vol.shape
    dvol = _dev(vol)
    tf = vr.TransferFunction2D(_skip_tables(vr)[1], opacity_unit=1 / 128)
    v = HeadlessViewer(120, 90)
    v.cameraPos = np.array([0.1, -0.05, -0.9], np.float32)
    P = _params(vr, 120, 90, (256, 256, 128))
    P.iso_value = float(v.currIsoVal) / 255.0
    for sh in (None, vr.Shading()):
        assert torch.equal(v.draw(dvol, (X, Y, Z), tf=tf, shading=sh), vr.raycast_tf2d(dvol, (X, Y, Z), v.camera(), P, tf, sh))
    with pytest.raises(ValueError):
        v.draw(dvol, (X, Y, Z), tf=tf, projection=vr.Projection())
    with pytest.raises(ValueError):
        v.draw(dvol, (X, Y, Z), mode=1, tf=tf)                  # an explicit mode that does not fit is not ignored
    bs, ijk = pool_set
    v = HeadlessViewer(96, 72)
    v.cameraPos = np.array([0.05, 0.0, -1.2], np.float32)
    for skip, sh in ((0, None), (8, None), (8, vr.Shading())):
        frame, cuts = v.draw_lod_pool(bs, ijk, GRID, pixel_tolerance=2.0, skip_cell=skip, tf=tf, shading=sh)
        P = _params(vr, 96, 72, BD)
        P.iso_value = float(v.currIsoVal) / 255.0
        info = bs.info(0)
        assert np.array_equal(cuts, vr.select_lod(v.camera(), P, BD, ijk, GRID, info["orig_tree_depth"],
                                                  info["max_tree_depth"], 2.0))       # the SHADED mode's two-voxel reach
        pool, table = bs.decode_lod_pool(cuts, ijk, GRID)
        assert torch.equal(frame, vr.raycast_pool_tf2d(pool, table, BD, GRID, v.camera(), P, tf, sh)), skip


def test_cpp_example_frame_equals_python(vr, tmp_path):
    """examples/transfer_function2d.cpp (g++ against Viewer.hpp and TransferFunction.hpp) draws the frame Python draws:
    the float frame bit for bit, and its PPM byte for byte."""
    from test_transfer_function2d_cpu import EXAMPLE_POINTS, EXAMPLE_WEIGHTS, _compile_example
    from volumerenderer_amd.viewer import HeadlessViewer
    exe = _compile_example(tmp_path)
    ppm, f32 = str(tmp_path / "frame.ppm"), str(tmp_path / "frame.f32")
    subprocess.check_call([exe, "render", ppm, f32], timeout=120)
    got = np.fromfile(f32, np.float32).reshape(64, 96, 4)
    X, Y, Z = 48, 40, 36
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    d2 = (2 * xx + 1 - X) ** 2 + (2 * yy + 1 - Y) ** 2 + (2 * zz + 1 - Z) ** 2
    vol = np.where(d2 < 18 * 18, 200, np.where(d2 < 32 * 32, 90, 0)).astype(np.uint8)
    tf = vr.TransferFunction2D.from_separable(vr.transfer_function_table(EXAMPLE_POINTS), EXAMPLE_WEIGHTS, None, 1 / 64,
                                              (0.05, 0.05, 0.1))
    sh = vr.Shading(light_dir=(0.5, 1.0, -0.5))
    v = HeadlessViewer(96, 64)
    v.cameraPos = np.array([0.2, -0.15, -0.85], np.float32)
    v.fov = 40.0
    want = v.draw(_dev(vol), (X, Y, Z), brick_dims=(X, Y, Z), tf=tf, shading=sh)
    assert np.array_equal(got, want.cpu().numpy())
    mine = str(tmp_path / "python.ppm")
    HeadlessViewer.dump_ppm(mine, want)
    assert open(ppm, "rb").read() == open(mine, "rb").read()
    a = want[..., 3].cpu().numpy()
    assert (a > 0.05).mean() > 0.1
    # boundary emphasis: the ray through the centre crosses four boundaries and two clear interiors
    flat = vr.TransferFunction2D.from_separable(vr.transfer_function_table(EXAMPLE_POINTS), [1.0] * 111, None, 1 / 64,
                                                (0.05, 0.05, 0.1))
    assert v.draw(_dev(vol), (X, Y, Z), brick_dims=(X, Y, Z), tf=flat, shading=sh)[..., 3].mean() > want[..., 3].mean()
