"""Every pool reader against the table contract of vrhip.h (at vr_pool_entry), on pools no producer of the project wrote:
the hand-built pools of tests/poolcases.py (any shift triple, slots at any byte, in any order, back to back; noise
everywhere else), uploaded next to refpool.expand of them as a dense volume.  Every comparison is torch.equal or
np.array_equal: the dense calls are pinned to the float64 marchers elsewhere, so bit identity with them is the contract.

  * vr_raycast_pool (composite, iso-surface, PARTIAL with a box), _tf, _tf_shaded, _tf_partial (lit and unlit), _tf2d and
    its partial (lit and unlit), _projection and its partial (MAX, MIN, MEAN) == the dense call, at four cameras of
    test_gpu_lod_pool.CAMERAS (outside, inside, grazing a brick face, down an axis), 48 x 40, without and with the pool's
    own skip grid; one 1 x 1 and one 65 x 63 frame per geometry;
  * vr_skip_grid_build_pool == vr_skip_grid_build == _grid_def (test_gpu_raymarch_edges.py) at cells 1, 3, 8, 31, 64;
  * vr_histogram_pool == refhist.hist_pool == the histogram of expand;
  * one slot beyond 2^32 bytes with a different slot at the same offset modulo 2^32;
  * a table at +8 bytes is refused by every reader with VR_ERR_INVALID and nothing is written."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marchcases as MC  # noqa: E402
import poolcases as PC  # noqa: E402
import refhist  # noqa: E402
import refpool as R  # noqa: E402
from test_gpu_lod_pool import CAMERAS, _cam  # noqa: E402
from test_gpu_raymarch_edges import _grid_def  # noqa: E402

pytestmark = pytest.mark.gpu
GEOS = range(len(PC.GEOMETRIES))
CAMS = [CAMERAS[0], CAMERAS[2], CAMERAS[4], CAMERAS[5]]      # outside, inside, grazing a brick face, down an axis
SKIP_CELLS = (1, 3, 8, 31, 64)
W, H = 48, 40
ISO = 100.0 / 255.0
BOX = ((0.25, 0.0, 0.125), (0.75, 0.8, 1.0))
# (kind, vr_render_params.mode)
KINDS = [("grey0", 0), ("grey1", 1), ("grey2", 2), ("tf", 0), ("shaded", 3), ("tf_partial", 0), ("tf_partial_lit", 3),
         ("tf2d", 3), ("tf2d_lit", 3), ("tf2d_partial", 3), ("tf2d_partial_lit", 3), ("max", 4), ("min", 4), ("mean", 4),
         ("max_partial", 4), ("min_partial", 4), ("mean_partial", 4)]


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def tables(vr):
    """Transfer functions with a transparent low range (the skip grid has something to skip), a directional light, the
    three projections."""
    lut, lut2 = MC.skip_tables()
    return dict(tf=vr.TransferFunction(lut, 1.0, MC.BACKGROUND), tf2=vr.TransferFunction2D(lut2, MC.GRAD_SCALE, 1.0, MC.BACKGROUND),
                sh=vr.Shading(*MC.SHADINGS[1]), proj={m: vr.Projection(m, (0.0, 1.0), MC.PROJ_BACKGROUND) for m in MC.OPS})


def _upload_pool(pool, view):
    """The pool as a tensor that starts `view` bytes into its allocation."""
    import torch
    buf = torch.empty(view + pool.size, dtype=torch.uint8, device="cuda")
    t = buf[view:]
    t.copy_(torch.from_numpy(pool))
    assert t.data_ptr() % 16 == view % 16
    return t


def _upload_table(table):
    import torch
    t = torch.from_numpy(np.frombuffer(table.tobytes(), np.uint8).copy()).cuda()
    assert t.data_ptr() % 16 == 0
    return t


def _sources(k):
    """(pool source, dense source) of case k: the leading arguments of the pool calls and of the dense calls."""
    import torch
    c = PC.cases()[k]
    pool, table = PC.build(k)
    vol = PC.volume(k)
    dims = vol.shape[::-1]
    return ((_upload_pool(pool, c["view"]), _upload_table(table), c["bd"], c["grid"]),
            (torch.from_numpy(np.array(vol)).cuda().reshape(-1), dims))


def _params(vr, kind, mode, dims, w=W, h=H):
    P = vr.default_params(w, h, tuple(max(2 * q, 16) for q in dims), mode, ISO)
    if kind == "grey2" or kind.endswith("partial") or kind.endswith("partial_lit"):
        P.box_min[:], P.box_max[:] = BOX
    return P


def _draw(vr, kind, pool, src, cam, P, T):
    """Frame `kind` of a source: the pool call or the dense call."""
    lit = T["sh"] if kind.endswith("lit") or kind == "shaded" else None
    if kind.startswith("grey"):
        return (vr.raycast_pool if pool else vr.raycast)(*src, cam, P)
    if kind == "tf":
        return (vr.raycast_pool_tf if pool else vr.raycast_tf)(*src, cam, P, T["tf"])
    if kind == "shaded":
        return (vr.raycast_pool_tf_shaded if pool else vr.raycast_tf_shaded)(*src, cam, P, T["tf"], lit)
    if kind.startswith("tf_partial"):
        return (vr.raycast_pool_tf_partial if pool else vr.raycast_tf_partial)(*src, cam, P, T["tf"], lit)
    if kind.startswith("tf2d_partial"):
        return (vr.raycast_pool_tf2d_partial if pool else vr.raycast_tf2d_partial)(*src, cam, P, T["tf2"], lit)
    if kind.startswith("tf2d"):
        return (vr.raycast_pool_tf2d if pool else vr.raycast_tf2d)(*src, cam, P, T["tf2"], lit)
    op = kind.split("_")[0]
    if kind.endswith("partial"):
        return (vr.raycast_pool_projection_partial if pool else vr.raycast_projection_partial)(*src, cam, P, T["proj"][op])
    return (vr.raycast_pool_projection if pool else vr.raycast_projection)(*src, cam, P, T["proj"][op])


def _check_frames(vr, T, psrc, dsrc, cams, name, w=W, h=H):
    """Every kind at every camera, without and with the skip grid (the pool's own on the pool call, the dense one on the
    dense call).  Returns the number of frames that show something."""
    import torch
    dims = dsrc[1]
    cell = 3 if max(dims) <= 16 else 8
    g_p, g_d = vr.build_skip_grid_pool(*psrc, cell), vr.build_skip_grid(*dsrc, cell)
    assert torch.equal(g_p, g_d), (name, "skip grid", cell)
    shown = 0
    for pos, front, fov in cams:
        cam = _cam(vr, pos, front, fov)
        for kind, mode in KINDS:
            for skip in (False, True):
                Pp, Pd = _params(vr, kind, mode, dims, w, h), _params(vr, kind, mode, dims, w, h)
                if skip:
                    vr.use_skip_grid(Pp, g_p, cell)
                    vr.use_skip_grid(Pd, g_d, cell)
                want = _draw(vr, kind, False, dsrc, cam, Pd, T)
                got = _draw(vr, kind, True, psrc, cam, Pp, T)
                if not torch.equal(got, want):
                    bad = (got != want).any(-1)
                    raise AssertionError("%s: %s at %s, skip grid %s: %d of %d pixels differ, first at %s"
                                         % (name, kind, pos, skip, int(bad.sum()), bad.numel(), tuple(bad.nonzero()[0].tolist())))
                shown += int(bool((want != want[0, 0]).any()))
    return shown


@pytest.mark.parametrize("geo", GEOS)
def test_frames_equal_dense_frames(vr, tables, geo):
    shown = 0
    for k in PC.of_geometry(geo):
        psrc, dsrc = _sources(k)
        n = _check_frames(vr, tables, psrc, dsrc, CAMS, PC.cases()[k]["name"])
        # a pool with a present cell is seen: some frame is not one colour throughout
        assert n > 0 or len(PC.cases()[k]["absent"]) == PC.ncells(PC.cases()[k]["grid"]), PC.cases()[k]["name"]
        shown += n
    print("POOL geometry %d: %d cases, %d frames show something" % (geo, len(PC.of_geometry(geo)), shown))


@pytest.mark.parametrize("geo", GEOS)
def test_frame_sizes(vr, tables, geo):
    """One pixel (its ray is the centre ray) and 65 x 63 (no whole wave tiles), on the geometry's per-cell random shifts."""
    k = PC.of_geometry(geo)[-1]
    psrc, dsrc = _sources(k)
    for w, h in ((1, 1), (65, 63)):
        _check_frames(vr, tables, psrc, dsrc, CAMS[:1], PC.cases()[k]["name"], w, h)


@pytest.mark.parametrize("geo", GEOS)
def test_skip_grids(vr, geo):
    """Cells larger than a brick and cells that divide nothing.  _grid_def walks its cells in Python: on the 64^3 volumes
    of the 32^3 family it is held to at one voxel per cell for one case (the per-cell random shifts), at the larger cells
    for all."""
    import torch
    ks = PC.of_geometry(geo)
    for k in ks:
        c = PC.cases()[k]
        psrc, dsrc = _sources(k)
        for S in SKIP_CELLS:
            g_p, g_d = vr.build_skip_grid_pool(*psrc, S), vr.build_skip_grid(*dsrc, S)
            assert torch.equal(g_p, g_d), (c["name"], S)
            if S > 1 or PC.volume(k).size <= 4096 or c["name"].endswith("random"):
                assert np.array_equal(g_p.cpu().numpy(), _grid_def(PC.volume(k), S)), (c["name"], S)


@pytest.mark.parametrize("geo", GEOS)
def test_histograms(vr, geo):
    for k in PC.of_geometry(geo):
        c = PC.cases()[k]
        pool, table = PC.build(k)
        psrc, _ = _sources(k)
        cells, total = vr.histogram_pool(*psrc)
        want_c, want_t = refhist.hist_pool(pool, table, c["bd"], c["grid"])
        assert np.array_equal(cells, want_c) and np.array_equal(total, want_t), c["name"]
        assert np.array_equal(total, np.bincount(PC.volume(k).reshape(-1), minlength=256)), c["name"]


def test_offset_beyond_32_bits(vr, tables):
    """Cell 0's slot at 2^32 + 4099 and cell 1's, other data, at 4099: an offset cut to 32 bits reads the wrong brick and
    stays inside the allocation.  The pool is not filled; the slots and their noise tails are slice copies."""
    import torch
    segments, table, seg = PC.high_offset()
    try:
        pool = torch.empty(PC.HIGH_BYTES, dtype=torch.uint8, device="cuda")
    except RuntimeError as e:                          # (torch.OutOfMemoryError is one)
        print("no %d-byte allocation: %s" % (PC.HIGH_BYTES, e))
        pytest.skip("the device cannot allocate 2^32 + 2^20 bytes: %s" % str(e).splitlines()[0])
    for s, a in segments:
        pool[s:s + a.size].copy_(torch.from_numpy(a))
    vol = R.expand(seg, table, PC.HIGH_BD, PC.HIGH_GRID)
    psrc = (pool, _upload_table(table), PC.HIGH_BD, PC.HIGH_GRID)
    dsrc = (torch.from_numpy(vol).cuda().reshape(-1), vol.shape[::-1])
    assert _check_frames(vr, tables, psrc, dsrc, CAMS, "high offset") > 0
    for S in (1, 3):
        g = vr.build_skip_grid_pool(*psrc, S)
        assert torch.equal(g, vr.build_skip_grid(*dsrc, S)) and np.array_equal(g.cpu().numpy(), _grid_def(vol, S))
    cells, total = vr.histogram_pool(*psrc)
    X = PC.HIGH_BD[0]
    for c in range(2):
        assert np.array_equal(cells[c], np.bincount(vol[:, :, c * X:(c + 1) * X].reshape(-1), minlength=256)), c
    assert np.array_equal(total, np.bincount(vol.reshape(-1), minlength=256))


def test_table_at_8_bytes_is_refused(vr, tables):
    """vr_pool_entry's own alignment is 8, the kernels load an entry as one 16-byte word: every reader refuses a table
    that is not 16-byte aligned with VR_ERR_INVALID before anything is launched (`out` keeps its poison)."""
    import torch
    from volumerenderer_amd import _lib
    k = PC.of_geometry(3)[0]
    c = PC.cases()[k]
    (pool, table, bd, grid), (_, dims) = _sources(k)
    buf = torch.zeros(table.numel() + 16, dtype=torch.uint8, device="cuda")
    off = buf[8:8 + table.numel()]
    off.copy_(table)
    assert off.data_ptr() % 16 == 8 and off.is_contiguous()
    psrc = (pool, off, bd, grid)
    cam = _cam(vr, *CAMS[0])
    for kind, mode in KINDS:
        P = _params(vr, kind, mode, dims)
        out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        lit = tables["sh"] if kind.endswith("lit") or kind == "shaded" else None
        op = kind.split("_")[0]
        call = {"grey": lambda: vr.raycast_pool(*psrc, cam, P, out=out),
                "tf": lambda: vr.raycast_pool_tf(*psrc, cam, P, tables["tf"], out=out),
                "shaded": lambda: vr.raycast_pool_tf_shaded(*psrc, cam, P, tables["tf"], lit, out=out),
                "tf_partial": lambda: vr.raycast_pool_tf_partial(*psrc, cam, P, tables["tf"], lit, out=out),
                "tf2d": lambda: vr.raycast_pool_tf2d(*psrc, cam, P, tables["tf2"], lit, out=out),
                "tf2d_partial": lambda: vr.raycast_pool_tf2d_partial(*psrc, cam, P, tables["tf2"], lit, out=out),
                "proj": lambda: vr.raycast_pool_projection(*psrc, cam, P, tables["proj"][op], out=out),
                "proj_partial": lambda: vr.raycast_pool_projection_partial(*psrc, cam, P, tables["proj"][op], out=out)}
        key = ("grey" if kind.startswith("grey") else "proj_partial" if mode == 4 and kind.endswith("partial") else
               "proj" if mode == 4 else kind[:-4] if kind.endswith("_lit") else kind)
        with pytest.raises(vr.VrError) as e:
            call[key]()
        assert e.value.status == -1, kind
        torch.cuda.synchronize()
        assert bool(torch.isnan(out).all()), kind
    grid_out = torch.full((2 * int(np.prod([(q + 2) // 3 for q in dims])),), 0xA5, dtype=torch.uint8, device="cuda")
    with pytest.raises(vr.VrError) as e:
        vr.build_skip_grid_pool(*psrc, 3, out=grid_out)
    assert e.value.status == -1
    torch.cuda.synchronize()
    assert bool((grid_out == 0xA5).all())
    cells, total = np.full((PC.ncells(grid), 256), 0xA5A5A5A5, np.uint32), np.full(256, 0xA5A5A5A5A5A5A5A5, np.uint64)
    i3 = lambda v: (C.c_int64 * 3)(*v)             # noqa: E731
    rc = _lib.lib().vr_histogram_pool(C.c_void_p(pool.data_ptr()), C.c_void_p(off.data_ptr()), i3(bd), i3(grid),
                                      C.c_void_p(cells.ctypes.data), C.c_void_p(total.ctypes.data), None)
    assert rc == -1 and (cells == 0xA5A5A5A5).all() and (total == 0xA5A5A5A5A5A5A5A5).all()
    # the same table, aligned, is taken
    assert vr.raycast_pool(pool, table, bd, grid, cam, _params(vr, "grey0", 0, dims)).shape == (H, W, 4), c["name"]
