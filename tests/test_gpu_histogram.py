"""Volume histograms on the GPU: vr_histogram_bricks against NumPy for every data family at every size and base offset
(each path of the kernels: teams, one workgroup per brick, parts; the data-aware shortcuts and the plain build), a total
beyond 2^32, vr_histogram_pool against vr_histogram_bricks of the dense level-of-detail decode, vr_histogram2d against
tests/refhist.py with its two invariants, and the C++ example's hashes.  Every comparison is exact."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def at_offset(host, off):
    """host's bytes on the device, `off` bytes past an aligned allocation."""
    import torch
    buf = torch.zeros(host.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + host.size]
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == off % 16
    return view


# ---- bricks --------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (3, 15), (5, 17), (7, 4096), (2, 4097), (3, 70001), (1, 5000003), (4099, 64)]
OFFSETS = (0, 1, 5, 15)


def runs_of(n, length, rng):
    """Runs of `length` equal bytes that start at offsets that are no multiple of 16."""
    out = rng.integers(0, 256, n, dtype=np.uint8)
    pos = int(rng.integers(1, 16))
    while pos + length <= n:
        out[pos:pos + length] = rng.integers(0, 256)
        pos += length + int(rng.integers(1, 40)) * 2 + 1          # (an odd gap: the next run starts at another offset mod 16)
        if pos % 16 == 0:
            pos += 3
    return out


def families(n, seed):
    rng = np.random.default_rng(seed)
    yield "uniform random", rng.integers(0, 256, n, dtype=np.uint8)
    for c in (0, 37, 255):
        yield "constant %d" % c, np.full(n, c, np.uint8)
    yield "two alternating values", np.where(np.arange(n) % 2 == 0, 11, 240).astype(np.uint8)
    for length in (16, 64, 1024):
        yield "runs of %d" % length, runs_of(n, length, rng)
    mix = rng.integers(0, 256, n, dtype=np.uint8)                 # the bench's mix: 4096-byte blocks, two thirds constant
    for blk in range(0, n, 4096):
        if rng.random() < 2.0 / 3.0:
            mix[blk:blk + 4096] = rng.integers(0, 256)
    yield "bench mix", mix


@pytest.mark.parametrize("B,V", SIZES)
def test_bricks_equal_numpy_for_every_family_at_every_offset(vr, B, V):
    import refhist
    for name, host in families(B * V, seed=B * 1000003 + V):
        want_b, want_t = refhist.hist_bricks(host, B)
        assert np.array_equal(want_b.sum(1, dtype=np.uint64), np.full(B, V, np.uint64))
        for off in OFFSETS:
            got_b, got_t = vr.histogram_bricks(at_offset(host, off), B)
            assert got_b.dtype == np.uint32 and got_t.dtype == np.uint64
            assert np.array_equal(got_b, want_b), (name, B, V, off)
            assert np.array_equal(got_t, want_t), (name, B, V, off)
            assert np.array_equal(got_b.astype(np.uint64).sum(0), got_t)         # the per-brick rows sum to the total


def test_constant_bricks_pass_every_narrow_counter(vr):
    """The whole count in one bin: 70 001 passes 2^16, 5 000 003 any per-lane narrow counter."""
    for B, V in ((3, 70001), (1, 5000003)):
        for c in (0, 37, 255):
            b, t = vr.histogram_bricks(at_offset(np.full(B * V, c, np.uint8), 5), B)
            assert [int(v) for v in b[:, c]] == [V] * B and int(t[c]) == B * V and int(b.sum(dtype=np.uint64)) == B * V


def test_either_output_alone(vr):
    import refhist
    from volumerenderer_amd import _lib
    L = _lib.lib()
    host = np.random.default_rng(5).integers(0, 256, 3 * 70001, dtype=np.uint8)
    want_b, want_t = refhist.hist_bricks(host, 3)
    dev = at_offset(host, 1)
    b, t = np.zeros((3, 256), np.uint32), np.zeros(256, np.uint64)
    assert L.vr_histogram_bricks(C.c_void_p(dev.data_ptr()), 3, 70001, C.c_void_p(b.ctypes.data), None, None) == 0
    assert L.vr_histogram_bricks(C.c_void_p(dev.data_ptr()), 3, 70001, None, C.c_void_p(t.ctypes.data), None) == 0
    assert np.array_equal(b, want_b) and np.array_equal(t, want_t)
    assert np.array_equal(vr.histogram(dev), want_t)               # one brick = the whole tensor
    # the small kernel too
    dev = at_offset(host[:3 * 64], 15)
    assert L.vr_histogram_bricks(C.c_void_p(dev.data_ptr()), 3, 64, None, C.c_void_p(t.ctypes.data), None) == 0
    assert np.array_equal(t, refhist.hist_bricks(host[:3 * 64], 3)[1])


def test_total_beyond_32_bits(vr):
    """17 bricks of 2^28 zero bytes with a handful of others: the only case that can catch a 32-bit total."""
    import torch
    B, V = 17, 1 << 28
    data = torch.zeros(B * V, dtype=torch.uint8, device="cuda")
    marks = {0: 1, V - 1: 2, V: 3, 5 * V + 12345: 255, B * V - 1: 255, 16 * V + 7: 37}
    for pos, val in marks.items():
        data[pos] = val
    b, t = vr.histogram_bricks(data, B)
    want_t = np.zeros(256, np.uint64)
    want_b = np.zeros((B, 256), np.uint32)
    want_b[:, 0] = V
    for pos, val in marks.items():
        want_b[pos // V, val] += 1
        want_b[pos // V, 0] -= 1
    want_t[:] = want_b.astype(np.uint64).sum(0)
    assert int(want_t[0]) == 17 * (1 << 28) - len(marks) > 1 << 32
    assert np.array_equal(t, want_t) and np.array_equal(b, want_b)


def test_plain_and_data_aware_kernels_agree(vr):
    """vr_debug_set("hist_plain", 1): the same kernels without their shortcuts, the same counts."""
    import refhist
    from volumerenderer_amd import _lib
    from test_reslice_cpu import scene_volume
    L = _lib.lib()
    cases = [(5, 17), (7, 4096), (3, 70001), (4099, 64)]
    vol = scene_volume()
    vol[:, :, 20:] = 9                                              # (a constant region for the 2-D shortcut)
    try:
        for plain in (1, 0):
            assert L.vr_debug_set(b"hist_plain", plain) == 0
            for B, V in cases:
                for name, host in families(B * V, seed=V):
                    got_b, got_t = vr.histogram_bricks(at_offset(host, 5), B)
                    want_b, want_t = refhist.hist_bricks(host, B)
                    assert np.array_equal(got_b, want_b) and np.array_equal(got_t, want_t), (plain, name, B, V)
            assert np.array_equal(vr.histogram2d(vol.reshape(-1), (28, 20, 24)), refhist.hist2d(vol)), plain
    finally:
        assert L.vr_debug_set(b"hist_plain", 0) == 0
    assert L.vr_debug_set(b"hist_nothing", 1) == -1


# ---- the pool ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pool_set(vr):
    """Eight 32^3 bricks on a 2 x 2 x 2 grid, in an order that is not the cells'."""
    from test_gpu_lod_pool import rm_like
    rng = np.random.default_rng(77)
    vols = [rm_like((32, 32, 32), s) for s in range(5)] + [rng.integers(0, 256, (32, 32, 32), dtype=np.uint8),
                                                             np.full((32, 32, 32), 9, np.uint8), rm_like((32, 32, 32), 9)[::-1].copy()]
    bs = vr.BrickSet(8, (32, 32, 32), 1, 2).build(np.stack(vols))
    ijk = np.array([(1, 1, 1), (0, 0, 0), (1, 0, 0), (0, 1, 1), (0, 1, 0), (1, 1, 0), (0, 0, 1), (1, 0, 1)], np.int64)
    return bs, ijk, (2, 2, 2)


def check_pool_histogram(vr, bs, ijk, grid, cuts):
    import refhist
    import torch
    from volumerenderer_amd.render import POOL_ENTRY
    cuts = np.array(cuts, np.int32)
    B, V = bs.num_bricks, bs.voxels_per_brick
    cells_n = grid[0] * grid[1] * grid[2]
    if np.all(cuts < 0):                                            # nothing to decode: a pool of one unread byte
        pool = torch.full((1,), 0xA5, dtype=torch.uint8, device="cuda")
        tab = np.zeros(cells_n, POOL_ENTRY)
        tab["offset"] = -1
        table = torch.from_numpy(np.frombuffer(tab.tobytes(), np.uint8).copy()).cuda()
    else:
        pool, table = bs.decode_lod_pool(cuts, ijk, grid)
    got_c, got_t = vr.histogram_pool(pool, table, bs.dims, grid)
    # the dense decode at the same cuts, culled bricks zeroed, brick by brick
    dense = torch.zeros(B * V, dtype=torch.uint8, device="cuda")
    bs.decode_lod(cuts, out=dense)
    want_b, want_t = vr.histogram_bricks(dense, B)
    cell_of = [int(i + grid[0] * (j + grid[1] * k)) for i, j, k in ijk]
    assert sorted(cell_of) == list(range(cells_n))
    assert np.array_equal(got_c[cell_of], want_b) and np.array_equal(got_t, want_t)
    assert int(got_t.sum()) == B * V
    # and the rule restated over the pool's own bytes
    tab = np.frombuffer(table.cpu().numpy().tobytes(), POOL_ENTRY)
    ref_c, ref_t = refhist.hist_pool(pool.cpu().numpy(), tab, bs.dims, grid)
    assert np.array_equal(got_c, ref_c) and np.array_equal(got_t, ref_t)
    return got_c, tab


def test_pool_histogram_equals_the_dense_decode(vr, pool_set):
    bs, ijk, grid = pool_set
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    assert D == 15
    # full depth, three coarse cuts whose shifts differ from axis to axis, two culled bricks
    cuts = [M, 4, -1, D, 8, -1, 11, M]
    cells, tab = check_pool_histogram(vr, bs, ijk, grid, cuts)
    shifts = {tuple(int(s) for s in tab[int(i + 2 * (j + 2 * k))]["shift"]) for (i, j, k), c in zip(ijk, cuts) if 0 <= c < D}
    assert len(shifts) == 3 and all(len(set(s)) > 1 for s in shifts), shifts
    for (i, j, k), c in zip(ijk, cuts):
        if c < 0:                                                   # an absent cell reads as 0
            row = cells[int(i + 2 * (j + 2 * k))]
            assert int(row[0]) == 32 ** 3 and not row[1:].any()
    check_pool_histogram(vr, bs, ijk, grid, [-1] * 8)               # every brick culled
    check_pool_histogram(vr, bs, ijk, grid, [M] * 8)                # every brick at full depth
    check_pool_histogram(vr, bs, ijk, grid, [0] * 8)                # one stored voxel per brick


# ---- two dimensions --------------------------------------------------------------------------------------------------------
def volumes_2d():
    from test_reslice_cpu import scene_volume
    rng = np.random.default_rng(9)
    yield "1x1x1", np.array([[[200]]], np.uint8)
    yield "2x3x1", rng.integers(0, 256, (1, 3, 2), dtype=np.uint8)
    yield "5x1x7", rng.integers(0, 256, (7, 1, 5), dtype=np.uint8)
    yield "64x64x3", rng.integers(0, 256, (3, 64, 64), dtype=np.uint8)
    yield "scene", scene_volume()
    yield "constant", np.full((9, 11, 70), 37, np.uint8)
    yield "constant, rows of whole words", np.full((3, 5, 512), 37, np.uint8)
    ramp = np.zeros((4, 6, 264), np.uint8)                           # flat runs and steps inside and across words
    ramp[:, :, 100:] = 80
    ramp[:, 3:, 131:] = 200
    ramp[2:, :, 7::9] += 5
    yield "steps", ramp
    z, y, x = np.meshgrid(np.arange(6), np.arange(10), np.arange(12), indexing="ij")
    yield "checkerboard", (((x + y + z) % 2) * 255).astype(np.uint8)


@pytest.fixture(scope="module")
def scene_table():
    """The whole-volume table of the scene, computed once."""
    import refhist
    from test_reslice_cpu import scene_volume
    return refhist.hist2d(scene_volume())


def test_hist2d_equals_the_restated_rule(vr):
    import refhist
    for name, vol in volumes_2d():
        dims = vol.shape[::-1]
        got = vr.histogram2d(vol.reshape(-1), dims)
        assert got.shape == (111, 256) and got.dtype == np.uint64
        assert np.array_equal(got, refhist.hist2d(vol)), name
        assert np.array_equal(got.sum(0), vr.histogram(vol.reshape(-1))), name      # column sums: the 1-D histogram
        assert int(got.sum()) == vol.size
        if name.startswith("constant"):
            assert int(got[0, 37]) == vol.size                      # everything in one cell
        if name == "checkerboard":
            assert got[110].any() and int(refhist.isqrt(3 * 255 * 255)) >> 2 == 110
        if name == "1x1x1":
            assert int(got[0, 200]) == 1


def test_hist2d_of_a_volume_at_a_byte_offset(vr, scene_table):
    from test_reslice_cpu import scene_volume
    for off in (1, 7):
        assert np.array_equal(vr.histogram2d(at_offset(scene_volume().reshape(-1), off), (28, 20, 24)), scene_table)


@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_hist2d_slabs_sum_to_the_whole_volume(vr, scene_table, world):
    import torch
    from test_reslice_cpu import SCENE_DIMS, scene_volume
    from volumerenderer_amd import _lib
    from volumerenderer_amd import distributed as D
    L = _lib.lib()
    vol = scene_volume()
    I3 = C.c_int64 * 3
    for axis in range(3):
        total = np.zeros((111, 256), np.uint64)
        for rank in range(world):
            org, lo, hi, local, (a0, a1) = D.slab_voxels(SCENE_DIMS, axis, rank, world, halo=1)
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(a0, a1)
            part = vr.histogram2d(np.ascontiguousarray(vol[tuple(sl)]).reshape(-1), local, SCENE_DIMS, org, lo, hi)
            own = [slice(lo[2], hi[2]), slice(lo[1], hi[1]), slice(lo[0], hi[0])]
            assert np.array_equal(part.sum(0), np.bincount(vol[tuple(own)].reshape(-1), minlength=256).astype(np.uint64))
            total += part
            # the same slab without its halo is refused, by the wrapper and by the library
            org0, lo0, hi0, local0, (b0, b1) = D.slab_voxels(SCENE_DIMS, axis, rank, world, halo=0)
            sl[2 - axis] = slice(b0, b1)
            bare = torch.from_numpy(np.ascontiguousarray(vol[tuple(sl)]).reshape(-1)).cuda()
            with pytest.raises(ValueError):
                vr.histogram2d(bare, local0, SCENE_DIMS, org0, lo0, hi0)
            hist = np.zeros((111, 256), np.uint64)
            assert L.vr_histogram2d(C.c_void_p(bare.data_ptr()), I3(*local0), I3(*SCENE_DIMS), I3(*org0), I3(*lo0), I3(*hi0),
                                    C.c_void_p(hist.ctypes.data), None) == -1
            assert not hist.any()
        assert np.array_equal(total, scene_table), (world, axis)


def test_hist2d_of_own_boxes_aligned_to_nothing(vr, scene_table):
    import refhist
    from test_reslice_cpu import SCENE_DIMS, scene_volume
    vol = scene_volume()
    flat = vol.reshape(-1)
    for lo, hi in (((3, 0, 5), (17, 20, 6)), ((0, 19, 0), (28, 20, 24)), ((27, 0, 23), (28, 1, 24)), ((1, 2, 3), (26, 17, 22))):
        got = vr.histogram2d(flat, SCENE_DIMS, own_lo=lo, own_hi=hi)
        assert np.array_equal(got, refhist.hist2d(vol, own_lo=lo, own_hi=hi)), (lo, hi)
        assert int(got.sum()) == (hi[0] - lo[0]) * (hi[1] - lo[1]) * (hi[2] - lo[2])
    # eight boxes around an interior point tile the volume
    cx, cy, cz = 13, 7, 5
    total = np.zeros((111, 256), np.uint64)
    for bx in ((0, cx), (cx, 28)):
        for by in ((0, cy), (cy, 20)):
            for bz in ((0, cz), (cz, 24)):
                total += vr.histogram2d(flat, SCENE_DIMS, own_lo=(bx[0], by[0], bz[0]), own_hi=(bx[1], by[1], bz[1]))
    assert np.array_equal(total, scene_table)
    # a local volume inside a larger global one: a block of the scene with one halo layer on every side
    org, dims = (2, 3, 4), (20, 12, 9)
    block = np.ascontiguousarray(vol[4:13, 3:15, 2:22])
    lo, hi = (3, 4, 5), (21, 14, 12)
    got = vr.histogram2d(block.reshape(-1), dims, SCENE_DIMS, org, lo, hi)
    assert np.array_equal(got, refhist.hist2d(vol, own_lo=lo, own_hi=hi))
    assert np.array_equal(got, refhist.hist2d(block, SCENE_DIMS, org, lo, hi))


def test_hist2d_rows_longer_than_a_segment(vr):
    """x-rows of more than 4096 voxels (several items per row) and more rows than one round of a workgroup takes."""
    import refhist
    rng = np.random.default_rng(3)
    vol = rng.integers(0, 256, (3, 7, 9001), dtype=np.uint8)
    vol[:, :, 3000:7000] //= 16
    assert np.array_equal(vr.histogram2d(vol.reshape(-1), (9001, 7, 3)), refhist.hist2d(vol))
    vol = rng.integers(0, 64, (40, 300, 5), dtype=np.uint8)           # 12 000 rows: more than 256 workgroups x 16
    assert np.array_equal(vr.histogram2d(vol.reshape(-1), (5, 300, 40)), refhist.hist2d(vol))


def test_window_from_a_device_histogram_is_accepted_by_the_projection(vr):
    import torch
    from test_reslice_cpu import SCENE_DIMS, scene_volume
    import refhist
    vol = scene_volume()
    h = vr.histogram(vol.reshape(-1))
    lo, hi = vr.window_from_histogram(h, 1, 0.02, 0.98)
    assert (np.float32(lo), np.float32(hi)) == refhist.window(h, 1, 0.02, 0.98) and 0.0 <= lo < hi <= 1.0
    proj = vr.projection_from_histogram(vr.histogram2d(vol.reshape(-1), SCENE_DIMS), "max", 1, 0.02, 0.98)
    assert proj.window == (lo, hi)
    cam, P = vr.default_camera(), vr.default_params(48, 36, SCENE_DIMS, 4)
    frame = vr.raycast_projection(vol.reshape(-1), SCENE_DIMS, cam, P, proj)
    assert bool(torch.isfinite(frame).all()) and 0.0 < float(frame[..., 0].max()) <= 1.0


# ---- the example -----------------------------------------------------------------------------------------------------------
def fnv1a64(data):
    h = 14695981039346656037
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_cpp_example_prints_the_hashes_of_the_python_tables(vr, tmp_path):
    import torch
    from test_histogram_cpu import compile_example
    from volumerenderer_amd.render import POOL_ENTRY
    exe = compile_example(tmp_path)
    vol = np.random.default_rng(41).integers(0, 256, (20, 24, 32), dtype=np.uint8)
    vol[5:12] //= 8
    vol[:, :3] = 0
    raw = tmp_path / "volume.raw"
    raw.write_bytes(vol.tobytes())
    r = subprocess.run([exe, str(raw)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    dev = torch.from_numpy(vol.reshape(-1)).cuda()
    bricks, total = vr.histogram_bricks(dev, 4)
    tab = np.zeros(3, POOL_ENTRY)
    tab["offset"], tab["shift"][2] = (0, -1, 512), (1, 1, 1)
    cells, ptotal = vr.histogram_pool(dev, torch.from_numpy(np.frombuffer(tab.tobytes(), np.uint8).copy()).cuda(), (8, 8, 8), (3, 1, 1))
    h2 = vr.histogram2d(dev, (32, 24, 20))
    want = [("bricks", bricks), ("total", total), ("pool_cells", cells), ("pool_total", ptotal), ("hist2d", h2)]
    for ln, (name, table) in zip(lines, want):
        assert ln == [name, "fnv1a64", fnv1a64(np.ascontiguousarray(table).tobytes())], name
    lo, hi = vr.window_from_histogram(total, 0, 0.05, 0.95)
    assert lines[5][0] == "window" and (np.float32(float(lines[5][1])), np.float32(float(lines[5][2]))) == (np.float32(lo), np.float32(hi))
    # the built-in volume runs too
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and len(r.stdout.strip().splitlines()) == 6, r.stdout + r.stderr
