"""Volume histograms without a GPU: the argument checks of the three device calls (each before the device), the window
rule vr_window_from_histogram against a restatement of it, refhist's integer square root, the slab boxes of
distributed.slab_voxels against vr_histogram2d's box check, histogram_all_reduce over gloo, the Python wrappers'
ValueErrors, and the C++ example's build."""
import ctypes as C
import math
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

INVALID, NO_DEVICE = -1, -2
I64x3 = C.c_int64 * 3


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def device_count(L):
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    return n.value


# ---- argument checks come before the device ----------------------------------------------------------------------------
def test_histogram_bricks_rejects_bad_arguments_before_the_device(L):
    buf = (C.c_uint8 * 64)()
    bricks, total = (C.c_uint32 * (4 * 256))(), (C.c_uint64 * 256)()

    def call(data=buf, nb=4, v=16, b=bricks, t=total):
        return L.vr_histogram_bricks(data, nb, v, b, t, None)

    for kw in (dict(data=None), dict(b=None, t=None), dict(nb=0), dict(nb=-3), dict(v=0), dict(v=-1), dict(v=1 << 32),
               dict(v=1 << 40)):
        assert call(**kw) == INVALID, kw
    if device_count(L) == 0:
        assert call() == NO_DEVICE                       # valid arguments reach the device check: no CPU fallback
        assert call(b=None) == NO_DEVICE and call(t=None) == NO_DEVICE      # either output alone will do
        assert call(v=(1 << 32) - 1) == NO_DEVICE        # the largest brick is inside the range
    assert not any(bricks) and not any(total)


def test_histogram_pool_rejects_bad_arguments_before_the_device(L):
    buf, table = (C.c_uint8 * 64)(), (C.c_uint8 * 16)()
    cells, total = (C.c_uint32 * 256)(), (C.c_uint64 * 256)()

    def call(pool=buf, tab=table, bd=(4, 4, 4), grid=(1, 1, 1), c=cells, t=total):
        return L.vr_histogram_pool(pool, tab, None if bd is None else I64x3(*bd), None if grid is None else I64x3(*grid), c, t, None)

    bad = [dict(pool=None), dict(tab=None), dict(bd=None), dict(grid=None), dict(c=None, t=None)]
    bad += [dict(bd=b) for b in ((4, 6, 4), (0, 4, 4), (4, -4, 4), (4, 4, 3), (-(1 << 40), 4, 4))]      # not positive powers of two
    bad += [dict(grid=g) for g in ((0, 1, 1), (1, -1, 1), (1, 1, 0))]
    bad += [dict(grid=(1 << 29, 1, 1)), dict(grid=(1, 1 << 40, 1)), dict(bd=(1 << 31, 4, 4))]           # extents of 2^31 and more
    bad += [dict(bd=(2048, 2048, 1024)), dict(bd=(1 << 16, 1 << 16, 1))]                                # X*Y*Z > 2^32 - 1
    bad += [dict(bd=(1, 1, 1), grid=(1 << 11, 1 << 10, 1 << 10))]                                       # 2^31 cells
    for kw in bad:
        assert call(**kw) == INVALID, kw
    if device_count(L) == 0:
        assert call() == NO_DEVICE
        assert call(c=None) == NO_DEVICE and call(t=None) == NO_DEVICE
        assert call(bd=(2048, 2048, 512)) == NO_DEVICE   # 2^31 voxels a cell: inside the range
    assert not any(cells) and not any(total)


# every condition vr_histogram2d states for its boxes, one at a time; the good call is a slab [4, 8) of 16 along z, held
# with one halo layer
GOOD_2D = dict(dims=(8, 6, 6), G=(8, 6, 16), org=(0, 0, 3), lo=(0, 0, 4), hi=(8, 6, 8))
BAD_2D = [
    dict(dims=(0, 6, 6)), dict(dims=(8, -1, 6)), dict(dims=(1 << 31, 6, 6)), dict(G=(8, 6, -16)), dict(G=(1 << 31, 6, 16)),
    dict(org=(0, -1, 3)), dict(org=(0, 0, 11)),                   # the local volume leaves the global one
    dict(lo=(0, 0, 8)), dict(lo=(8, 0, 4)), dict(hi=(8, 6, 4)), dict(lo=(0, 3, 4), hi=(8, 2, 8)),      # empty
    dict(lo=(0, 0, 2)), dict(lo=(-1, 0, 4)), dict(hi=(8, 6, 10)), dict(hi=(9, 6, 8)), dict(hi=(8, 7, 8)),   # leaves the local volume
    dict(lo=(0, 0, 3)),                                           # the neighbour below the box is not held
    dict(hi=(8, 6, 9)),                                           # the neighbour above the box is not held
    dict(dims=(8, 6, 4), org=(0, 0, 4)),                          # no halo at all: both
    dict(dims=(7, 6, 6), hi=(7, 6, 8)),                           # x: 7 of 8 voxels held, the box's last neighbour missing
    dict(dims=(8, 5, 6), org=(0, 1, 3), lo=(0, 1, 4)),            # y: the box starts where the volume does, not at 0
]
GOOD_2D_MORE = [
    dict(dims=(8, 6, 16), G=(0, 0, 0), org=(0, 0, 0), lo=(0, 0, 0), hi=(8, 6, 16)),     # the whole volume, global_dims 0
    dict(dims=(8, 6, 5), org=(0, 0, 0), lo=(0, 0, 0), hi=(8, 6, 4)),                    # the first slab: clamped at 0
    dict(dims=(8, 6, 5), org=(0, 0, 11), lo=(0, 0, 12), hi=(8, 6, 16)),                 # the last slab: clamped at G - 1
    dict(lo=(3, 0, 5), hi=(4, 6, 6)),                                                   # a box aligned to nothing
    dict(dims=(1, 1, 1), G=(1, 1, 1), org=(0, 0, 0), lo=(0, 0, 0), hi=(1, 1, 1)),
]


def call_2d(L, vol, hist, **kw):
    a = dict(GOOD_2D)
    a.update(kw)
    return L.vr_histogram2d(vol, I64x3(*a["dims"]), I64x3(*a["G"]), I64x3(*a["org"]), I64x3(*a["lo"]), I64x3(*a["hi"]), hist, None)


def test_histogram2d_rejects_bad_arguments_before_the_device(L):
    vol, hist = (C.c_uint8 * (8 * 6 * 16))(), (C.c_uint64 * (111 * 256))()
    g = GOOD_2D
    args = [vol, I64x3(*g["dims"]), I64x3(*g["G"]), I64x3(*g["org"]), I64x3(*g["lo"]), I64x3(*g["hi"]), hist]
    for k in range(7):                                             # every pointer null in turn
        holed = list(args)
        holed[k] = None
        assert L.vr_histogram2d(*holed, None) == INVALID, k
    for kw in BAD_2D:
        assert call_2d(L, vol, hist, **kw) == INVALID, kw
    if device_count(L) == 0:
        assert call_2d(L, vol, hist) == NO_DEVICE
        for kw in GOOD_2D_MORE:
            assert call_2d(L, vol, hist, **kw) == NO_DEVICE, kw
    assert not any(hist)


def test_python_wrapper_raises_value_error_before_anything_touches_a_device():
    """The same box conditions as ValueError: the checks come before the volume is moved to a device."""
    import torch
    from volumerenderer_amd import render as R
    vol = torch.zeros(1, dtype=torch.uint8)
    for kw in BAD_2D:
        a = dict(GOOD_2D)
        a.update(kw)
        with pytest.raises(ValueError):
            R.histogram2d(vol, a["dims"], a["G"], a["org"], a["lo"], a["hi"])
    for args in ((vol, (8, 6)), (vol, (8, 6, 6), (8, 6)), (vol, (8, 6, 6), None, 3), (vol, (8, 6, 6), None, (0, 0, 0), (1, 1))):
        with pytest.raises(ValueError):
            R.histogram2d(*args)


def test_window_wrapper_raises_value_error(L):
    from volumerenderer_amd import render as R
    h = np.zeros(256, np.uint64)
    h[40] = 7
    assert R.window_from_histogram(h) == (np.float32(40) / np.float32(255), np.float32(41) / np.float32(255))
    for args in ((h[:255],), (h.astype(np.float64),), (h, -1), (h, 256), (h, 0, -0.1, 0.5), (h, 0, 0.5, 1.1), (h, 0, 0.6, 0.5),
                 (h, 0, math.nan, 0.5), (h, 41), (np.zeros(256, np.uint64),), (-h.astype(np.int64),)):
        with pytest.raises(ValueError):
            R.window_from_histogram(*args)
    h2 = np.zeros((111, 256), np.uint64)                           # a 2-D table: its column sums
    h2[0, 10], h2[7, 200] = 5, 5
    assert R.window_from_histogram(h2, 0, 0.0, 1.0) == (np.float32(10) / np.float32(255), np.float32(200) / np.float32(255))


# ---- the window rule ---------------------------------------------------------------------------------------------------
def window_c(L, hist, first_bin, lo, hi):
    h = (C.c_uint64 * 256)(*[int(v) for v in hist])
    wl, wh = C.c_float(-7.0), C.c_float(-7.0)
    rc = L.vr_window_from_histogram(h, first_bin, lo, hi, C.byref(wl), C.byref(wh))
    if rc != 0:
        assert rc == INVALID and wl.value == -7.0 and wh.value == -7.0      # refused: nothing written
        return None
    return np.float32(wl.value), np.float32(wh.value)


def check_window(L, hist, first_bin, lo, hi):
    import refhist
    want, got = refhist.window(hist, first_bin, lo, hi), window_c(L, hist, first_bin, lo, hi)
    assert got == want, (first_bin, lo, hi, got, want)
    if got is not None:
        assert 0.0 <= got[0] < got[1] <= 1.0                       # what vr_raycast_projection accepts
        assert got[0] == np.float32(round(float(got[0]) * 255)) / np.float32(255)
    return got


def test_window_rule_on_hand_made_histograms(L):
    f = lambda k: np.float32(k) / np.float32(255)
    spike = np.zeros(256, np.uint64)
    spike[100] = 1000
    assert check_window(L, spike, 0, 0.01, 0.99) == (f(100), f(101))
    assert check_window(L, spike, 0, 0.0, 1.0) == (f(100), f(101))
    assert check_window(L, spike, 0, 1.0, 1.0) == (f(100), f(101))          # no bin passes all of N: the last populated one
    assert check_window(L, spike, 0, 0.0, 0.0) == (f(100), f(101))          # hi_k = first_bin <= lo_k
    assert check_window(L, spike, 100, 0.5, 0.5) == (f(100), f(101))
    assert check_window(L, spike, 101, 0.01, 0.99) is None                   # all the mass below first_bin
    top = np.zeros(256, np.uint64)
    top[255] = 3
    assert check_window(L, top, 0, 0.01, 0.99) == (f(254), f(255))           # 256 would pass the end: both move down
    assert check_window(L, top, 255, 0.0, 1.0) == (f(254), f(255))
    two = np.zeros(256, np.uint64)
    two[0], two[30], two[220] = 10 ** 12, 500, 500                          # a background that dwarfs the data
    assert check_window(L, two, 0, 0.01, 0.99) == (f(0), f(1))
    assert check_window(L, two, 1, 0.01, 0.99) == (f(30), f(220))
    assert check_window(L, two, 1, 0.5, 0.5) == (f(220), f(221))             # cum_30 = N/2 is not above N/2; equal fractions
    assert check_window(L, two, 1, 0.0, 0.5) == (f(30), f(31))               # ... but it reaches it
    big = np.zeros(256, np.uint64)
    big[3], big[9] = (1 << 62) + 1, 1 << 62                                  # counts no double holds exactly
    check_window(L, big, 0, 0.5, 0.5)
    for first, lo, hi in ((-1, 0.1, 0.9), (256, 0.1, 0.9), (0, -0.01, 0.9), (0, 0.1, 1.01), (0, 0.9, 0.1), (0, math.nan, 0.9),
                          (0, 0.1, math.nan), (0, math.inf, math.inf)):
        assert window_c(L, spike, first, lo, hi) is None, (first, lo, hi)
    assert window_c(L, np.zeros(256, np.uint64), 0, 0.1, 0.9) is None        # N == 0
    wl = C.c_float()
    assert L.vr_window_from_histogram(None, 0, 0.1, 0.9, C.byref(wl), C.byref(wl)) == INVALID
    h = (C.c_uint64 * 256)(*[1] * 256)
    assert L.vr_window_from_histogram(h, 0, 0.1, 0.9, None, C.byref(wl)) == INVALID
    assert L.vr_window_from_histogram(h, 0, 0.1, 0.9, C.byref(wl), None) == INVALID


def test_window_rule_equals_its_restatement_on_random_histograms(L):
    rng = np.random.default_rng(2025)
    kinds = {"clamped": 0, "shifted": 0, "wide": 0}
    for case in range(200):
        h = rng.integers(0, 1 << int(rng.integers(1, 40)), 256).astype(np.uint64)
        if case % 3 == 0:                                          # sparse: a few populated bins
            h[rng.random(256) < 0.95] = 0
            h[int(rng.integers(0, 256))] += 1
        if case % 7 == 0:
            h[255] += 1 << 41                                      # most of the mass in the last bin
        first = int(rng.choice([0, 0, 1, int(rng.integers(0, 256))]))
        lo = float(rng.choice([0.0, 0.01, 0.05, 0.5, float(rng.random())]))
        hi = float(rng.choice([lo, 0.99, 1.0, lo + (1.0 - lo) * float(rng.random())]))
        if hi < lo:
            hi = lo
        got = check_window(L, h, first, lo, hi)
        if got is not None:
            lo_k, hi_k = round(float(got[0]) * 255), round(float(got[1]) * 255)
            kinds["clamped"] += int(hi_k == lo_k + 1)
            kinds["shifted"] += int(hi_k == 255 and h[255] > 0 and lo_k == 254)
            kinds["wide"] += int(hi_k > lo_k + 1)
    assert all(v > 0 for v in kinds.values()), kinds


# ---- the integer square root -----------------------------------------------------------------------------------------------
def test_refhist_isqrt_is_exact_over_the_whole_range():
    import refhist
    s = np.arange(0, 3 * 255 * 255 + 1)
    assert [int(v) for v in refhist.isqrt(s)] == [math.isqrt(int(v)) for v in s]
    assert int(refhist.isqrt(3 * 255 * 255)) >> 2 == 110 == refhist.GRAD_BINS - 1


# ---- slabs ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("world", [2, 3, 5, 8])
def test_slab_voxels_tile_the_volume_and_pass_the_box_check(L, world):
    from volumerenderer_amd import distributed as D
    dims = (28, 20, 24)
    vol, hist = (C.c_uint8 * (28 * 20 * 24))(), (C.c_uint64 * (111 * 256))()
    want = NO_DEVICE if device_count(L) == 0 else None
    for axis in range(3):
        owned = np.zeros(dims[::-1], np.int32)
        for rank in range(world):
            org, lo, hi, local, (a0, a1) = D.slab_voxels(dims, axis, rank, world)
            assert org[axis] == a0 and local[axis] == a1 - a0 and a0 == max(0, lo[axis] - 1) and a1 == min(dims[axis], hi[axis] + 1)
            assert all(org[k] == 0 and lo[k] == 0 and hi[k] == dims[k] and local[k] == dims[k] for k in range(3) if k != axis)
            owned[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] += 1
            if want is not None:                                   # (with a device the GPU tests make these calls)
                assert call_2d(L, vol, hist, dims=local, G=dims, org=org, lo=lo, hi=hi) == want
            # no halo: refused wherever the slab has a neighbour
            org0, lo0, hi0, local0, _ = D.slab_voxels(dims, axis, rank, world, halo=0)
            assert (lo0, hi0) == (lo, hi)
            assert call_2d(L, vol, hist, dims=local0, G=dims, org=org0, lo=lo0, hi=hi0) == INVALID
        assert np.all(owned == 1)
    for bad in (dict(axis=3), dict(rank=world), dict(rank=-1), dict(halo=-1)):
        kw = dict(dims=dims, axis=0, rank=0, world=world, halo=1)
        kw.update(bad)
        with pytest.raises(ValueError):
            D.slab_voxels(**kw)
    with pytest.raises(ValueError):
        D.slab_voxels((4, 4, 4), 1, 0, 5)                           # more ranks than layers


# ---- the all-reduce ------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rank_tables(rank):
    rng = np.random.default_rng(100 + rank)
    h2 = rng.integers(0, 1 << 40, (111, 256)).astype(np.uint64)
    h1 = rng.integers(0, 1 << 31, 256).astype(np.uint32)
    return h2, h1


def _reduce_worker(rank, world, port, out_dir):
    import torch
    import torch.distributed as dist
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from volumerenderer_amd import distributed as D
        h2, h1 = _rank_tables(rank)
        r2, r1 = D.histogram_all_reduce(h2), D.histogram_all_reduce(h1.astype(np.uint64))
        rt = D.histogram_all_reduce(torch.from_numpy(h1.astype(np.int64)))
        assert isinstance(r2, np.ndarray) and r2.dtype == np.uint64 and r2.shape == (111, 256)
        assert isinstance(rt, torch.Tensor) and rt.dtype == torch.int64
        assert np.array_equal(h2, _rank_tables(rank)[0])            # the input is left alone
        np.savez(os.path.join(out_dir, "rank%d.npz" % rank), r2=r2, r1=r1, rt=rt.numpy())
    finally:
        dist.destroy_process_group()


def test_histogram_all_reduce_over_gloo(tmp_path):
    import torch.multiprocessing as mp
    from volumerenderer_amd import distributed as D
    world = 3
    mp.spawn(_reduce_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    want2 = sum(_rank_tables(r)[0] for r in range(world))
    want1 = sum(_rank_tables(r)[1].astype(np.uint64) for r in range(world))
    for r in range(world):
        got = np.load(str(tmp_path / ("rank%d.npz" % r)))
        assert np.array_equal(got["r2"], want2) and np.array_equal(got["r1"], want1) and np.array_equal(got["rt"], want1.astype(np.int64))
    # no process group: the identity
    h = _rank_tables(0)[0]
    assert D.histogram_all_reduce(h) is h


# ---- the example ---------------------------------------------------------------------------------------------------------------
def compile_example(out_dir):
    """examples/histogram.cpp (vrhip/Histogram.hpp) built with g++ against libvrhip.so; returns the program's path."""
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(str(out_dir), "histogram")
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "histogram.cpp"), "-L" + lib, "-lvrhip",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_example_compiles_and_is_loud_without_a_gpu(L, tmp_path):
    exe = compile_example(tmp_path)
    if device_count(L) == 0:
        r = subprocess.run([exe], capture_output=True, text=True)
        assert r.returncode != 0 and "no usable HIP device" in (r.stdout + r.stderr)


def test_header_constants_match_python():
    from volumerenderer_amd import render as R
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    assert "#define VR_HIST_BINS      256" in hdr and "#define VR_HIST_GRAD_BINS 111" in hdr
    assert (R.HIST_BINS, R.HIST_GRAD_BINS) == (256, 111) and math.isqrt(3 * 255 * 255) >> 2 == 110
