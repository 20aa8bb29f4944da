"""Error-bounded level of detail on the GPU: k_brick_error against NumPy (exact integers, every path of the kernel,
buffers at byte offsets), vr_brickset_error_table against bs.decode(cut) plus NumPy for every kind of set, and the
selection end to end: cuts chosen with bound 0 decode, pool and draw exactly what the full depth does."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


# ---- the kernel ----------------------------------------------------------------------------------------------------
def errors_py(a, b, B):
    from volumerenderer_amd.codec import BRICK_ERROR
    d = np.abs(a.astype(np.int64).reshape(B, -1) - b.astype(np.int64).reshape(B, -1))
    out = np.zeros(B, BRICK_ERROR)
    out["sum_abs"], out["sum_sq"], out["max_abs"], out["num_diff"] = d.sum(1), (d * d).sum(1), d.max(1), (d != 0).sum(1)
    return out


def at_offset(host, off):
    """host's bytes on the device, `off` bytes past an aligned allocation."""
    import torch
    buf = torch.zeros(host.size + 16, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + host.size]
    view.copy_(torch.from_numpy(host))
    assert view.data_ptr() % 16 == off % 16
    return view


def check_kernel(vr, B, V, offsets, seed):
    rng = np.random.default_rng(seed)
    a, b = rng.integers(0, 256, B * V, dtype=np.uint8), rng.integers(0, 256, B * V, dtype=np.uint8)
    eq = rng.integers(0, B * V, B * V // 2)                     # (some equal pairs, wherever they fall)
    b[eq] = a[eq]
    want = errors_py(a, b, B)
    for oa, ob in offsets:
        da, db = at_offset(a, oa), at_offset(b, ob)
        got = vr.measure_error_bricks(da, db, B)
        assert np.array_equal(got, want), (B, V, oa, ob, got[:2], want[:2])
        same = vr.measure_error_bricks(da, at_offset(a, ob), B)
        assert not same["sum_abs"].any() and not same["sum_sq"].any() and not same["max_abs"].any() \
            and not same["num_diff"].any(), (B, V, oa, ob)


@pytest.mark.parametrize("B", [1, 3, 70])
@pytest.mark.parametrize("V", [1, 15, 16, 17, 4101])
def test_kernel_equals_numpy_at_every_pair_of_offsets(vr, V, B):
    check_kernel(vr, B, V, [(oa, ob) for oa in (0, 1, 3) for ob in (0, 1, 3)], seed=V * 100 + B)


@pytest.mark.parametrize("V", [63, 64, 65, 256, 257, 1024, 1025, 4096, 4097, 16384, 16385, 40000])
def test_kernel_equals_numpy_around_its_thresholds(vr, V):
    """The team widths of the small kernel (64 bytes per lane and step), the step to one workgroup per brick (4096) and
    to several parts per brick (16384)."""
    check_kernel(vr, 5, V, [(0, 0), (1, 1), (1, 3)], seed=V)


def test_sums_do_not_overflow(vr):
    import torch
    V = 64 ** 3
    a = torch.zeros(2 * V, dtype=torch.uint8, device="cuda")
    b = torch.full((2 * V,), 255, dtype=torch.uint8, device="cuda")
    got = vr.measure_error_bricks(a, b, 2)
    for e in got:
        assert (int(e["sum_sq"]), int(e["sum_abs"]), int(e["max_abs"]), int(e["num_diff"])) == \
            (17045913600, 66846720, 255, 262144)
    # one brick of the same bytes: fewer, longer parts per workgroup
    one = vr.measure_error_bricks(a, b, 1)[0]
    assert (int(one["sum_sq"]), int(one["sum_abs"]), int(one["max_abs"]), int(one["num_diff"])) == \
        (2 * 17045913600, 2 * 66846720, 255, 2 * 262144)


def test_one_large_brick(vr):
    check_kernel(vr, 1, 128 ** 3, [(0, 0), (3, 3)], seed=7)


def test_many_tiny_bricks(vr):
    check_kernel(vr, 5000, 64, [(0, 0), (1, 3)], seed=8)


# ---- the table -----------------------------------------------------------------------------------------------------
def check_table(vr, bs, vox):
    """Every cut 0 .. M against bs.decode(cut_depth=c) plus NumPy: against the original voxels (where there are any),
    against the set's own full decode (last row all zero), against a coarse decode; a sub-range equals its rows."""
    import torch
    from test_error_table_cpu import table_py
    B, V = bs.num_bricks, bs.voxels_per_brick
    M = bs.info(0)["max_tree_depth"]
    decs = [bs.decode(cut_depth=c).cpu().numpy().reshape(B, V).copy() for c in range(M + 1)]
    full = bs.decode().cpu().numpy().reshape(B, V).copy()
    assert np.array_equal(full, decs[M])
    t_full = bs.error_table()
    assert t_full.shape == (M + 1, B)
    assert np.array_equal(t_full, table_py(decs, full))
    for f in ("sum_abs", "sum_sq", "max_abs", "num_diff"):
        assert not t_full[M][f].any()
    refs = [torch.from_numpy(decs[M // 2].reshape(-1)).cuda()]
    if vox is not None:
        refs.append(np.ascontiguousarray(vox, np.uint8).reshape(-1))
    scratch = torch.empty(B * V, dtype=torch.uint8, device="cuda")
    for ref in refs:
        host = ref.cpu().numpy() if isinstance(ref, torch.Tensor) else ref
        t = bs.error_table(reference=ref, scratch=scratch)
        assert np.array_equal(t, table_py(decs, host.reshape(B, V)))
        assert np.array_equal(scratch.cpu().numpy().reshape(B, V), decs[M])       # left with the decode at cut_hi
        lo, hi = M // 3, M - 2
        assert np.array_equal(bs.error_table(reference=ref, cuts=(lo, hi)), t[lo:hi + 1])
        assert np.array_equal(bs.error_table(reference=ref, cuts=(M, M)), t[M:])
    return t_full


@pytest.fixture(scope="module")
def known_set(vr, oracle):
    """The four bricks with known answers and four more rm_like seeds: 16^3, tolerance 2, 3 epochs."""
    from test_error_table_cpu import known_bricks
    from test_gpu_lod import rm_like
    vols = known_bricks(oracle) + [rm_like((16, 16, 16), s) for s in (5, 6, 7, 8)]
    bs = vr.BrickSet(8, (16, 16, 16), 2, 3)
    bs.build(np.stack(vols))
    return bs, np.stack(vols)


def test_table_16cubed_bricks_and_the_oracle_column(vr, known_set):
    from test_error_table_cpu import KNOWN_RM_LIKE_MAX_ABS
    bs, vox = known_set
    t = check_table(vr, bs, vox)
    assert [int(v) for v in t["max_abs"][:, 2]] == KNOWN_RM_LIKE_MAX_ABS


def test_table_64cubed_bricks(vr):
    from test_gpu_lod import rm_like
    vox = np.stack([rm_like((64, 64, 64), 1), rm_like((64, 64, 64), 2)[::-1].copy()])
    check_table(vr, vr.BrickSet(2, (64, 64, 64), 1, 2).build(vox), vox)


def test_table_tiled_geometry(vr):
    from test_gpu_lod import rm_like
    vox = rm_like((64, 64, 128), 4)[None]
    check_table(vr, vr.BrickSet(1, (128, 64, 64), 1, 2).build(vox), vox)


def test_table_general_extents(vr):
    """12 x 10 x 7 bricks: 840 bytes each, so the second and third start at no multiple of 16 (the peeled path)."""
    rng = np.random.default_rng(31)
    z, y, x = np.meshgrid(np.arange(7), np.arange(10), np.arange(12), indexing="ij")
    vox = np.stack([np.clip(20 * z + 9 * y + 3 * x * s + rng.integers(0, 4, z.shape), 0, 255).astype(np.uint8) for s in (1, 2, 3)])
    check_table(vr, vr.BrickSet(3, (12, 10, 7), 2, 3).build(vox), vox)


def test_table_midrange_set(vr, oracle):
    from volumerenderer_amd import _lib
    from test_gpu_lod import rm_like
    vox = np.stack([rm_like((16, 16, 16), 12), oracle.gen_sphere(16, 7)])
    check_table(vr, vr.BrickSet(2, (16, 16, 16), 2, 3, variant=_lib.VARIANT_MIDRANGE).build(vox), vox)


def test_table_of_a_set_opened_from_a_file(vr):
    bs = vr.BrickSet.open(os.path.join(GOLD, "ref_sphere_n3_16_tol1_ep2.tree.bin"))
    check_table(vr, bs, None)


def test_table_argument_checks_with_a_set(vr):
    import torch
    from volumerenderer_amd import _lib
    L = _lib.lib()
    from test_gpu_lod import rm_like
    vox = rm_like((64, 64, 128), 4)[None]
    bs = vr.BrickSet(1, (128, 64, 64), 1, 2)
    n = bs.voxels_per_brick
    ref = torch.zeros(n, dtype=torch.uint8, device="cuda")
    scratch = torch.full((n + 16,), 0xA5, dtype=torch.uint8, device="cuda")
    M = 7 + 6 + 6 + 7                                          # (a set has no info before its build)
    tab = np.zeros(M + 1, vr.BRICK_ERROR)

    def call(h=bs._h, r=ref.data_ptr(), s=scratch.data_ptr(), lo=0, hi=M, t=tab.ctypes.data):
        return L.vr_brickset_error_table(h, C.c_void_p(r), C.c_void_p(s), lo, hi, C.c_void_p(t), None)

    assert call() == -5                                        # VR_ERR_STATE: before build
    bs.build(vox)
    assert bs.info(0)["max_tree_depth"] == M
    for kw in (dict(h=None), dict(r=None), dict(s=None), dict(t=None), dict(lo=-1), dict(hi=M + 1), dict(lo=5, hi=4),
               dict(s=scratch.data_ptr() + 1), dict(s=scratch.data_ptr() + 8)):   # tiled geometry: 16-byte stores
        assert call(**kw) == -1, kw
    torch.cuda.synchronize()
    assert torch.all(scratch == 0xA5) and not tab["num_diff"].any()              # nothing launched, nothing written
    assert call() == 0


# ---- selection end to end ----------------------------------------------------------------------------------------------
def test_cuts_selected_with_bound_zero_lose_nothing(vr, oracle):
    import torch
    from test_error_table_cpu import KNOWN_CUTS, known_bricks
    vox = np.stack(known_bricks(oracle))
    bs = vr.BrickSet(4, (16, 16, 16), 2, 3).build(vox)
    B, V = 4, 4096
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    full = bs.decode().clone()
    table = bs.error_table(reference=full)
    cuts = vr.select_lod_error(table, 0, V)
    assert list(cuts) == KNOWN_CUTS
    assert list(vr.select_lod_error(table, 0, V, cuts_in=[-1, 2, 19, 10])) == [-1, 2, 17, 10]
    assert torch.equal(bs.decode_lod(cuts), full)
    # a smaller pool, the same frame
    ijk, grid, bd, dims = np.array([(0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0)]), (2, 2, 1), (16, 16, 16), (32, 32, 16)
    _, bytes_sel = vr.lod_pool_layout(bd, ijk, grid, cuts, D, M)
    _, bytes_full = vr.lod_pool_layout(bd, ijk, grid, np.full(B, M, np.int32), D, M)
    assert bytes_sel < bytes_full
    pool, tab = bs.decode_lod_pool(cuts, ijk, grid)
    assert pool.numel() == bytes_sel
    cam, P = vr.default_camera(), vr.default_params(96, 64, dims)
    want = vr.raycast(vr.assemble_bricks(full, bd, ijk, grid), dims, cam, P)
    assert torch.equal(vr.raycast_pool(pool, tab, bd, grid, cam, P), want)
    assert len(torch.unique(want)) > 8                          # (a frame with the volume in it)
    # the rate / distortion curve: bytes grow and the error at the last cut is none
    rd = vr.rate_distortion(bs, table, ijk, grid)
    assert list(rd["cut"]) == list(range(M + 1)) and np.all(np.diff(rd["pool_bytes"]) >= 0)
    assert rd["pool_bytes"][M] == bytes_full and np.isinf(rd["psnr"][M]) and np.isfinite(rd["psnr"][0])
    # a bound of 4 grey levels buys one more level on the two busy bricks
    cuts4 = vr.select_lod_error(table, 0, V, max_abs=4)
    assert list(cuts4[2:]) == [16, 16] and np.all(cuts4 <= cuts)
    d = (bs.decode_lod(cuts4).to(torch.int16) - full.to(torch.int16)).abs().reshape(B, V).amax(1)
    assert int(d.max()) <= 4 and [int(v) for v in d] == [int(table[c, b]["max_abs"]) for b, c in enumerate(cuts4)]


def test_two_tables_queued_on_one_side_stream(vr, known_set):
    import torch
    bs, vox = known_set
    ref = torch.from_numpy(vox.reshape(-1)).cuda()
    alone = bs.error_table(reference=ref)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    first = bs.error_table(reference=ref, stream=s)
    second = bs.error_table(reference=ref, cuts=(2, 9), stream=s)
    third = bs.error_table(stream=s)                               # (its reference is decoded on the same stream)
    assert np.array_equal(first, alone) and np.array_equal(second, alone[2:10])
    assert np.array_equal(third, bs.error_table())


# ---- the example ---------------------------------------------------------------------------------------------------
def test_cpp_example_prints_the_python_table_and_equal_hashes(vr, oracle, tmp_path):
    from test_error_table_cpu import KNOWN_CUTS, compile_example, known_bricks
    exe = compile_example(tmp_path)
    vox = np.stack(known_bricks(oracle))
    raw = tmp_path / "bricks.raw"
    raw.write_bytes(vox.tobytes())
    r = subprocess.run([exe, str(raw)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().splitlines()
    table = vr.BrickSet(4, (16, 16, 16), 2, 3).build(vox).error_table()
    for b in range(4):
        w = lines[b].split()
        assert w[:3] == ["brick", str(b), "max_abs"] and [int(v) for v in w[3:]] == [int(v) for v in table["max_abs"][:, b]]
    assert lines[4].split() == ["cuts"] + [str(c) for c in KNOWN_CUTS]
    w = lines[5].split()
    assert w[0:2] == ["lod", "fnv1a64"] and w[3:5] == ["full", "fnv1a64"] and w[2] == w[5] and len(w[2]) == 16
    # the built-in bricks: the same promise
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    w = r.stdout.strip().splitlines()[-1].split()
    assert w[2] == w[5]
