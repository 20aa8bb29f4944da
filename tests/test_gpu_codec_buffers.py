"""Where the codec's kernels read and write relative to the buffers a caller hands in (include/vrhip.h, "alignment of
caller buffers" and the "Alignment:" line of each codec entry point).

 * test_offset_views_codec: every caller buffer at byte offsets 1..15 (16 = the aligned control) inside allocations
   poisoned with 0xA5 / 0x5A.  A call that would launch a kernel with vector accesses to the caller's buffer is refused
   with VR_ERR_INVALID and writes nothing; every other call works at any offset, equals the oracle and leaves the bands
   on both sides alone.
 * test_guard_bands_aligned: at aligned views with >= 4096 bytes of band on each side every decode entry point, on
   every decode kernel, writes exactly the bytes it owns -- for 1, 2 and 5 bricks.
 * test_batched_odd_sized_bricks: bricks with an odd voxel count start misaligned inside the set's own buffers.

Expected values are the oracle's (oracle.OracleTree), compared a second time with the GPU's own result from plainly
allocated buffers.

The shape table, (z, y, x): the header's two geometry terms decide which calls are vector-path.  128 x 8 x 4 has no
tiled geometry (its six deepest levels split x, y, x, x, x, x): it decodes through k_decode_lane, and the smallest
brick the tiled kernels (tile / fine / quad / region) serve is 128 x 64 x 64, which is therefore in the table too."""
import ctypes as C

import numpy as np
import pytest

from test_gpu_codec import _mixed_volume, rm_like

pytestmark = pytest.mark.gpu

IN_POISON, OUT_POISON = 0xA5, 0x5A
BAND = 4096
VR_ERR_INVALID, VR_ERR_UNSUPPORTED = -1, -7
TOL, EP = 1, 2
VOLUME_KDTREE, MIDRANGE = 0, 2

# (z, y, x) -> (x-run geometry: build is vector-path, tiled geometry: every decode is vector-path)
SHAPES = {
    (8, 8, 8): (False, False),          # D = 9: k_pyramid<true> rounds, k_decode_lane
    (16, 16, 16): (True, False),        # D = 12: the smallest k_pyramid12 build; k_decode_lane
    (32, 8, 16): (True, False),
    (4, 8, 128): (True, False),
    (64, 64, 128): (True, True),        # the smallest tiled brick: tile / fine / quad / region by the switches
    (64, 128, 128): (True, True),
    (5, 9, 7): (False, False),          # general extents, V = 315: k_decode_lane<true> + k_owner_gather
    (3, 1, 1): (False, False),
}
# the set's decode switches -> the kernel a tiled set then uses at cuts >= D-3 / above
SWITCHES = {"region": None, "quad": "decode_quad", "fine": "decode_fine_v1", "tile": "decode_walk"}


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


# ---- the header's rule, restated ---------------------------------------------------------------------------------------
def _pow2(v):
    return v > 0 and v & (v - 1) == 0


def split_axes(X, Y, Z):
    """Depth d splits axis d % 3, or the next axis that still has more than one voxel (vrhip.h, vr_lod_pool_layout)."""
    ext, axes = [X, Y, Z], []
    for d in range(sum(v.bit_length() - 1 for v in ext)):
        sd, i = d % 3, 0
        while ext[0] * ext[1] * ext[2] > 1 and ext[sd] == 1:
            i += 1
            sd = (d + i) % 3
        ext[sd] //= 2
        axes.append(sd)
    return axes


def x_run_geometry(X, Y, Z):
    if not all(_pow2(v) and v <= 1024 for v in (X, Y, Z)):
        return False
    axes = split_axes(X, Y, Z)
    return len(axes) >= 12 and axes[-12:].count(0) >= 4


def tiled_geometry(X, Y, Z):
    if not all(_pow2(v) and v <= 1024 for v in (X, Y, Z)) or X < 128:
        return False
    lg = tuple(v.bit_length() - 1 for v in (X, Y, Z))
    m = min(lg)
    return lg in ((m, m, m), (m + 1, m, m), (m + 1, m + 1, m))


def test_shape_table_is_the_headers_rule():
    for (z, y, x), want in SHAPES.items():
        assert (x_run_geometry(x, y, z), tiled_geometry(x, y, z)) == want, (z, y, x)
    for x, y, z in ((128, 32, 16), (64, 64, 64)):
        assert not tiled_geometry(x, y, z)
    for x, y, z in ((128, 128, 64), (128, 128, 128), (256, 256, 128), (256, 256, 256)):
        assert tiled_geometry(x, y, z) and x_run_geometry(x, y, z)
    assert not x_run_geometry(8, 64, 64)


# ---- volumes and oracle trees, computed once and shared ----------------------------------------------------------------
_REFS = {}
_CUTS = {}


def ref_brick(oracle, shape, i, midrange):
    """Brick i of a shape: 0 mixed boxes, 1 rm_like, 2 constant, 3 noise, then again with other seeds."""
    key = (shape, i, midrange)
    if key not in _REFS:
        rng = np.random.default_rng(7000 + 31 * i + sum(shape))
        kind = i % 4
        vol = (_mixed_volume(rng, shape) if kind == 0 else rm_like(shape, 3 + i) if kind == 1 else
               np.full(shape, (37 + 50 * i) & 255, np.uint8) if kind == 2 else rng.integers(0, 256, shape, dtype=np.uint8))
        _REFS[key] = (vol, oracle.OracleTree(vol.copy(), tolerance=TOL, max_epochs=EP, midrange=midrange,
                                             guarded=midrange).build())
    return _REFS[key]


def want(oracle, shape, i, midrange, cut, rng_stream=False):
    """The oracle's decode of brick i at `cut` (None or maxTreeDepth = levelCut), flat."""
    key = (shape, i, midrange, cut, rng_stream)
    if key not in _CUTS:
        ref = ref_brick(oracle, shape, i, midrange)[1]
        full = cut is None or cut >= ref.maxTreeDepth
        if rng_stream:
            v = ref.levelCutRange(None if full else cut)
        else:
            v = ref.levelCut() if full else ref.levelCutProgressive(cut)
        _CUTS[key] = np.ascontiguousarray(v).reshape(-1).copy()
    return _CUTS[key]


def set_volumes(oracle, shape, bricks, midrange):
    """`bricks`: the brick kinds of the set, e.g. (0, 2) = a mixed and a constant brick."""
    return np.stack([ref_brick(oracle, shape, i, midrange)[0] for i in bricks])


def the_cuts(D, M):
    return sorted({c for c in (D - 7, D - 3, D, M - 1) if c >= 0}) + [None]


# ---- poisoned allocations -----------------------------------------------------------------------------------------------
class Window:
    """n bytes at `offset` bytes past a 256-byte boundary, inside an allocation filled with `poison`, at least BAND
    bytes of it on each side."""

    def __init__(self, n, offset, poison):
        import torch
        self.n, self.poison = n, poison
        self.base = torch.full((BAND + 256 + offset + n + BAND,), poison, dtype=torch.uint8, device="cuda")
        self.start = BAND + (-(self.base.data_ptr() + BAND)) % 256 + offset
        self.view = self.base[self.start:self.start + n]
        assert self.view.data_ptr() % 256 == offset % 256 and self.view.numel() == n
        assert self.start >= BAND and self.base.numel() - self.start - n >= BAND

    def fill(self, host):
        import torch
        self.view.copy_(torch.from_numpy(np.ascontiguousarray(host).reshape(-1)))
        return self

    def read(self):
        """(the view's bytes, True if both bands still hold the poison)"""
        h = self.base.cpu().numpy()
        a, b = self.start, self.start + self.n
        return h[a:b].copy(), bool(np.all(h[:a] == self.poison) and np.all(h[b:] == self.poison))

    def untouched(self):
        return bool(np.all(self.base.cpu().numpy() == self.poison))


def refused(vr, call):
    """The call raises VR_ERR_INVALID."""
    with pytest.raises(vr.VrError) as ei:
        call()
    assert ei.value.status == VR_ERR_INVALID, ei.value
    return True


def check_built(oracle, bs, shape, bricks, midrange, what):
    """Tree bytes, distance maps and info of every brick against its own oracle tree."""
    for b, i in enumerate(bricks):
        ref = ref_brick(oracle, shape, i, midrange)[1]
        info, st = bs.info(b), ref.leaf_stats()
        w = (what, b)
        assert info["orig_tree_depth"] == ref.origTreeDepth and info["max_tree_depth"] == ref.maxTreeDepth, w
        assert info["num_active_nodes"] == ref.numActiveNodes and info["num_reverts"] == ref.numReverts, w
        assert info["max_error_before"] == st["max_before"] and info["max_error_after"] == st["max_after"], w
        assert abs(info["mean_l1_after"] - st["l1_after"]) < 1e-12 and info["zero_run_rewrites"] == 0, w
        assert np.array_equal(bs.tree(b), ref.tree), w
        assert list(bs.distance_map(b)) == list(ref.distanceMap), w
        if midrange:
            assert np.array_equal(bs.tree_range(b), ref.tree_range), w
            assert list(bs.distance_map_range(b)) == list(ref.distanceMap_range), w
            assert np.array_equal(bs.packed4(b), ref.convertToByteArray()), w


def lod_plan(B, D, M, culled):
    """Mixed per-brick cuts, brick `culled` skipped."""
    pool = [c for c in (M, D - 3, D, M - 1, D - 7, 0) if c >= 0]
    return np.array([-1 if b == culled else pool[b % len(pool)] for b in range(B)], np.int32)


def check_lod_bytes(oracle, got, shape, bricks, midrange, cuts, poison, what):
    V = int(np.prod(shape))
    for b, i in enumerate(bricks):
        if cuts[b] < 0:
            assert np.all(got[b * V:(b + 1) * V] == poison), (what, "culled brick written", b)
        else:
            assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, midrange, int(cuts[b]))), (what, b, cuts[b])


def pool_plans(B, D, M):
    """(name, cuts): every brick at full resolution (straight to its slot); coarse bricks with stored rows of >= 4
    voxels where the brick allows it (k_pool_pack's words), one culled; one voxel per brick (k_pool_pack's bytes)."""
    full = np.full(B, M, np.int32)
    coarse = np.array([-1 if b == B - 1 and B > 1 else (max(D - 3, 0) if b % 2 == 0 else M) for b in range(B)], np.int32)
    one = np.array([-1 if b == 0 and B > 1 else 0 for b in range(B)], np.int32)
    return [("full", full), ("coarse", coarse), ("one voxel", one)]


def pool_is_vector_path(dims, tiled, table, cuts, ijk, grid):
    for b, c in enumerate(cuts):
        if c < 0:
            continue
        e = table[ijk[b][0] + grid[0] * (ijk[b][1] + grid[1] * ijk[b][2])]
        sh = [int(v) for v in e["shift"]]
        if (tiled if not any(sh) else (dims[0] >> sh[0]) >= 4):
            return True
    return False


def check_pool_bytes(oracle, got, shape, bricks, midrange, cuts, table, ijk, grid, poison, what):
    z, y, x = shape
    used = np.zeros(got.size, bool)
    for b, i in enumerate(bricks):
        e = table[ijk[b][0] + grid[0] * (ijk[b][1] + grid[1] * ijk[b][2])]
        if cuts[b] < 0:
            assert e["offset"] == -1
            continue
        sx, sy, sz = (int(v) for v in e["shift"])
        dense = want(oracle, shape, i, midrange, int(cuts[b])).reshape(shape)
        stored = dense[::1 << sz, ::1 << sy, ::1 << sx].reshape(-1)
        o = int(e["offset"])
        assert o % 256 == 0 and o + stored.size <= got.size, (what, b)
        used[o:o + stored.size] = True
        assert np.array_equal(got[o:o + stored.size], stored), (what, b, cuts[b], (sx, sy, sz))
    assert np.all(got[~used] == poison), (what, "pool bytes outside the decoded slots written")


def run_pool(vr, oracle, bs, shape, bricks, midrange, cuts, offset, tiled, what):
    """decode_lod_pool with the pool (exactly the layout's bytes) and the table at byte offsets; returns True if the
    call was vector-path."""
    from volumerenderer_amd.render import POOL_ENTRY
    B = len(bricks)
    ijk, grid = np.array([(b, 0, 0) for b in range(B)], np.int64), (B, 1, 1)
    info = bs.info(0)
    table, nbytes = vr.lod_pool_layout(bs.dims, ijk, grid, cuts, info["orig_tree_depth"], info["max_tree_depth"])
    assert nbytes > 0
    pool = Window(nbytes, offset, OUT_POISON)
    tab = Window(B * POOL_ENTRY.itemsize, (offset + 5) % 16 or 16, IN_POISON)
    vector = pool_is_vector_path(bs.dims, tiled, table, cuts, ijk, grid)
    if vector and offset % 16:
        assert refused(vr, lambda: bs.decode_lod_pool(cuts, ijk, grid, pool=pool.view, table=tab.view))
        assert pool.untouched() and tab.untouched(), (what, "refused call wrote")
        return True
    bs.decode_lod_pool(cuts, ijk, grid, pool=pool.view, table=tab.view)
    got, ok = pool.read()
    assert ok, (what, "pool bands")
    check_pool_bytes(oracle, got, shape, bricks, midrange, cuts, table, ijk, grid, OUT_POISON, what)
    tgot, ok = tab.read()
    assert ok, (what, "table bands")
    assert np.array_equal(np.frombuffer(tgot.tobytes(), POOL_ENTRY), table), what
    return vector


# ---- test_offset_views_codec --------------------------------------------------------------------------------------------
def offsets_one_set(vr, oracle, shape, midrange):
    import torch
    x_run, tiled = SHAPES[shape]
    z, y, x = shape
    V = z * y * x
    general = not all(_pow2(v) for v in shape)
    bricks = (0, 2) if V >= (1 << 19) else (0, 1, 2)
    B = len(bricks)
    vols = set_volumes(oracle, shape, bricks, midrange)
    ref0 = ref_brick(oracle, shape, bricks[0], midrange)[1]
    D, M = ref0.origTreeDepth, ref0.maxTreeDepth
    variant = MIDRANGE if midrange else VOLUME_KDTREE
    # the GPU's own result from plainly allocated buffers: the second check
    plain = vr.BrickSet(B, (x, y, z), TOL, EP, variant).build(vols)
    check_built(oracle, plain, shape, bricks, midrange, "plain")
    aligned = {c: plain.decode(cut_depth=-1 if c is None else c).cpu().numpy() for c in the_cuts(D, M)}
    bs = vr.BrickSet(B, (x, y, z), TOL, EP, variant)
    bs.build(vols)              # the set holds trees before the first refused build
    for offset in range(1, 17):
        mis = offset % 16 != 0
        what = (shape, midrange, offset)
        # build: the input view and its bands are unchanged afterwards
        src = Window(B * V, offset, IN_POISON).fill(vols)
        before = src.base.cpu().numpy().copy()
        if x_run and mis:
            assert refused(vr, lambda: bs.build(src.view))
        else:
            bs.build(src.view)
        check_built(oracle, bs, shape, bricks, midrange, what)     # (after a refusal: the previous trees)
        torch.cuda.synchronize()
        assert np.array_equal(src.base.cpu().numpy(), before), (what, "build wrote to its input")
        # decode at every cut
        for c in the_cuts(D, M):
            for name, sw in SWITCHES.items():
                if sw and not (tiled and c is None):
                    continue        # the kernels behind the switches: the full decode of a tiled set
                if sw:
                    bs.set_switch(sw, 1)
                out = Window(B * V, offset, OUT_POISON)
                if tiled and mis:
                    assert refused(vr, lambda: bs.decode(out.view, cut_depth=-1 if c is None else c))
                    assert out.untouched(), (what, c, name, "refused decode wrote")
                else:
                    bs.decode(out.view, cut_depth=-1 if c is None else c)
                    got, ok = out.read()
                    assert ok, (what, c, name, "decode bands")
                    for b, i in enumerate(bricks):
                        assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, midrange, c)), (what, c, name, b)
                    assert np.array_equal(got, aligned[c]), (what, c, name)
                if sw:
                    bs.set_switch(sw, 0)
        if midrange:
            for c in (None, max(D - 3, 0)):
                out = Window(B * V, offset, OUT_POISON)
                if tiled and mis:
                    assert refused(vr, lambda: bs.decode_range(out.view, cut_depth=-1 if c is None else c))
                    assert out.untouched(), (what, c, "refused decode_range wrote")
                else:
                    bs.decode_range(out.view, cut_depth=-1 if c is None else c)
                    got, ok = out.read()
                    assert ok, (what, c, "decode_range bands")
                    for b, i in enumerate(bricks):
                        assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, True, c, True)), (what, c, b)
        # decode_lod, mixed cuts with a culled brick
        cuts = lod_plan(B, D, M, culled=1)
        out = Window(B * V, offset, OUT_POISON)
        if tiled and mis:
            assert refused(vr, lambda: bs.decode_lod(cuts, out=out.view))
            assert out.untouched(), (what, "refused decode_lod wrote")
        else:
            bs.decode_lod(cuts, out=out.view)
            got, ok = out.read()
            assert ok, (what, "decode_lod bands")
            check_lod_bytes(oracle, got, shape, bricks, midrange, cuts, OUT_POISON, what)
        out = Window(B * V, offset, OUT_POISON)     # every brick skipped: nothing is launched at any offset
        bs.decode_lod(np.full(B, -1, np.int32), out=out.view)
        torch.cuda.synchronize()
        assert out.untouched(), (what, "decode_lod of skipped bricks wrote")
        # decode_lod_pool, pool and table at offsets
        if general:
            out = Window(4096, offset, OUT_POISON)
            with pytest.raises(vr.VrError) as ei:
                bs.decode_lod_pool(np.zeros(B, np.int32), np.array([(b, 0, 0) for b in range(B)], np.int64), (B, 1, 1),
                                   pool=out.view, table=torch.zeros(B * 16, dtype=torch.uint8, device="cuda"))
            assert ei.value.status == VR_ERR_UNSUPPORTED and out.untouched(), what
        else:
            paths = {name: run_pool(vr, oracle, bs, shape, bricks, midrange, cuts, offset, tiled, what + (name,))
                     for name, cuts in pool_plans(B, D, M)}
            # what the header says of the three plans
            assert paths == {"full": tiled, "coarse": True, "one voxel": False}, (what, paths)
    # offset 16 came last: the aligned calls above followed fifteen rounds of refusals on the same handle


def offsets_error_helpers(vr):
    """vr_measure_error / vr_query_error: both inputs and the output at independent offsets, against NumPy."""
    from volumerenderer_amd import _lib
    import torch
    L = _lib.lib()
    rng = np.random.default_rng(99)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n in (1, 255, 257):
        a, b = rng.integers(0, 256, n, dtype=np.uint8), rng.integers(0, 256, n, dtype=np.uint8)
        a[0], b[0], a[-1], b[-1] = 0, 255, 255, 0          # the extremes at both ends
        err = np.abs(a.astype(np.int32) - b.astype(np.int32))
        for k in range(1, 17):
            oa, ob, oo = k, (5 * k + 3) % 16 or 16, (11 * k + 7) % 16 or 16
            wa, wb = Window(n, oa, IN_POISON).fill(a), Window(n, ob, IN_POISON).fill(b)
            wo = Window(n, oo, OUT_POISON)
            what = (n, oa, ob, oo)
            mx, mean = vr.measure_error(wa.view, wb.view)
            assert mx == int(err.max()) and abs(mean - float(err.sum()) / n) < 1e-12, what
            st = L.vr_query_error(C.c_void_p(wa.view.data_ptr()), C.c_void_p(wb.view.data_ptr()), n,
                                  C.c_void_p(wo.view.data_ptr()), stream)
            assert st == 0, what
            torch.cuda.synchronize()
            got, ok = wo.read()
            assert ok and np.array_equal(got, err.astype(np.uint8)), what
            for w, h in ((wa, a), (wb, b)):
                got, ok = w.read()
                assert ok and np.array_equal(got, h), (what, "an input changed")


@pytest.mark.parametrize("case", list(SHAPES) + ["error_helpers"], ids=lambda c: c if isinstance(c, str) else "%dx%dx%d" % c)
def test_offset_views_codec(vr, oracle, case):
    if case == "error_helpers":
        return offsets_error_helpers(vr)
    offsets_one_set(vr, oracle, case, midrange=False)
    offsets_one_set(vr, oracle, case, midrange=True)


# ---- test_guard_bands_aligned -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(SHAPES), ids=lambda s: "%dx%dx%d" % s)
def test_guard_bands_aligned(vr, oracle, shape):
    """MidRangeTree sets (they have every decode entry point), 1, 2 and 5 bricks, every buffer 256-byte aligned."""
    import torch
    _, tiled = SHAPES[shape]
    z, y, x = shape
    V = z * y * x
    general = not all(_pow2(v) for v in shape)
    for B in (1, 2, 5):
        bricks = tuple((0, 1, 2)[b % 3] for b in range(B))
        vols = set_volumes(oracle, shape, bricks, True)
        src = Window(B * V, 0, IN_POISON).fill(vols)
        before = src.base.cpu().numpy().copy()
        bs = vr.BrickSet(B, (x, y, z), TOL, EP, MIDRANGE).build(src.view)
        check_built(oracle, bs, shape, bricks, True, (shape, B))
        torch.cuda.synchronize()
        assert np.array_equal(src.base.cpu().numpy(), before), (shape, B, "build wrote to its input")
        info = bs.info(0)
        D, M = info["orig_tree_depth"], info["max_tree_depth"]
        for name, sw in SWITCHES.items():
            if sw and not tiled:
                continue
            if sw:
                bs.set_switch(sw, 1)
            what = (shape, B, name)
            for c in the_cuts(D, M):
                out = Window(B * V, 0, OUT_POISON)
                bs.decode(out.view, cut_depth=-1 if c is None else c)
                got, ok = out.read()
                assert ok, (what, c, "decode wrote outside its bricks")
                for b, i in enumerate(bricks):
                    assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, True, c)), (what, c, b)
            for culled in sorted({0, B - 1}):       # the first brick culled, the last brick culled
                cuts = lod_plan(B, D, M, culled)
                out = Window(B * V, 0, OUT_POISON)
                bs.decode_lod(cuts, out=out.view)
                got, ok = out.read()
                assert ok, (what, culled, "decode_lod wrote outside its bricks")
                check_lod_bytes(oracle, got, shape, bricks, True, cuts, OUT_POISON, what)
            if not general:
                for pname, cuts in pool_plans(B, D, M):
                    run_pool(vr, oracle, bs, shape, bricks, True, cuts, 0, tiled, what + (pname,))
            if sw:
                bs.set_switch(sw, 0)
        for c in (None, D, max(D - 3, 0)):
            out = Window(B * V, 0, OUT_POISON)
            bs.decode_range(out.view, cut_depth=-1 if c is None else c)
            got, ok = out.read()
            assert ok, (shape, B, c, "decode_range wrote outside its bricks")
            for b, i in enumerate(bricks):
                assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, True, c, True)), (shape, B, c, b)
        n = min(B * V, 1000)
        wo = Window(B * V, 0, OUT_POISON)
        from volumerenderer_amd import _lib
        st = _lib.lib().vr_query_error(C.c_void_p(src.view.data_ptr()), C.c_void_p(src.view.data_ptr() + (B * V - n)), n,
                                       C.c_void_p(wo.view.data_ptr()), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert st == 0
        torch.cuda.synchronize()
        got, ok = wo.read()
        flat = vols.reshape(-1).astype(np.int32)
        assert ok and np.array_equal(got[:n], np.abs(flat[:n] - flat[B * V - n:]).astype(np.uint8))
        assert np.all(got[n:] == OUT_POISON), "vr_query_error wrote more than n bytes"


# ---- test_batched_odd_sized_bricks --------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(5, 9, 7), (3, 1, 1), (7, 9, 2)], ids=lambda s: "%dx%dx%d" % s)
def test_batched_odd_sized_bricks(vr, oracle, shape):
    """General extents with a voxel count that is no multiple of 16 (315, 3, 126): brick b of a set starts at byte b * V,
    misaligned inside the set's own buffers.  Every brick must equal its single-brick oracle."""
    z, y, x = shape
    V = z * y * x
    for midrange in (False, True):
        for B in (2, 3, 7):
            bricks = tuple((3, 1, 2, 7, 5, 0, 11)[b] for b in range(B))       # noise, rm_like, constant, noise ...
            vols = set_volumes(oracle, shape, bricks, midrange)
            bs = vr.BrickSet(B, (x, y, z), TOL, EP, MIDRANGE if midrange else VOLUME_KDTREE).build(vols)
            what = (shape, midrange, B)
            check_built(oracle, bs, shape, bricks, midrange, what)
            info = bs.info(0)
            D, M = info["orig_tree_depth"], info["max_tree_depth"]
            for c in (None, max(D - 1, 0), D // 2):
                out = Window(B * V, 0, OUT_POISON)
                bs.decode(out.view, cut_depth=-1 if c is None else c)
                got, ok = out.read()
                assert ok, (what, c, "decode bands")
                for b, i in enumerate(bricks):
                    assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, midrange, c)), (what, c, b)
                if midrange:
                    out = Window(B * V, 0, OUT_POISON)
                    bs.decode_range(out.view, cut_depth=-1 if c is None else c)
                    got, ok = out.read()
                    assert ok, (what, c, "decode_range bands")
                    for b, i in enumerate(bricks):
                        assert np.array_equal(got[b * V:(b + 1) * V], want(oracle, shape, i, True, c, True)), (what, c, b)
            for culled in range(B):
                cuts = lod_plan(B, D, M, culled)
                out = Window(B * V, 0, OUT_POISON)
                bs.decode_lod(cuts, out=out.view)
                got, ok = out.read()
                assert ok, (what, culled, "decode_lod bands")
                check_lod_bytes(oracle, got, shape, bricks, midrange, cuts, OUT_POISON, what)
