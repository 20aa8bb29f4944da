"""Many-brick sets on the GPU: the batch axis past 64, past 1024 and at VR_MAX_BRICKS.

Every comparison is bit for bit against the oracle's results for the 37 contents of tests/manybricks.py, tiled over the
set (brick b holds content (b + rot) % 37, so no brick equals a neighbour at distance 1, 16, 32, 64 or 1024).  What
depends on B and is reached here: k_brick_offsets' scan rounds and carry (every compact stream of brick >= 1024), the
level loop's split into brick ranges at its thresholds, the three B-sized regions of a per-brick decode's lists and the
staged passes of the pool decode, the one-workgroup-per-brick kernels, the per-brick reductions, the archives, and
vr_assemble_bricks / vr_disassemble_bricks, which no test checked directly."""
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import manybricks as MB  # noqa: E402

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FILL = 0xA5
GRID = (41, 5, 5)              # 1025 cells


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def expect(oracle):
    """expect(dims, tolerance, epochs, midrange): the oracle's results for the 37 contents, made once."""
    made = {}

    def get(dims, tolerance=1, max_epochs=2, midrange=False):
        key = (tuple(dims), tolerance, max_epochs, midrange)
        if key not in made:
            made[key] = MB.Expect(oracle, dims, tolerance, max_epochs, midrange)
        return made[key]
    return get


@pytest.fixture(scope="module")
def built(vr, expect):
    """built(dims, B, midrange): a set of B bricks built once with the defaults (contents not rotated), and its Expect."""
    sets = {}

    def get(dims, B, midrange=False):
        key = (tuple(dims), B, midrange)
        if key not in sets:
            e = expect(dims, 1, 2, midrange)
            bs = vr.BrickSet(B, dims, 1, 2, vr.VARIANT_MIDRANGE if midrange else vr.VARIANT_RECOVER)
            bs.build(MB.voxels(dims, B))
            sets[key] = (bs, e)
        return sets[key]
    yield get
    sets.clear()


def check_bricks(bs, e, B, rot=0, bricks=None, what=None):
    """info(b)["num_active_nodes"], tree(b) and distance_map(b) (MidRangeTree: both streams) of every brick, or of `bricks`."""
    who = MB.content_of(B, rot)
    for b in (range(B) if bricks is None else bricks):
        i = int(who[b])
        assert bs.info(b)["num_active_nodes"] == e.num_active[i], (what, "numActiveNodes", b)
        assert np.array_equal(bs.tree(b), e.tree[i]), (what, "tree", b)
        assert np.array_equal(bs.distance_map(b), e.dmap[i]), (what, "distance map", b)
        if e.midrange:
            assert np.array_equal(bs.tree_range(b), e.tree_range[i]), (what, "range tree", b)
            assert np.array_equal(bs.distance_map_range(b), e.dmap_range[i]), (what, "range distance map", b)


def first_bad(got, want):
    """None, or the first brick whose bytes differ (both (B, V))."""
    bad = np.flatnonzero(np.any(got != want, axis=1))
    return None if bad.size == 0 else int(bad[0])


def check_decode(bs, e, B, rot=0, cut=-1, what=None):
    got = bs.decode(cut_depth=cut).cpu().numpy().reshape(B, -1)
    assert first_bad(got, e.decode(B, cut, rot)) is None, (what, "decode", cut, first_bad(got, e.decode(B, cut, rot)))


def configs(B):
    """(compaction on build, level-loop streams): both compactions at every concurrency that gives a part 16 bricks."""
    return [(on_build, c) for on_build in (True, False) for c in MB.CONCURRENCY if c == 1 or B >= 16 * c]


def run_builds(vr, e, B):
    """One handle, one build per configuration, the contents rotated by one each time (so no build can pass on what the
    one before left behind): every brick's bytes and the full decode."""
    variant = vr.VARIANT_MIDRANGE if e.midrange else vr.VARIANT_RECOVER
    bs = vr.BrickSet(B, e.dims, e.tolerance, e.max_epochs, variant)
    for rot, (on_build, conc) in enumerate(configs(B)):
        what = (e.dims, B, "compact on build" if on_build else "compact lazily", "streams %d" % conc)
        bs.set_compaction(on_build)
        bs.set_concurrency(conc)
        bs.build(MB.voxels(e.dims, B, rot))
        if on_build:
            check_bricks(bs, e, B, rot, what=what)
            check_decode(bs, e, B, rot, what=what)
        else:                   # the decode first: it reads the gapped streams, the lazy copy has not been made yet
            check_decode(bs, e, B, rot, what=what)
            check_bricks(bs, e, B, rot, what=what)
    return bs


# ---- build -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", sorted(MB.FUSED_B))
def test_build_16cubed(vr, expect, B):
    run_builds(vr, expect(MB.FUSED), B)


@pytest.mark.parametrize("B", MB.OTHER_B)
@pytest.mark.parametrize("dims", [MB.UNFUSED, MB.GENERAL], ids=["8x8x8", "12x6x5"])
def test_build_unfused_and_general(vr, expect, dims, B):
    run_builds(vr, expect(dims), B)


@pytest.mark.parametrize("B", MB.MIDRANGE_B)
def test_build_midrange_both_streams(vr, expect, B):
    run_builds(vr, expect(MB.FUSED, 1, 2, True), B)


def test_build_with_prunes_and_reverts(vr, expect):
    """Tolerance 6, five epochs: the level loop prunes and reverts, per brick, in every range of the split."""
    e = expect(MB.FUSED, 6, 5)
    assert any(t.numReverts > 0 for t in e.trees)
    bs = run_builds(vr, e, 1025)
    rot = len(configs(1025)) - 1
    who = MB.content_of(1025, rot)
    for b in (0, 31, 32, 63, 64, 512, 1023, 1024):
        assert bs.info(b)["num_reverts"] == e.trees[int(who[b])].numReverts, b


def test_rebuild_a_b_a_on_one_handle(vr, expect):
    """A, then the contents rotated, then A again: every brick of every build, compact offsets that move each time."""
    e, B = expect(MB.FUSED), 1025
    bs = vr.BrickSet(B, MB.FUSED, 1, 2)
    for rot in (0, 5, 0):
        bs.build(MB.voxels(MB.FUSED, B, rot))
        check_bricks(bs, e, B, rot, what=("rebuild", rot))
        check_decode(bs, e, B, rot, what=("rebuild", rot))


# ---- decode ----------------------------------------------------------------------------------------------------------
DECODE_SETS = [(MB.FUSED, B, False) for B in (1, 33, 65, 1025, 3000)] + \
    [(d, B, False) for d in (MB.UNFUSED, MB.GENERAL) for B in MB.OTHER_B] + [(MB.FUSED, B, True) for B in MB.MIDRANGE_B]


def _set_id(s):
    return "%dx%dx%d-%d%s" % (s[0] + (s[1], "-mid" if s[2] else ""))


@pytest.mark.parametrize("case", DECODE_SETS, ids=_set_id)
def test_uniform_decode_at_every_level_class(built, case):
    """decode() at full depth and at cuts 0, Ds - 1, Ds and D: all voxels of all bricks."""
    dims, B, midrange = case
    bs, e = built(dims, B, midrange)
    for c in [-1] + MB.uniform_cuts(dims):
        check_decode(bs, e, B, cut=c, what=case)
    if midrange:
        for c in [-1] + MB.uniform_cuts(dims):
            got = bs.decode_range(cut_depth=c).cpu().numpy().reshape(B, -1)
            assert first_bad(got, e.decode_range(B, c)) is None, (case, "range", c)


@pytest.mark.parametrize("case", DECODE_SETS, ids=_set_id)
def test_decode_lod_lists(built, case):
    """A cut per brick that cycles through every class, -1 included: the cuts, the "above the index level" list and the
    class lists each hold every tenth brick or so.  Skipped bricks keep the sentinel written beforehand."""
    import torch
    dims, B, midrange = case
    bs, e = built(dims, B, midrange)
    for rot in (0, 1, 4):
        cuts = MB.cut_pattern(dims, B, rot)
        out = torch.full((B * bs.voxels_per_brick,), FILL, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=out)
        got = out.cpu().numpy().reshape(B, -1)
        want = e.decode_lod(B, cuts, FILL)
        bad = first_bad(got, want)
        assert bad is None, (case, rot, bad, int(cuts[bad]))


def np_assemble(bricks, dims, ijk, grid, fill=0):
    """[gz*Z][gy*Y][gx*X]: brick b (flat, x fastest) at cell ijk[b]; cells without a brick hold `fill`."""
    X, Y, Z = dims
    vol = np.full((grid[2] * Z, grid[1] * Y, grid[0] * X), fill, np.uint8)
    for b, (i, j, k) in enumerate(ijk):
        vol[k * Z:(k + 1) * Z, j * Y:(j + 1) * Y, i * X:(i + 1) * X] = np.asarray(bricks[b]).reshape(Z, Y, X)
    return vol


def grid_map(seed, grid=GRID):
    """Every cell of the grid once, in a seeded random order: (cells, 3) int64."""
    cells = np.array([(i, j, k) for k in range(grid[2]) for j in range(grid[1]) for i in range(grid[0])], np.int64)
    return cells[np.random.default_rng(seed).permutation(len(cells))]


def test_decode_lod_pool_many_staged_passes(vr, built):
    """1025 bricks into a pool: six of every ten bricks coarse (617: nineteen staged passes of VR_POOL_STAGE_BRICKS and a
    ragged one of 9), three at full resolution, one skipped.  The table is the header's layout rule restated, the pool
    read through tests/refpool.py equals the oracle's per-brick cuts, bytes outside the slots keep a sentinel."""
    import torch
    import refpool
    from volumerenderer_amd.render import POOL_ENTRY
    B = 1025
    bs, e = built(MB.FUSED, B)
    ijk = grid_map(11)
    cuts = MB.cut_pattern(MB.FUSED, B, 2)
    shifts = [refpool.kd_shifts(MB.FUSED, c) if c >= 0 else (0, 0, 0) for c in cuts]
    coarse = sum(1 for c, s in zip(cuts, shifts) if c >= 0 and any(s))
    full = sum(1 for c, s in zip(cuts, shifts) if c >= 0 and not any(s))
    assert coarse == 617 and coarse > 32 * 3 and coarse % 32 == 9 and full >= 100 and int(np.sum(cuts < 0)) >= 100
    # the layout rule of vrhip.h, restated
    want_table = np.zeros(B, POOL_ENTRY)
    want_table["offset"] = -1
    total = 0
    slots = []
    for b in range(B):
        if cuts[b] < 0:
            continue
        n = 4096 >> sum(shifts[b])
        total = (total + 255) // 256 * 256
        cell = int(ijk[b][0] + GRID[0] * (ijk[b][1] + GRID[1] * ijk[b][2]))
        want_table[cell]["offset"], want_table[cell]["shift"] = total, shifts[b]
        slots.append((total, n))
        total += n
    layout, need = vr.lod_pool_layout(MB.FUSED, ijk, GRID, cuts, e.D, e.M)
    assert need == total and np.array_equal(layout, want_table)
    pool = torch.full((need + 256,), FILL, dtype=torch.uint8, device="cuda")
    table = torch.zeros(B * POOL_ENTRY.itemsize, dtype=torch.uint8, device="cuda")
    bs.decode_lod_pool(cuts, ijk, GRID, pool=pool, table=table)
    host, got_table = pool.cpu().numpy(), table.cpu().numpy().view(POOL_ENTRY)
    assert np.array_equal(got_table, want_table)
    outside = np.ones(host.size, bool)
    for off, n in slots:
        outside[off:off + n] = False
    assert np.all(host[outside] == FILL), "pool bytes outside the slots were written"
    got = refpool.expand(host, got_table, MB.FUSED, GRID)
    want = np_assemble(e.decode_lod(B, cuts, 0), MB.FUSED, ijk, GRID)
    assert np.array_equal(got, want)


# ---- per-brick reductions ----------------------------------------------------------------------------------------
def test_error_table_1025_bricks(built):
    """Every cut's row against the original voxels: the oracle's decode at that cut, then NumPy (table_py)."""
    from test_error_table_cpu import table_py
    B = 1025
    bs, e = built(MB.FUSED, B)
    vox = MB.voxels(MB.FUSED, B)
    got = bs.error_table(reference=vox)
    assert got.shape == (e.M + 1, B)
    per_content = table_py([e.cut(c) for c in range(e.M + 1)], MB.contents(MB.FUSED)[1].reshape(MB.PERIOD, -1))
    want = per_content[:, MB.content_of(B)]
    assert np.array_equal(got, want), np.argwhere(got != want)[:4]
    own = bs.error_table(cuts=(e.M, e.M))                        # against the set's own full decode: all zero
    assert not any(own[f].any() for f in ("sum_abs", "sum_sq", "max_abs", "num_diff"))


def test_measure_error_and_histogram_1025_bricks(vr, built):
    import torch
    B = 1025
    bs, e = built(MB.FUSED, B)
    vox = MB.voxels(MB.FUSED, B)
    dec = bs.decode(cut_depth=9)
    want_dec = e.decode(B, 9)
    assert np.array_equal(dec.cpu().numpy().reshape(B, -1), want_dec)
    got = vr.measure_error_bricks(dec, torch.from_numpy(vox.reshape(-1)).cuda(), B)
    d = np.abs(want_dec.astype(np.int64) - vox.astype(np.int64))
    assert np.array_equal(got["sum_abs"], d.sum(1)) and np.array_equal(got["sum_sq"], (d * d).sum(1))
    assert np.array_equal(got["max_abs"], d.max(1)) and np.array_equal(got["num_diff"], (d != 0).sum(1))
    for data in (vox, want_dec):
        bricks, total = vr.histogram_bricks(np.ascontiguousarray(data).reshape(-1), B)
        want = np.stack([np.bincount(row, minlength=256) for row in data])
        assert np.array_equal(bricks, want)
        assert np.array_equal(total, want.sum(0).astype(np.uint64))


# ---- archives and installs -------------------------------------------------------------------------------------------
def test_archive_round_trips_1025_bricks(vr, built, tmp_path):
    """save_set -> open_set, load_set into a second handle, and set_trees of the oracle's own 1025 streams into a fresh
    one: every brick's bytes and the full decode, each time."""
    B = 1025
    bs, e = built(MB.FUSED, B)
    p = str(tmp_path / "set.vrbset")
    bs.save_set(p)
    opened = vr.BrickSet.open_set(p)
    assert opened.num_bricks == B
    check_bricks(opened, e, B, what="open_set")
    check_decode(opened, e, B, what="open_set")
    second = vr.BrickSet(B, MB.FUSED, 1, 2)
    second.load_set(p)
    check_bricks(second, e, B, what="load_set")
    check_decode(second, e, B, what="load_set")
    # the oracle's streams, rotated so that the installed set is not the one the file holds
    rot = 3
    who = MB.content_of(B, rot)
    tables = [vr.stream_block_table(MB.FUSED, e.tree[i], int(e.num_active[i]), e.dmap[i]) for i in range(MB.PERIOD)]
    fresh = vr.BrickSet(B, MB.FUSED, 1, 2)
    order = np.random.default_rng(5).permutation(B)
    fresh.set_trees(order, [e.tree[who[b]] for b in order], [int(e.num_active[who[b]]) for b in order],
                    [e.dmap[who[b]] for b in order], [tables[who[b]] for b in order])
    check_bricks(fresh, e, B, rot, what="set_trees")
    check_decode(fresh, e, B, rot, what="set_trees")
    for c in (0, 5, 12):
        check_decode(fresh, e, B, rot, cut=c, what="set_trees")


# ---- vr_assemble_bricks / vr_disassemble_bricks ----------------------------------------------------------------------
def offset_view(n, off, fill=FILL):
    """(whole buffer, view of n bytes that starts `off` bytes past a 16-byte boundary), the buffer full of `fill`."""
    import torch
    buf = torch.full((n + 32,), fill, dtype=torch.uint8, device="cuda")
    assert buf.data_ptr() % 16 == 0
    view = buf[off:off + n]
    assert view.data_ptr() % 16 == off % 16
    return buf, view


def check_assemble(vr, dims, grid, ijk, seed, src_off=0, dst_off=0):
    """Both directions against NumPy for nb = len(ijk) bricks; cells and bytes that are not named keep the sentinel."""
    import torch
    nb, V = len(ijk), dims[0] * dims[1] * dims[2]
    cells = grid[0] * grid[1] * grid[2]
    rng = np.random.default_rng(seed)
    bricks = rng.integers(0, 256, (nb, V), dtype=np.uint8)
    bricks[bricks == FILL] = 0                                       # (so that the sentinel is no brick's value)
    sbuf, src = offset_view(nb * V, src_off)
    src.copy_(torch.from_numpy(bricks.reshape(-1)))
    dbuf, dst = offset_view(cells * V, dst_off)
    vr.assemble_bricks(src, dims, ijk, grid, out=dst)
    torch.cuda.synchronize()
    want = np_assemble(bricks, dims, ijk, grid, FILL)
    whole = dbuf.cpu().numpy()
    assert np.array_equal(whole[dst_off:dst_off + cells * V].reshape(want.shape), want), (dims, grid, nb, src_off, dst_off)
    assert np.all(whole[:dst_off] == FILL) and np.all(whole[dst_off + cells * V:] == FILL)
    # and back, from the volume just checked
    bbuf, back = offset_view(nb * V, src_off)
    vr.disassemble_bricks(dst, dims, ijk, grid, out=back)
    torch.cuda.synchronize()
    whole = bbuf.cpu().numpy()
    assert np.array_equal(whole[src_off:src_off + nb * V].reshape(nb, V), bricks), (dims, grid, nb, src_off, dst_off)
    assert np.all(whole[:src_off] == FILL) and np.all(whole[src_off + nb * V:] == FILL)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1), (0, 1), (1, 0)], ids=["aligned", "both+1", "dst+1", "src+1"])
def test_assemble_1025_bricks_permuted_map(vr, offsets):
    """1025 bricks of 16^3 on a 41 x 5 x 5 grid in a permuted order; through 1-byte-offset views the byte-copy kernels."""
    check_assemble(vr, MB.FUSED, GRID, grid_map(21), 1, *offsets)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1)], ids=["aligned", "both+1"])
def test_assemble_partial_map_keeps_the_other_cells(vr, offsets):
    check_assemble(vr, MB.FUSED, GRID, grid_map(22)[:700], 2, *offsets)


@pytest.mark.parametrize("offsets", [(0, 0), (1, 1)], ids=["aligned", "both+1"])
def test_assemble_rows_of_48(vr, offsets):
    """A first extent that is a multiple of 16 and no power of two: three vectors per row."""
    check_assemble(vr, (48, 2, 3), (3, 4, 5), grid_map(23, (3, 4, 5)), 3, *offsets)
    check_assemble(vr, (48, 2, 3), (3, 4, 5), grid_map(24, (3, 4, 5))[:31], 4, *offsets)


def test_assemble_refuses_bad_extents_and_cells(vr):
    import torch
    src = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), FILL, dtype=torch.uint8, device="cuda")
    for fn in (vr.assemble_bricks, vr.disassemble_bricks):
        for bd in ((8, 4, 4), (24, 2, 2), (17, 1, 1)):
            with pytest.raises(vr.VrError) as err:
                fn(src, bd, [(0, 0, 0)], (1, 1, 1), out=dst)
            assert err.value.status == -7, bd                              # VR_ERR_UNSUPPORTED
        for cell in ((2, 0, 0), (0, 2, 0), (0, 0, 1), (-1, 0, 0), (0, 0, -1)):
            with pytest.raises(vr.VrError) as err:
                fn(src, (16, 2, 2), [(0, 0, 0), cell], (2, 2, 1), out=dst)
            assert err.value.status == -1, cell                            # VR_ERR_INVALID
    torch.cuda.synchronize()
    assert bool((dst == FILL).all())                                       # nothing was launched


def seventy_maps():
    """70 distinct brick maps in one process: the first 64 are cached on the device for the life of the process, the
    others take the branch that uploads its own copy and frees it.  Each call is checked both ways.  Run as a child
    process, so that the process-wide cache of the test session is left as it was."""
    import torch
    sys.path.insert(0, ROOT)
    import volumerenderer_amd as vr
    dims, grid = (16, 2, 2), (4, 2, 2)
    V, cells = 64, 16
    rng = np.random.default_rng(70)
    seen = set()
    for m in range(70):
        nb = 2 + m % (cells - 1)
        ijk, draw = grid_map(1000 + m, grid)[:nb], 0
        while ijk.tobytes() in seen:                     # (two short maps may come out alike: draw again)
            draw += 1
            ijk = grid_map(2000 + 100 * m + draw, grid)[:nb]
        seen.add(ijk.tobytes())
        bricks = rng.integers(0, 250, (nb, V), dtype=np.uint8)
        out = torch.full((cells * V,), 255, dtype=torch.uint8, device="cuda")
        vr.assemble_bricks(bricks.reshape(-1), dims, ijk, grid, out=out)
        want = np_assemble(bricks, dims, ijk, grid, 255)
        assert np.array_equal(out.cpu().numpy().reshape(want.shape), want), m
        back = vr.disassemble_bricks(out, dims, ijk, grid)
        assert np.array_equal(back.cpu().numpy().reshape(nb, V), bricks), m
    assert len(seen) == 70
    print("70 maps ok")


def test_assemble_seventy_distinct_maps(vr):
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "seventy_maps"], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0 and "70 maps ok" in r.stdout, r.stdout + r.stderr


# ---- the limit ---------------------------------------------------------------------------------------------------------
def test_a_set_of_vr_max_bricks(vr, expect):
    """VR_MAX_BRICKS bricks of 2 x 2 x 2: the last brick count every launch accepts.  The whole decode, and the bytes of
    about 200 bricks: every multiple of 1024 with its two neighbours, and the last."""
    import re
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    B = int(re.search(r"#define\s+VR_MAX_BRICKS\s+(\d+)", hdr).group(1))
    assert B == 65535
    with pytest.raises(vr.VrError) as err:
        vr.BrickSet(B + 1, MB.TINY, 1, 2)
    assert err.value.status == -7
    e = expect(MB.TINY)
    bs = vr.BrickSet(B, MB.TINY, 1, 2)
    bs.build(MB.voxels(MB.TINY, B))
    check_decode(bs, e, B, what="limit")
    check_decode(bs, e, B, cut=1, what="limit")
    sample = sorted({b for k in range(0, B + 1, 1024) for b in (k - 1, k, k + 1) if 0 <= b < B} | {B - 1})
    assert 180 <= len(sample) <= 220
    check_bricks(bs, e, B, bricks=sample, what="limit")


if __name__ == "__main__":
    if sys.argv[1:] == ["seventy_maps"]:
        seventy_maps()
