"""The general-extent decode (k_geom_owner, k_decode_lane<true>, k_owner_gather) on grammar-random
foreign streams: any extent that is not a power of two, or longer than 1024, through vr_brickset_set_tree,
vr_brickset_open, vr_brickset_set_trees (the GPU index and k_cut_from_top) and the archive calls.  Streams and
references come from tests/refstream.py (make_general; tests/test_stream_grammar_general_cpu.py pins them to the oracle
and asserts what the streams contain: voxels a branch halving dropped, branches of every length, pruned boxes of
several cells).  Everything is bit-exact against the reference: no tolerance, no masked voxel."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402
import test_gpu_foreign_streams as F  # noqa: E402  (helpers only: main_cuts, check_switches, decode, install)

pytestmark = pytest.mark.gpu

VR_ERR_FORMAT, VR_ERR_UNSUPPORTED = -6, -7
POISON = 0xA5
DEAD = 0xFFFFFFFF
SMALL = [(3, 1, 1), (5, 3, 2), (7, 9, 2), (12, 6, 5), (24, 10, 6)]      # D = 1, 4 (K < 6), 6, 7, 9: one index block
LARGE = [(40, 16, 24), (2048, 2, 2), (96, 64, 48)]                      # D = 13, 13, 17: 2, 2 and 32 blocks of 4096 leaves
BIG = ("dense7", "blockprune", "mixed", "leafprune")
LAWS = ("std", "sat", "chain_ns")
EVERY_CUT = [(12, 6, 5), (7, 9, 2)]


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def families_at(dims):
    return BIG if dims in LARGE else R.FAMILIES


def all_cuts(M):
    return [None] + list(range(M, -1, -1))


def table_of(lv):
    from volumerenderer_amd.codec import stream_block_table
    return stream_block_table(lv.dims, R.pack(lv.tokens), lv.tokens.size, lv.dmap)


def install_many(vr, lvs, bricks=None, bs=None, num_bricks=None, tables=True):
    """lvs installed as `bricks` (default 0 .. len - 1) in one vr_brickset_set_trees call."""
    bricks = list(range(len(lvs))) if bricks is None else list(bricks)
    if bs is None:
        bs = vr.BrickSet(num_bricks or len(lvs), lvs[0].dims)
    bs.set_trees(bricks, [R.pack(lv.tokens) for lv in lvs], [lv.tokens.size for lv in lvs], [lv.dmap for lv in lvs],
                 tables=[table_of(lv) for lv in lvs] if tables else None)
    return bs


def lod(bs, cuts):
    import torch
    X, Y, Z = bs.dims
    out = torch.full((bs.num_bricks * X * Y * Z,), POISON, dtype=torch.uint8, device="cuda")
    bs.decode_lod(np.array(cuts, np.int32), out=out)
    return out.cpu().numpy().reshape(bs.num_bricks, Z, Y, X)


def test_depths_are_the_expected_ones(vr):
    for dims, D in zip(SMALL + LARGE, (1, 4, 6, 7, 9, 13, 13, 17)):
        lv = R.make_general(dims, "root3", "std")
        assert lv.D == D and F.install(vr, lv).info(0)["orig_tree_depth"] == D


# ---- a. per family ----

@pytest.mark.parametrize("dims", SMALL + LARGE, ids=F._ids)
def test_families(vr, dims):
    for family in families_at(dims):
        for law in LAWS:
            lv = R.make_general(dims, family, law)
            cuts = all_cuts(lv.M) if dims in EVERY_CUT else F.main_cuts(lv.D, lv.M)
            F.check_switches(F.install(vr, lv), [R.decode_levels(lv)], cuts, (family, law))


# ---- b. the GPU index: vr_brickset_set_trees, cuts above the index depth from the heap the kernel wrote ----

@pytest.mark.parametrize("tables", [True, False], ids=["tables", "no_tables"])
@pytest.mark.parametrize("dims", [(12, 6, 5)] + LARGE, ids=F._ids)
def test_gpu_index(vr, dims, tables):
    fams = [(f, law) for f in families_at(dims) for law in LAWS]          # three bricks a set: one law each
    for group in (fams[i:i + 3] for i in range(0, len(fams), 3)):
        lvs = [R.make_general(dims, f, law) for f, law in group]
        D, M = lvs[0].D, lvs[0].M
        Ds = D - min(D, 6)
        gpu = install_many(vr, lvs, tables=tables)
        host = vr.BrickSet(len(lvs), dims)
        for b, lv in enumerate(lvs):
            F.install(vr, lv, brick=b, bs=host)
        for b, lv in enumerate(lvs):
            assert gpu.info(b) == host.info(b), group[b]
            assert np.array_equal(gpu.tree(b), R.pack(lv.tokens)) and np.array_equal(gpu.distance_map(b), lv.dmap), group[b]
        cuts = all_cuts(M) if dims == (12, 6, 5) else F.main_cuts(D, M) + F.cut_list(D, M, [Ds, Ds - 1, Ds - 2, 1])
        assert any(c is not None and c < Ds for c in cuts) and any(c is not None and c >= Ds for c in cuts)
        decs = [R.decode_levels(lv) for lv in lvs]
        for c in cuts:
            got = F.decode(gpu, c)
            assert got.tobytes() == F.decode(host, c).tobytes(), (group, c)
            assert np.array_equal(got, np.stack([d.at(c) for d in decs])), (group, c)
        F.check_switches(gpu, decs, [None, D, Ds - 1 if Ds > 0 else 0], group)


# ---- c. sets: re-installs that leave nothing behind, per-brick cuts, the pool's refusal ----

@pytest.mark.parametrize("how", ["set_tree", "set_trees"])
def test_reinstall_leaves_nothing_stale(vr, how):
    dims = LARGE[0]

    def put(bs, brick, lv):
        if how == "set_tree":
            F.install(vr, lv, brick=brick, bs=bs)
        else:
            install_many(vr, [lv], bricks=[brick], bs=bs)

    lvs = [R.make_general(dims, "mixed", "std"), R.make_general(dims, "dense7", "chain_ns"), R.make_general(dims, "leafprune", "sat")]
    M = lvs[0].M
    bs = vr.BrickSet(3, dims)
    for b, lv in enumerate(lvs):
        put(bs, b, lv)
    F.check_switches(bs, [R.decode_levels(lv) for lv in lvs], F.main_cuts(lvs[0].D, M), "first")
    # brick 1 with a stream at most a quarter as long, then brick 1 and brick 2 with longer ones
    short = R.make_general(dims, "blockprune", "std")
    assert short.tokens.size * 4 <= lvs[1].tokens.size
    for brick, lv in ((1, short), (1, R.make_general(dims, "dense7", "sat")), (2, R.make_general(dims, "dense7", "std"))):
        assert lv is short or lv.tokens.size > lvs[brick].tokens.size
        lvs[brick] = lv
        put(bs, brick, lv)
        assert bs.info(brick)["num_active_nodes"] == lv.tokens.size and np.array_equal(bs.tree(brick), R.pack(lv.tokens))
        decs = [R.decode_levels(v) for v in lvs]
        for c in all_cuts(M):
            assert np.array_equal(F.decode(bs, c), np.stack([d.at(c) for d in decs])), (brick, c)
    F.check_switches(bs, decs, [None, lvs[0].D, 3], "last")


@pytest.mark.parametrize("how", ["set_tree", "set_trees"])
def test_per_brick_cuts_with_a_brick_never_installed(vr, how):
    import torch
    dims = LARGE[0]
    X, Y, Z = dims
    lvs = {0: R.make_general(dims, "mixed", "sat"), 1: R.make_general(dims, "dense7", "chain_ns"), 3: R.make_general(dims, "leafprune", "std")}
    bs = vr.BrickSet(4, dims)
    if how == "set_tree":
        for b, lv in lvs.items():
            F.install(vr, lv, brick=b, bs=bs)
    else:
        install_many(vr, list(lvs.values()), bricks=list(lvs), bs=bs)
    assert bs.info(2)["num_active_nodes"] == 0
    decs = {b: R.decode_levels(lv) for b, lv in lvs.items()}
    D, M = lvs[0].D, lvs[0].M
    Ds = D - 6
    menu = [-1, 0, Ds - 1, Ds, D - 3, D, D + 2, M]
    plans = [[menu[(r + 3 * b) % len(menu)] for b in range(4)] for r in range(len(menu))] + [[M, M, -1, M], [-1, -1, -1, -1]]
    for cuts in plans:
        cuts[2] = -1
        got = lod(bs, cuts)
        for b, c in enumerate(cuts):
            if c < 0:
                assert np.all(got[b] == POISON), (cuts, b)
            else:
                assert np.array_equal(got[b], decs[b].at(c)), (cuts, b)
    # the pool decode serves power-of-two extents only: refused, nothing written, and the set decodes as before
    pool = torch.full((1 << 20,), POISON, dtype=torch.uint8, device="cuda")
    table = torch.full((4 * 16,), 0x5A, dtype=torch.uint8, device="cuda")
    with pytest.raises(vr.VrError) as e:
        bs.decode_lod_pool(np.array([M, D, -1, 3], np.int32), np.array([(b, 0, 0) for b in range(4)], np.int64), (4, 1, 1),
                           pool=pool, table=table)
    assert e.value.status == VR_ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert torch.all(pool == POISON) and torch.all(table == 0x5A)
    got = lod(bs, [M, D - 3, -1, 0])
    assert np.array_equal(got[0], decs[0].at(M)) and np.array_equal(got[1], decs[1].at(D - 3)) and np.array_equal(got[3], decs[3].at(0))
    assert np.all(got[2] == POISON)


# ---- d. 64-bit token offsets ----

@pytest.mark.parametrize("dims", [(12, 6, 5), (40, 16, 24)], ids=F._ids)
def test_foreign_streams_with_64_bit_offsets(vr, monkeypatch, dims):
    """VRHIP_FORCE_IDX64 (read when the set is created; it takes hold from depth 12 on) takes the set through the
    block-relative index and the zeroed bases that set_tree writes for an installed stream."""
    for family, law in (("dense7", "std"), ("blockprune", "sat"), ("mixed", "chain_ns"), ("leafprune", "std")):
        lv = R.make_general(dims, family, law)
        monkeypatch.setenv("VRHIP_FORCE_IDX64", "1")
        bs = F.install(vr, lv)
        monkeypatch.delenv("VRHIP_FORCE_IDX64")
        dec = R.decode_levels(lv)
        D = lv.D
        cuts = [None, D, D - 3, 0]
        first = {c: F.decode(bs, c) for c in cuts}
        for c in cuts:
            assert np.array_equal(first[c][0], dec.at(c)), (family, "default", c)
        bs.set_switch("decode_walk", 1)
        for c in cuts:
            assert np.array_equal(F.decode(bs, c)[0], dec.at(c)), (family, "decode_walk", c)
        bs.set_switch("decode_walk", 0)
        for c in cuts:
            assert F.decode(bs, c).tobytes() == first[c].tobytes(), (family, "default again", c)


# ---- e. bytes in, bytes out ----

@pytest.mark.parametrize("dims", SMALL + LARGE, ids=F._ids)
def test_bytes_in_bytes_out(vr, tmp_path, dims):
    for family, law in [(f, "std") for f in families_at(dims)] + [("mixed", "chain_ns"), ("leafprune", "sat")]:
        lv = R.make_general(dims, family, law)
        packed = R.pack(lv.tokens)
        want, got = str(tmp_path / "want.bin"), str(tmp_path / "got.bin")
        R.write_file(want, dims, lv.tokens, lv.dmap)
        opened = vr.BrickSet.open(want)
        assert opened.dims == tuple(dims) and opened.num_bricks == 1
        info = opened.info(0)
        assert info["num_active_nodes"] == lv.tokens.size and info["tree_bytes"] == packed.size, family
        assert info["orig_tree_depth"] == lv.D and info["max_tree_depth"] == lv.M
        assert np.array_equal(opened.tree(0), packed) and np.array_equal(opened.distance_map(0), lv.dmap), family
        opened.save(got)
        assert open(got, "rb").read() == open(want, "rb").read(), (family, law)
        dec = R.decode_levels(lv)
        for c in (None, lv.D, max(lv.D - 2, 0)):
            assert np.array_equal(F.decode(opened, c)[0], dec.at(c)), (family, law, c)


def test_archive_round_trip(vr, tmp_path):
    """The archive of an installed set reopens to the same decode, its own archive is the same file, and the next
    timestep loads into the same handle."""
    dims = LARGE[0]
    steps = [[R.make_general(dims, "mixed", "std"), R.make_general(dims, "dense7", "chain_ns"), R.make_general(dims, "leafprune", "sat")],
             [R.make_general(dims, "blockprune", "chain_ns"), R.make_general(dims, "mixed", "sat"), R.make_general(dims, "dense7", "std")]]
    D, M = steps[0][0].D, steps[0][0].M
    Ds = D - 6
    cuts = [None, D, Ds - 1, 0]
    paths = [str(tmp_path / ("t%d.vrbs" % t)) for t in range(2)]
    for t, lvs in enumerate(steps):
        src = vr.BrickSet(3, dims)
        for b, lv in enumerate(lvs):
            F.install(vr, lv, brick=b, bs=src)
        src.save_set(paths[t])
    want = [{c: np.stack([R.decode_levels(lv).at(c) for lv in lvs]) for c in cuts} for lvs in steps]
    opened = vr.BrickSet.open_set(paths[0])
    assert opened.dims == tuple(dims) and opened.num_bricks == 3
    for c in cuts:
        assert np.array_equal(F.decode(opened, c), want[0][c]), c
    for b, lv in enumerate(steps[0]):
        assert np.array_equal(opened.tree(b), R.pack(lv.tokens)) and np.array_equal(opened.distance_map(b), lv.dmap)
        assert opened.info(b)["num_active_nodes"] == lv.tokens.size
    again = str(tmp_path / "again.vrbs")
    opened.save_set(again)
    assert open(again, "rb").read() == open(paths[0], "rb").read()
    opened.load_set(paths[1])
    for c in cuts:
        assert np.array_equal(F.decode(opened, c), want[1][c]), c
    for b, lv in enumerate(steps[1]):
        assert np.array_equal(opened.tree(b), R.pack(lv.tokens))


# ---- f. refusals: a stream the grammar does not produce ----

def malformed(t):
    return (("last token dropped", t[:-1]), ("a token appended", np.append(t, 0).astype(np.uint8)),
            ("ends inside a grown branch", t[:-3]))


@pytest.mark.parametrize("dims", [(12, 6, 5), (40, 16, 24)], ids=F._ids)
def test_malformed_streams_are_refused_by_set_tree(vr, dims):
    held = R.make_general(dims, "mixed", "std")
    bs = F.install(vr, held)
    before = F.decode(bs, None).copy()
    assert np.array_equal(before[0], R.decode_levels(held).at())
    lv = R.make_general(dims, "dense7", "sat")
    for what, bad in malformed(lv.tokens):
        with pytest.raises(vr.VrError) as e:
            bs.set_tree(0, R.pack(bad), bad.size, lv.dmap)
        assert e.value.status == VR_ERR_FORMAT, what
        assert bs.info(0)["num_active_nodes"] == held.tokens.size, what
        assert np.array_equal(bs.tree(0), R.pack(held.tokens)), what
        assert F.decode(bs, None).tobytes() == before.tobytes(), what
        assert np.array_equal(F.decode(bs, 0)[0], R.decode_levels(held).at(0)), what


@pytest.mark.parametrize("dims", [(12, 6, 5), (40, 16, 24)], ids=F._ids)
def test_malformed_streams_are_refused_by_set_trees(vr, dims):
    """The rule of tests/test_gpu_archive.py::test_malformed_input_is_refused: a stream that fails in the kernel leaves
    every brick named in the call never installed, the others untouched, and a later valid install succeeds."""
    held = [R.make_general(dims, "mixed", "std"), R.make_general(dims, "leafprune", "std"), R.make_general(dims, "blockprune", "sat")]
    decs = [R.decode_levels(lv) for lv in held]
    D, M = held[0].D, held[0].M
    good = R.make_general(dims, "mixed", "sat")
    lv = R.make_general(dims, "dense7", "sat")
    tab = table_of(lv)
    assert (tab[0] != DEAD).all()
    bs = install_many(vr, held)
    for what, bad in malformed(lv.tokens):
        with pytest.raises(vr.VrError) as e:
            bs.set_trees([0, 2], [R.pack(good.tokens), R.pack(bad)], [good.tokens.size, bad.size], [good.dmap, lv.dmap],
                         tables=[table_of(good), tab])
        assert e.value.status == VR_ERR_FORMAT, what
        assert [bs.info(b)["num_active_nodes"] for b in range(3)] == [0, held[1].tokens.size, 0], what
        got = lod(bs, [-1, M, -1])
        assert np.all(got[0] == POISON) and np.all(got[2] == POISON), what
        assert np.array_equal(got[1], decs[1].at()), what
        assert np.array_equal(lod(bs, [-1, 0, -1])[1], decs[1].at(0)), what
        install_many(vr, [held[0], held[2]], bricks=[0, 2], bs=bs)       # a later valid install succeeds
        for c in (None, D - 3, 0):
            assert np.array_equal(F.decode(bs, c), np.stack([d.at(c) for d in decs])), (what, c)
