"""Compressed brick-set archives on the GPU: vr_brickset_set_trees (stored streams installed in one call, the decode
index rebuilt by k_index_from_stream from a block table), cuts above the index depth without the host, the archive
file and the player.  Streams and references come from tests/refstream.py; the cuts and the switch rounds are those of
tests/test_gpu_foreign_streams.py.  Everything is bit-exact: no tolerance, no masked voxel.

The malformed inputs used here are a subset of the corpus tests/archive_main.cpp runs through the same walker source
under the sanitizers (tests/test_archive_cpu.py)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402
import test_gpu_foreign_streams as F  # noqa: E402  (helpers only: main_cuts, check_switches, decode)

pytestmark = pytest.mark.gpu

VR_ERR_STATE, VR_ERR_FORMAT, VR_ERR_UNSUPPORTED = -5, -6, -7
POISON = 0xA5
DEAD = 0xFFFFFFFF
ONE_WALKER = [(4, 1, 2), (16, 8, 4)]          # one walker from the root (D < 12)
BLOCKS = [(128, 8, 4), (128, 8, 8)]           # exactly one block (D = 12), two blocks
TILED = [(128, 64, 64), (128, 128, 64)]       # tile and region plans: 128 and 256 blocks, several waves of walkers
LAWS = ("std", "sat", "chain_ns")


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def table_of(lv):
    from volumerenderer_amd.codec import stream_block_table
    return stream_block_table(lv.dims, R.pack(lv.tokens), lv.tokens.size, lv.dmap)


def install(vr, lvs, bricks=None, bs=None, num_bricks=None, tables=True):
    """lvs installed as `bricks` (default 0 .. len - 1) in ONE vr_brickset_set_trees call."""
    bricks = list(range(len(lvs))) if bricks is None else list(bricks)
    if bs is None:
        bs = vr.BrickSet(num_bricks or len(lvs), lvs[0].dims)
    bs.set_trees(bricks, [R.pack(lv.tokens) for lv in lvs], [lv.tokens.size for lv in lvs], [lv.dmap for lv in lvs],
                 tables=[table_of(lv) for lv in lvs] if tables else None)
    return bs


def test_block_table_binding_matches_the_levels(vr):
    """vr_stream_block_table through the binding (no device needed): live blocks are the nodes of depth D - 12."""
    lv = R.make((128, 8, 8), "mixed", "std")
    off, top = table_of(lv)
    assert off.dtype == np.uint32 and off.size == 2 and top.size == 4
    assert np.array_equal(off != DEAD, lv.tok[1] != 255) and top[1] == lv.dmap[0]
    live = off != DEAD
    assert np.array_equal(lv.tokens[off[live].astype(np.int64)], lv.tok[1][live])


# ---- a. every family, installed on the GPU, against the NumPy reference ----

@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("dims", TILED, ids=F._ids)
def test_families_on_tiled_extents(vr, dims, family):
    for law in LAWS:
        lv = R.make(dims, family, law)
        F.check_switches(install(vr, [lv]), [R.decode_levels(lv)], F.main_cuts(lv.D, lv.M), (family, law))


@pytest.mark.parametrize("dims", ONE_WALKER + BLOCKS, ids=F._ids)
def test_families_on_small_extents(vr, dims):
    for family in R.FAMILIES:
        for law in LAWS:
            lv = R.make(dims, family, law)
            F.check_switches(install(vr, [lv]), [R.decode_levels(lv)], F.main_cuts(lv.D, lv.M), (family, law))


# ---- b. the host path is the reference: identical bytes from every decode ----

@pytest.mark.parametrize("laws", [("std", "sat", "std"), ("std", "chain_ns", "sat")], ids=["standard", "other_chain"])
@pytest.mark.parametrize("dims", [TILED[0], BLOCKS[1]], ids=F._ids)
def test_same_bytes_as_the_host_path(vr, dims, laws):
    import torch
    lvs = [R.make(dims, f, law) for f, law in zip(("mixed", "blockprune", "dense7"), laws)]
    gpu = install(vr, lvs, tables=False)                    # tables made by the call itself
    host = vr.BrickSet(3, dims)
    for b, lv in enumerate(lvs):
        host.set_tree(b, R.pack(lv.tokens), lv.tokens.size, lv.dmap)
    D, M = lvs[0].D, lvs[0].M
    Ds = D - min(D, 6)
    for b, lv in enumerate(lvs):
        assert gpu.info(b) == host.info(b)
        assert np.array_equal(gpu.tree(b), R.pack(lv.tokens)) and np.array_equal(gpu.distance_map(b), lv.dmap)
    for c in F.main_cuts(D, M):
        assert F.decode(gpu, c).tobytes() == F.decode(host, c).tobytes(), c
    X, Y, Z = dims
    plans = [[-1, Ds - 1, M], [0, -1, D - 3], [Ds, 3, -1], [D + 2, Ds - 2, 0], [M, M, M]]
    ijk, grid = np.array([(b, 0, 0) for b in range(3)], np.int64), (3, 1, 1)
    for cuts in plans:
        cuts = np.array(cuts, np.int32)
        got = []
        for bs in (gpu, host):
            out = torch.full((3 * X * Y * Z,), POISON, dtype=torch.uint8, device="cuda")
            bs.decode_lod(cuts, out=out)
            got.append(out.cpu().numpy().tobytes())
        assert got[0] == got[1], list(cuts)
        _, nbytes = vr.lod_pool_layout(dims, ijk, grid, cuts, D, M)
        got = []
        for bs in (gpu, host):
            pool = torch.full((nbytes + 4096,), POISON, dtype=torch.uint8, device="cuda")
            table = torch.full((3 * 16,), 0x5A, dtype=torch.uint8, device="cuda")
            bs.decode_lod_pool(cuts, ijk, grid, pool=pool, table=table)
            got.append(pool.cpu().numpy().tobytes() + table.cpu().numpy().tobytes())
        assert got[0] == got[1], list(cuts)


# ---- c. bricks never named, dead blocks, and re-installs that leave nothing behind ----

def test_reinstall_leaves_no_stale_entry(vr):
    import torch
    dims = TILED[0]
    X, Y, Z = dims
    first = {0: R.make(dims, "dense7", "std"), 1: R.make(dims, "root3", "std"), 2: R.make(dims, "shallow", "sat"),
             4: R.make(dims, "leafprune", "std")}
    D, M = first[0].D, first[0].M
    assert (table_of(first[2])[0] == DEAD).any() and (table_of(first[1])[0] == DEAD).all()      # blocks dead above depth D - 12
    bs = install(vr, list(first.values()), bricks=list(first), num_bricks=5)
    decs = {b: R.decode_levels(lv) for b, lv in first.items()}
    assert bs.info(3)["num_active_nodes"] == 0
    for cuts in ([M, D - 3, D - 7, -1, 0], [3, M, D + 2, -1, D - 7]):
        out = torch.full((5 * X * Y * Z,), POISON, dtype=torch.uint8, device="cuda")
        bs.decode_lod(np.array(cuts, np.int32), out=out)
        got = out.cpu().numpy().reshape(5, Z, Y, X)
        assert np.all(got[3] == POISON)
        for b in first:
            assert np.array_equal(got[b], decs[b].at(cuts[b])), (cuts, b)
    # every brick again, the one never named too, with sparser streams
    second = [R.make(dims, "blockprune", "std"), R.make(dims, "shallow", "std"), R.make(dims, "root3", "sat"),
              R.make(dims, "root_children3", "std"), R.make(dims, "blockprune", "sat")]
    assert second[0].tokens.size < first[0].tokens.size and second[4].tokens.size < first[4].tokens.size
    install(vr, second, bs=bs)
    fresh = install(vr, second)
    decs = [R.decode_levels(lv) for lv in second]
    cuts = [None, M - 1, D, D - 3, D - 6, D - 7, 3, 0]
    F.check_switches(bs, decs, cuts, "re-installed")
    for c in cuts:
        assert F.decode(bs, c).tobytes() == F.decode(fresh, c).tobytes(), c
    for b, lv in enumerate(second):
        assert bs.info(b)["num_active_nodes"] == lv.tokens.size and np.array_equal(bs.tree(b), R.pack(lv.tokens))


# ---- d. the archive: save, open, load ----

def sphere_bricks(dims, nb, phase):
    """uint8 [nb][Z][Y][X]: a soft ball per brick, moved and scaled by `phase` (what an encoder sees: smooth data with
    constant regions)."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    out = []
    for b in range(nb):
        c = np.array([X, Y, Z]) * (0.5 + 0.1 * np.sin(phase + b))
        r = np.sqrt((x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2)
        out.append(np.clip(255.0 - (6.0 + phase) * r, 0, 255).astype(np.uint8))
    return np.stack(out)


def test_archive_round_trip(vr, tmp_path):
    dims, nb = TILED[0], 2
    steps = [sphere_bricks(dims, nb, p) for p in (0.0, 1.5)]
    built = [vr.BrickSet(nb, dims, 2, 2).build(v.reshape(-1)) for v in steps]
    info = built[0].info(0)
    D = info["orig_tree_depth"]
    Ds = D - 6
    cuts = [None, D, D - 3, Ds, Ds - 1, 0]
    paths = [str(tmp_path / ("t%d.vrbs" % t)) for t in range(2)]
    for bs, p in zip(built, paths):
        bs.save_set(p)
    opened = vr.BrickSet.open_set(paths[0])
    assert opened.dims == tuple(dims) and opened.num_bricks == nb
    for c in cuts:
        assert F.decode(opened, c).tobytes() == F.decode(built[0], c).tobytes(), c
    for b in range(nb):
        assert np.array_equal(opened.tree(b), built[0].tree(b)) and np.array_equal(opened.distance_map(b), built[0].distance_map(b))
        assert opened.info(b)["num_active_nodes"] == built[0].info(b)["num_active_nodes"]
    # an archive of an installed set is the archive of the built one, byte for byte
    again = str(tmp_path / "again.vrbs")
    opened.save_set(again)
    assert open(again, "rb").read() == open(paths[0], "rb").read()
    # the next timestep into the same handle
    opened.load_set(paths[1])
    for c in cuts:
        assert F.decode(opened, c).tobytes() == F.decode(built[1], c).tobytes(), c
    for b in range(nb):
        assert np.array_equal(opened.tree(b), built[1].tree(b))
    # refusals that need no parse of a stream: geometry, magic, checksum; the set keeps the second timestep
    blob = bytearray(open(paths[0], "rb").read())
    other = vr.BrickSet(nb + 1, dims)
    for what, bad in (("magic", bytes([blob[0] ^ 1]) + bytes(blob[1:])), ("checksum", bytes(blob[:-1]) + bytes([blob[-1] ^ 0x40])),
                      ("cut short", bytes(blob[:-16]))):
        p = str(tmp_path / "bad.vrbs")
        open(p, "wb").write(bad)
        with pytest.raises(vr.VrError) as e:
            opened.load_set(p)
        assert e.value.status == VR_ERR_FORMAT, what
        with pytest.raises(vr.VrError) as e:
            vr.BrickSet.open_set(p)
        assert e.value.status == VR_ERR_FORMAT, what
    with pytest.raises(vr.VrError) as e:
        other.load_set(paths[0])
    assert e.value.status == VR_ERR_FORMAT
    assert F.decode(opened, None).tobytes() == F.decode(built[1], None).tobytes()


# ---- e. malformed input: refused, the named bricks never installed, the others untouched ----

@pytest.mark.parametrize("dims", [BLOCKS[1], TILED[0]], ids=F._ids)
def test_malformed_input_is_refused(vr, dims):
    import torch
    X, Y, Z = dims
    held = [R.make(dims, "mixed", "std"), R.make(dims, "leafprune", "std"), R.make(dims, "blockprune", "sat")]
    decs = [R.decode_levels(lv) for lv in held]
    M = held[0].M
    good = R.make(dims, "mixed", "sat")
    lv = R.make(dims, "dense7", "sat")
    t, tab = lv.tokens, table_of(lv)
    assert (tab[0] != DEAD).all() and tab[0].size >= 2
    swapped, late, shifted = tab[0].copy(), tab[0].copy(), tab[0].copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    late[-1] = t.size
    shifted[-1] += 1
    by_host = [("offsets that do not increase", t, (swapped, tab[1])), ("an offset at the end of the stream", t, (late, tab[1]))]
    by_kernel = [("last token dropped", t[:-1], tab), ("ends inside a grown branch", t[:-3], tab),
                 ("a token appended", np.append(t, 0).astype(np.uint8), tab), ("an offset off by one", t, (shifted, tab[1]))]
    bs = install(vr, held)

    def attempt(bad, table):
        with pytest.raises(vr.VrError) as e:
            bs.set_trees([0, 2], [R.pack(good.tokens), R.pack(bad)], [good.tokens.size, bad.size], [good.dmap, lv.dmap],
                         tables=[table_of(good), table])
        return e.value.status

    for what, bad, table in by_host:            # checked before anything is enqueued: the set is unchanged
        assert attempt(bad, table) == VR_ERR_FORMAT, what
        assert [bs.info(b)["num_active_nodes"] for b in range(3)] == [h.tokens.size for h in held], what
        assert np.array_equal(F.decode(bs, None), np.stack([d.at() for d in decs])), what
    for what, bad, table in by_kernel:
        assert attempt(bad, table) == VR_ERR_FORMAT, what
        assert [bs.info(b)["num_active_nodes"] for b in range(3)] == [0, held[1].tokens.size, 0], what
        out = torch.full((3 * X * Y * Z,), POISON, dtype=torch.uint8, device="cuda")
        bs.decode_lod(np.array([-1, M, -1], np.int32), out=out)
        got = out.cpu().numpy().reshape(3, Z, Y, X)
        assert np.all(got[0] == POISON) and np.all(got[2] == POISON), what
        assert np.array_equal(got[1], decs[1].at()), what
        assert np.array_equal(F.decode(bs, held[1].D - 7)[1], decs[1].at(held[1].D - 7)), what
        install(vr, [held[0], held[2]], bricks=[0, 2], bs=bs)       # a later valid install succeeds
        assert np.array_equal(F.decode(bs, None), np.stack([d.at() for d in decs])), what
        assert np.array_equal(F.decode(bs, 3), np.stack([d.at(3) for d in decs])), what


# ---- f. the player ----

def test_archive_player(vr, tmp_path):
    from volumerenderer_amd.pipeline import ArchivePlayer, ArchiveSource
    dims, nb = (32, 32, 16), 3
    steps = [sphere_bricks(dims, nb, p) for p in (0.0, 1.0, 2.0)]
    built = [vr.BrickSet(nb, dims, 2, 2).build(v.reshape(-1)) for v in steps]
    paths = [str(tmp_path / ("t%d.vrbs" % t)) for t in range(3)]
    for bs, p in zip(built, paths):
        bs.save_set(p)
    info = built[0].info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    lod = np.array([D - 7, M, D - 2], np.int32)
    player = ArchivePlayer(nb, dims)
    for kwargs, want in (({}, [bs.decode() for bs in built]), ({"cut_depth": D - 3}, [bs.decode(cut_depth=D - 3) for bs in built]),
                         ({"cuts": lod}, [bs.decode_lod(lod) for bs in built])):
        for overlap in (True, False):
            seen = {}
            player.run(ArchiveSource(paths), on_decoded=lambda t, vol, stream: seen.__setitem__(t, vol.clone()),
                       overlap=overlap, **kwargs)
            assert sorted(seen) == [0, 1, 2]
            for t in range(3):
                assert seen[t].cpu().numpy().tobytes() == want[t].cpu().numpy().tobytes(), (kwargs, overlap, t)


# ---- g. what this call does not serve ----

def test_refusals_by_state_and_variant(vr):
    dims = (16, 8, 4)
    lv = R.make(dims, "mixed", "std")
    args = ([0], [R.pack(lv.tokens)], [lv.tokens.size], [lv.dmap])
    mr = vr.BrickSet(1, dims, variant=vr.VARIANT_MIDRANGE)
    with pytest.raises(vr.VrError) as e:
        mr.set_trees(*args)
    assert e.value.status == VR_ERR_UNSUPPORTED
    built = vr.BrickSet(1, dims).build(np.zeros(16 * 8 * 4, np.uint8))
    with pytest.raises(vr.VrError) as e:
        built.set_trees(*args)
    assert e.value.status == VR_ERR_STATE
    assert built.info(0)["num_active_nodes"] > 0 and not built.decode().any()
