"""The install path as a sequence (DESIGN.md "Installed streams"): plan, host pass, buffers, and only then the first
write.  Pinned here on the device: a refused vr_brickset_set_tree / vr_brickset_set_trees call leaves a set of installed
streams, and a fresh set, exactly as it was; and the two engines, taking turns on one brick beside a neighbour the other
engine installed, always leave what a fresh handle with the same streams holds.  Streams and references come from
tests/refstream.py; the plan's own fields are compared without a device in tests/test_install_plan.py.  A grammar error
the device finds is vr_brickset_set_trees' documented "every named brick left never installed":
test_gpu_foreign_general.py and test_gpu_archive.py keep that."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402
import test_gpu_foreign_streams as F  # noqa: E402  (helpers only: decode, _ids)
from test_gpu_foreign_general import lod, table_of  # noqa: E402

pytestmark = pytest.mark.gpu

VR_OK, VR_ERR_INVALID, VR_ERR_STATE, VR_ERR_FORMAT = 0, -1, -5, -6
# D = 12, one block; D = 13, two blocks; D = 4 < 6, no fine side-car; general extents, D = 7
EXTENTS = [(16, 16, 16), (32, 16, 16), (4, 2, 2), (12, 6, 5)]


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def make(dims, family, law):
    general = any(d & (d - 1) for d in dims)
    return R.make_general(dims, family, law) if general else R.make(dims, family, law)


def _ptr(a):
    return None if a is None else a.ctypes.data


def raw_set_tree(bs, brick, tree, nbytes, na, dmap, maplen):
    return bs._L.vr_brickset_set_tree(bs._h, int(brick), _ptr(tree), int(nbytes), int(na), _ptr(dmap), int(maplen))


def raw_set_trees(bs, bricks, rows):
    """rows: (tree, tree_bytes, num_active, dmap, map_len, block_off, top_val) per entry; the status, not an exception"""
    from volumerenderer_amd import _lib
    descs = (_lib.TreeDesc * len(rows))()
    for d, (tree, nbytes, na, dmap, maplen, off, top) in zip(descs, rows):
        d.tree, d.tree_bytes, d.num_active, d.distance_map, d.map_len = _ptr(tree), int(nbytes), int(na), _ptr(dmap), int(maplen)
        d.block_off, d.top_val = _ptr(off), _ptr(top)
    b = np.asarray(bricks, np.int32)
    return bs._L.vr_brickset_set_trees(bs._h, len(rows), b.ctypes.data_as(C.POINTER(C.c_int32)), descs, None)


def good_row(lv, tables=True):
    t = R.pack(lv.tokens)
    off, top = table_of(lv) if tables else (None, None)
    return [t, t.size, lv.tokens.size, np.ascontiguousarray(lv.dmap, np.uint8), lv.dmap.size, off, top]


def refusals(engine, bad, good):
    """(name, call(bs) -> status, expected status): every refusable call that needs no fault.  `bad` aims at brick 0;
    the device engine's calls carry a flawless entry for brick 1 in front of it, which must not be installed either."""
    D = bad.D
    Dc = max(D - 12, 0)

    def row(**change):
        r = good_row(bad)
        for k, v in change.items():
            r[("tree", "nbytes", "na", "dmap", "maplen", "off", "top").index(k)] = v
        return r

    need = (bad.tokens.size + 3) // 4
    assert need >= 2
    wrong = table_of(bad)[0].copy()
    wrong[0] = Dc + 1               # block 0 is at token Dc or dead (host_plan.h block_table_ok)
    if engine == "set_tree":
        one = lambda brick, r: (lambda bs: raw_set_tree(bs, brick, *r[:5]))     # noqa: E731
        return [("short tree_bytes", one(0, row(nbytes=need - 1)), VR_ERR_FORMAT),
                ("short map_len", one(0, row(maplen=bad.M)), VR_ERR_INVALID),
                ("num_active 0", one(0, row(na=0)), VR_ERR_INVALID),
                ("brick out of range", one(3, row()), VR_ERR_INVALID)]
    two = lambda r, bricks=(1, 0): (lambda bs: raw_set_trees(bs, bricks, [good_row(good), r]))      # noqa: E731
    return [("short tree_bytes", two(row(nbytes=need - 1)), VR_ERR_FORMAT),
            ("short map_len", two(row(maplen=bad.M)), VR_ERR_INVALID),
            ("num_active 0", two(row(na=0)), VR_ERR_INVALID),
            ("a brick named twice", two(row(), (1, 1)), VR_ERR_INVALID),
            ("one table pointer null", two(row(top=None)), VR_ERR_INVALID),
            ("the other table pointer null", two(row(off=None)), VR_ERR_INVALID),
            ("a table that fails the host check", two(row(off=wrong)), VR_ERR_FORMAT),
            ("brick out of range", two(row(), (1, 3)), VR_ERR_INVALID)]


def put(vr, engine, bs, bricks, lvs):
    if engine == "set_tree":
        for b, lv in zip(bricks, lvs):
            F.install(vr, lv, brick=b, bs=bs)
    else:
        assert raw_set_trees(bs, bricks, [good_row(lv) for lv in lvs]) == VR_OK


def state_of(bs, cuts, bricks):
    """everything a caller can read of the set: info, bytes and map of every brick, and the decodes of `bricks` at `cuts`"""
    n = bs.num_bricks
    s = [(bs.info(b), bs.tree(b).tobytes() if bs.info(b)["num_active_nodes"] else b"", bs.distance_map(b).tobytes()) for b in range(n)]
    return s + [lod(bs, [c if b in bricks else -1 for b in range(n)]).tobytes() for c in cuts]


@pytest.mark.parametrize("engine", ["set_tree", "set_trees"])
@pytest.mark.parametrize("dims", EXTENTS, ids=F._ids)
def test_refused_calls_change_nothing(vr, dims, engine):
    held = [make(dims, "mixed", "std"), make(dims, "leafprune", "chain_ns")]     # bricks 0 and 2; brick 1 never installed
    bad, good = make(dims, "shallow", "sat"), make(dims, "dense0", "std")
    D, M = bad.D, bad.M
    Ds = D - min(D, 6)
    cuts = sorted({Ds, max(Ds - 1, 0), M})          # the index depth, below it, the maximum depth
    other = "set_trees" if engine == "set_tree" else "set_tree"
    for holder in (engine, other):                  # whichever engine installed what the set holds
        bs = vr.BrickSet(3, dims)
        put(vr, holder, bs, [0, 2], held)
        before = state_of(bs, cuts, (0, 2))
        assert before[1][0]["num_active_nodes"] == 0
        for name, call, status in refusals(engine, bad, good):
            assert call(bs) == status, (holder, name)
            assert state_of(bs, cuts, (0, 2)) == before, (holder, name)
    # a fresh set stays fresh, and a good install after the refusals gives what a fresh handle gets
    bs = vr.BrickSet(3, dims)
    for name, call, status in refusals(engine, bad, good):
        assert call(bs) == status, ("fresh", name)
        with pytest.raises(vr.VrError) as e:
            bs.save_set(os.devnull)
        assert e.value.status == VR_ERR_STATE, ("fresh", name)
    put(vr, engine, bs, [0, 2], held)
    fresh = vr.BrickSet(3, dims)
    put(vr, engine, fresh, [0, 2], held)
    assert state_of(bs, cuts, (0, 2)) == state_of(fresh, cuts, (0, 2)) == before


@pytest.mark.parametrize("dims", [(32, 16, 16), (12, 6, 5)], ids=F._ids)
def test_the_two_engines_take_turns_on_one_set(vr, dims):
    """brick 0 by set_tree, set_trees, set_tree, each time another stream (standard and other grown-branch distances:
    the fine rule decides anew), and each time brick 1 again by the other engine: the cut values of a brick change
    their source between the host bytes and the heap the kernel wrote, under one shared state"""
    turns = [("set_tree", make(dims, "mixed", "std"), make(dims, "blockprune", "std")),
             ("set_trees", make(dims, "dense7", "chain_ns"), make(dims, "shallow", "sat")),
             ("set_tree", make(dims, "leafprune", "sat"), make(dims, "mono_up", "chain_ns"))]
    D, M = turns[0][1].D, turns[0][1].M
    Ds = D - min(D, 6)
    cuts = sorted({M, D, D - 3, Ds, Ds - 1, 0}, reverse=True)
    bs = vr.BrickSet(2, dims)
    for engine, lv, neighbour in turns:
        other = "set_trees" if engine == "set_tree" else "set_tree"
        put(vr, engine, bs, [0], [lv])
        put(vr, other, bs, [1], [neighbour])
        for how in ("set_tree", "set_trees"):
            fresh = vr.BrickSet(2, dims)
            put(vr, how, fresh, [0, 1], [lv, neighbour])
            for b in (0, 1):
                assert bs.info(b) == fresh.info(b), (engine, how, b)
                assert bs.tree(b).tobytes() == fresh.tree(b).tobytes() and bs.distance_map(b).tobytes() == fresh.distance_map(b).tobytes()
            decs = [R.decode_levels(lv), R.decode_levels(neighbour)]
            for c in cuts:
                got = F.decode(bs, c)
                assert got.tobytes() == F.decode(fresh, c).tobytes(), (engine, how, c)
                assert np.array_equal(got, np.stack([d.at(c) for d in decs])), (engine, c)
