"""k_index12 -- the decode index of a fused build, 32 consecutive 4096-leaf blocks per workgroup, dead blocks written in
16-byte pieces, constant bricks included -- against the CPU oracle and against the same data built under the
`index_per_block` switch (k_index12_block, a wave per block, with k_const_finish over every entry of a constant brick).

The index is not visible to the host; what reads it is: the decode at every cut that starts from another index array
(D-7 and D-6: idxVal; D-3: idxVal3; D and the full depth: idxOff and the strings), through k_decode_region (default),
k_decode_quad and the walking kernel, and a decode_lod whose cuts differ from brick to brick.  All of that, with stream
bytes, distance maps and info(), is compared bit for bit between the two handles; the default handle is also compared
with the oracle (trees, distance maps, info, full decode).

Shapes are the smallest at which the kernel can go wrong: one block (31 idle prologue lanes), four (the smallest with
SkipBlocks), exactly one full workgroup, two workgroups.  The contents put dead runs of 1, 2 and 15 blocks, a run across
the workgroup boundary at block 32, a dead tail, a workgroup without a live block, one whose only live block is its
last, all-live bricks and constant bricks between busy ones into the 64-block shape.  Whether a constant box beside
noise is dead or a uniform string (live) depends on the level distances: `_runs` builds bricks in which it is dead
for certain, `_mixed` bricks hold both kinds, and test_content_classes reads the classes off the oracle."""
import numpy as np
import pytest

from test_gpu_const_boxes import (MIX_VALUES, _against_oracle, _from_leaves, _leaf_order, _make, _mixed, _noise_box, _outputs,
                                  _refs, _same)
from test_gpu_const_boxes import vr  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

S12 = (16, 16, 16)          # (z, y, x): D = 12, one block
S14 = (16, 32, 32)          # D = 14, four blocks
S17 = (32, 64, 64)          # D = 17, 32 blocks: one workgroup
S18 = (64, 64, 64)          # D = 18, 64 blocks: two workgroups
BENCH = (128, 256, 256)     # bench.py's brick

RUNS = (0, 2, 5, 21, 37, 38)        # live blocks: dead runs 1, 2-4, 6-20, 22-36 (across block 32), 39-63


def _nblk(shape):
    return shape[0] * shape[1] * shape[2] // 4096


def _runs(O, shape, busy, seed, v=128, amp=28):
    """Boxes `busy` are noise whose extremes are v - amp and v + amp, all others are v.  Every depth-(D-12) truth is then
    v, every level above has distance 0 and reproduces v exactly, and every constant box is pruned at its root or
    above: dead for certain, where `_mixed` leaves it to the level distances whether a constant box is dead or a
    uniform string (`_dead_boxes` reads the class off the oracle)."""
    rng = np.random.default_rng(seed)
    leaves = np.full((_nblk(shape), 4096), v, np.int64)
    for b in busy:
        box = np.clip(_noise_box(rng) - 128 + v, v - amp, v + amp)
        box[0], box[4095] = v - amp, v + amp
        leaves[b] = box
    return _from_leaves(O, leaves.reshape(-1).astype(np.uint8), shape)


def _contents(O, shape, which="A"):
    """Bricks of `shape`: for 64 blocks the patterns named above; for fewer blocks what is left of them."""
    nb = _nblk(shape)
    rng = np.random.default_rng(41 + nb + (7 if which == "B" else 0))
    noise = rng.integers(0, 256, shape, dtype=np.uint8)
    if nb < 64:
        vols = [_runs(O, shape, (0,), 1), np.full(shape, 8, np.uint8), noise, np.full(shape, 0, np.uint8),
                _runs(O, shape, (nb - 1,), 2, v=131), np.full(shape, 255, np.uint8),
                _mixed(O, shape, 3, [128, 131], busy=tuple(range(0, nb, 3))), _mixed(O, shape, 4, MIX_VALUES, busy=(nb // 2,))]
        return vols if which == "A" else vols[::-1]
    if which == "B":
        return [np.full(shape, 131, np.uint8), _runs(O, shape, (31, 32), 11), noise,
                _mixed(O, shape, 12, [128, 131], busy=tuple(range(0, 32))), np.full(shape, 8, np.uint8),
                _runs(O, shape, (1, 62), 13, v=90), _mixed(O, shape, 14, MIX_VALUES, busy=RUNS),
                np.full(shape, 0, np.uint8), _mixed(O, shape, 15, [90, 200], busy=()), _runs(O, shape, tuple(range(0, 32)), 16)]
    return [_runs(O, shape, RUNS, 1), np.full(shape, 0, np.uint8), _runs(O, shape, (63,), 2), np.full(shape, 8, np.uint8),
            _runs(O, shape, tuple(range(32, 64)), 3, v=200), noise, np.full(shape, 255, np.uint8),
            _mixed(O, shape, 4, [128, 131], busy=(3, 40)), _mixed(O, shape, 5, [128, 131], busy=()),
            _mixed(O, shape, 6, MIX_VALUES, busy=RUNS)]


_CACHE = {}


def _case(O, shape, which="A", tol=1, ep=2, midrange=False):
    """(volumes, oracle trees) of a content set: computed once, shared by the tests, never changed"""
    key = (shape, which, tol, ep, midrange)
    if key not in _CACHE:
        vols = [np.ascontiguousarray(v) for v in _contents(O, shape, which)]
        _CACHE[key] = (vols, _refs(O, vols, tol, ep, midrange))
    return _CACHE[key]


def _with(bs, switch, fn):
    if switch is None:
        return fn()
    bs.set_switch(switch, 1)
    try:
        return fn()
    finally:
        bs.set_switch(switch, 0)


def _index_outputs(bs, n, shape, midrange):
    """_outputs and everything that consumes the index"""
    out = _outputs(bs, n, shape, midrange)
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    cuts = sorted({D - 7, D - 6, D - 3, D, M})
    for sw in (None, "decode_quad", "decode_walk"):
        for c in cuts:
            out["cut%d %s" % (c, sw)] = _with(bs, sw, lambda: bs.decode(cut_depth=c).cpu().numpy())
            if midrange:
                out["range cut%d %s" % (c, sw)] = _with(bs, sw, lambda: bs.decode_range(cut_depth=c).cpu().numpy())
    lod = [cuts[(3 * b + 1) % len(cuts)] for b in range(n)]
    out["lod"] = bs.decode_lod(lod).cpu().numpy()
    return out


def _check(vr, vols, refs, tol, ep, midrange=False):
    """A fresh default handle against the oracle and against a handle built with index_per_block"""
    n, shape = len(vols), vols[0].shape
    what = (shape, tol, ep, midrange)
    new = _make(vr, n, shape, tol, ep, midrange).build(np.stack(vols))
    _against_oracle(new, vols, refs, midrange, what)
    old = _make(vr, n, shape, tol, ep, midrange, switches=("index_per_block",)).build(np.stack(vols))
    _same(_index_outputs(new, n, shape, midrange), _index_outputs(old, n, shape, midrange), what)


def _live_boxes(O, ref, shape):
    """boxes whose 4096 decoded voxels are not one value: live for certain (a dead block decodes to one scalar); the
    others are dead blocks or uniform strings"""
    leaves = ref.levelCut().reshape(-1)[_leaf_order(O, shape)].reshape(_nblk(shape), 4096)
    return set(np.flatnonzero(~(leaves == leaves[:, :1]).all(axis=1)).tolist())


@pytest.mark.parametrize("shape", [S12, S14, S17, S18], ids=["16x16x16", "32x32x16", "64x64x32", "64x64x64"])
def test_shapes(vr, oracle, shape):
    """Tolerance 1, two epochs: dead, live and constant-brick blocks in every shape."""
    vols, refs = _case(oracle, shape)
    _check(vr, vols, refs, 1, 2)


def _dead_boxes(O, vol, ref):
    """constant boxes whose depth-(D-12) node the oracle reconstructs exactly: everything below keeps that value, so
    the node (or an ancestor) is a pruned token and the block is dead for certain"""
    nb = _nblk(vol.shape)
    leaves = vol.reshape(-1)[_leaf_order(O, vol.shape)].reshape(nb, 4096)
    const = (leaves == leaves[:, :1]).all(axis=1)
    return set(np.flatnonzero(const & (np.asarray(ref.recon_all)[nb - 1:2 * nb - 1] == leaves[:, 0])).tolist())


def test_content_classes(oracle):
    """The contents hold the runs they are named for, read off the oracle: which boxes are live for certain (their
    decode is not one value) and which are dead for certain (constant and exact at the block's root)."""
    vols, refs = _case(oracle, S18)
    every = set(range(64))
    for b, live in ((0, set(RUNS)), (2, {63}), (4, set(range(32, 64)))):
        assert _live_boxes(oracle, refs[b], S18) == live, b
        assert _dead_boxes(oracle, vols[b], refs[b]) == every - live, b
    assert _live_boxes(oracle, refs[5], S18) == every
    assert _live_boxes(oracle, refs[7], S18) == {3, 40}
    # constant boxes of MIX_VALUES between six noise boxes: dead ones and uniform strings (live) side by side
    dead = _dead_boxes(oracle, vols[9], refs[9])
    assert _live_boxes(oracle, refs[9], S18) == set(RUNS) and 0 < len(dead) < 64 - len(RUNS)
    for b, v in ((1, 0), (3, 8), (6, 255)):
        assert int(vols[b].min()) == v == int(vols[b].max())
    for shape, nb in ((S14, 4), (S17, 32)):
        vols, refs = _case(oracle, shape)
        assert _dead_boxes(oracle, vols[0], refs[0]) == set(range(1, nb))
        assert _dead_boxes(oracle, vols[4], refs[4]) == set(range(nb - 1))
    vols, refs = _case(oracle, S18, "B")
    assert _dead_boxes(oracle, vols[1], refs[1]) == every - {31, 32}
    assert _dead_boxes(oracle, vols[5], refs[5]) == every - {1, 62}


def test_tolerance_zero(vr, oracle):
    """Nothing is pruned: every block is live, those of constant boxes and constant bricks too."""
    vols, refs = _case(oracle, S17, tol=0)
    _check(vr, vols, refs, 0, 2)


def test_midrange_tree(vr, oracle):
    """Variant 2: the index serves both streams' decodes."""
    vols, refs = _case(oracle, S14, midrange=True)
    _check(vr, vols, refs, 1, 2, midrange=True)


def test_block_relative_entries(vr, oracle, monkeypatch):
    """64-bit trees keep the entries relative to their block and the blocks' offsets in idxBase, written by the
    prologue's lanes: VRHIP_FORCE_IDX64 takes small bricks through that path, on two workgroups."""
    monkeypatch.setenv("VRHIP_FORCE_IDX64", "1")
    vols, refs = _case(oracle, S18)
    _check(vr, vols, refs, 1, 2)


def test_rebuilds_on_one_handle(vr, oracle):
    """A, B, A, B on one handle with the switch off, on, on, off: blocks flip between dead and live, bricks between
    constant and not, and the two kernels alternate.  Every rebuild equals the oracle and a fresh handle: a byte left
    from the other kernel or the other build would show."""
    sets = {"A": _case(oracle, S18, "A"), "B": _case(oracle, S18, "B")}
    n = len(sets["A"][0])
    assert len(sets["B"][0]) == n
    bs = _make(vr, n, S18, 1, 2)
    for name, per_block in (("A", 0), ("B", 1), ("A", 1), ("B", 0)):
        V, R = sets[name]
        bs.set_switch("index_per_block", per_block)
        bs.build(np.stack(V))
        what = "rebuild %s, index_per_block %d" % (name, per_block)
        _against_oracle(bs, V, R, False, what)
        fresh = _make(vr, n, S18, 1, 2).build(np.stack(V))
        _same(_index_outputs(bs, n, S18, False), _index_outputs(fresh, n, S18, False), what + ", against a fresh handle")


def test_bench_brick(vr):
    """One brick of the benchmark's volume, 2048 blocks: against the switch only (the oracle is too slow here)."""
    import bench
    vols = list(bench.make_bricks("rm_like", 1, BENCH[::-1], 12345))
    assert int(vols[0].min()) != int(vols[0].max())
    new = _make(vr, 1, BENCH, 1, 2).build(np.stack(vols))
    old = _make(vr, 1, BENCH, 1, 2, switches=("index_per_block",)).build(np.stack(vols))
    _same(_index_outputs(new, 1, BENCH, False), _index_outputs(old, 1, BENCH, False), "bench brick")
