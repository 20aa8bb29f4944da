"""k_decode_region's uniform path: a 16^3 box that k_prune_emit12_const composed a string for (BrickSet::boxUniform) is
decoded as one quad and broadcast.  Against the CPU oracle, against the same handle with `no_uniform_decode` on (every
live box parsed token by token) and against `decode_quad` (round 2's kernel, which never reads the flag).

The shapes are the smallest that region_plan accepts, one per position of x in the deepest (a, b, c) triple:
128x64x64 (x deepest, 16 regions of eight boxes), 128x128x64 (x second, the bench's order) and 128x128x128 (x first).

Kinds of box, read off the oracle's own stream and reconstruction (`_kinds`): 'busy' (not constant), and for the
constant boxes of a busy brick 'live' (255 tokens or more: pruned no higher than in-block level 7, so its 64 index
entries are live -- the boxes the new path serves), 'short' (3 .. 127 tokens), 'one' (one token) and 'none' (under a
pruned ancestor); the last three have dead index entries and take the dead-block path as before.  Every case asserts
that the kinds it is about occur.

A launch gives a workgroup the regions rid, rid + G, ...: with 512 bricks of 128x64x64 G is 4, a workgroup walks the
four regions of one y position (rid = 4 (z >> 4) + (y >> 4)), and wave w decodes box w along x of each (`_walks`)."""
import numpy as np
import pytest

from test_gpu_const_boxes import MIX_VALUES, _box_geom, _from_leaves, _make, _mixed, _noise_box, _refs
from test_gpu_const_boxes import vr  # noqa: F401  (the module's fixture)
from test_gpu_uniform_blocks import EDGE_VALUES, _box_classes, _box_tokens

pytestmark = pytest.mark.gpu

SHAPES = {"128x64x64": (64, 64, 128), "128x128x64": (64, 128, 128), "128x128x128": (128, 128, 128)}      # (z, y, x)
FAR = [90, 200, 0, 255, 3, 252]         # far from the noise boxes' midrange (128)
RULES = (0, 1, 2, 3, 4)


# ---------------------------------------------------------------- geometry and census ----
_REGIONS = {}


def _regions(O, shape):
    """the regions of a brick in the kernel's order (x fastest, then y, then z): eight box numbers each, along x"""
    if shape not in _REGIONS:
        by = {}
        for b in range(shape[0] * shape[1] * shape[2] // 4096):
            (ox, oy, oz), e = _box_geom(O, shape, b)
            assert e == (16, 16, 16), e
            by.setdefault((oz // 16, oy // 16, ox // 128), []).append((ox, b))
        _REGIONS[shape] = [[b for _, b in sorted(v)] for _, v in sorted(by.items())]
        assert all(len(r) == 8 for r in _REGIONS[shape])
    return _REGIONS[shape]


def _kinds(O, vol, ref):
    """[(kind, tokens)] per box"""
    out = []
    for k, n in zip(_box_classes(O, vol, ref), _box_tokens(ref)):
        if k in ("skipped", "filled"):
            k = "live" if n >= 255 else ("short" if n > 1 else ("one" if n == 1 else "none"))
        out.append((k, n))
    return out


def _rule_boxes(rule, i):
    """the eight boxes of region i under a rule: a value, or None for a noise box"""
    far = [FAR[(i + k) % len(FAR)] for k in range(8)]
    if rule == 0:
        return far
    if rule == 1:
        return [None if k % 2 == 0 else 252 for k in range(8)]
    if rule == 2:
        return [128] * 8
    if rule == 3:
        return far[:4] + [128] * 4
    return [200] * 6 + [None] * 2


def _by_rule(O, shape, seed, rules=RULES):
    """region i filled by rules[i mod len(rules)]"""
    rng = np.random.default_rng(seed)
    regs = _regions(O, shape)
    leaves = np.empty((8 * len(regs), 4096), np.int64)
    for i, r in enumerate(regs):
        for b, v in zip(r, _rule_boxes(rules[i % len(rules)], i)):
            leaves[b] = _noise_box(rng) if v is None else v
    return _from_leaves(O, leaves.reshape(-1).astype(np.uint8), shape)


def _volumes(O, shape, tol):
    """the busy bricks of a shape's set at tolerance 1 (two epochs) or 2 (one epoch)"""
    nb = shape[0] * shape[1] * shape[2] // 4096
    values = MIX_VALUES + EDGE_VALUES
    if nb > 128:      # the larger shapes: the bricks that bring each kind, no more (the oracle's time grows with the voxels)
        if tol == 1:
            return [_mixed(O, shape, 2, values, busy=range(0, nb, nb // 16)), _by_rule(O, shape, 1)]
        return [_by_rule(O, shape, 1), _by_rule(O, shape, 2)]
    if tol == 1:
        return [_mixed(O, shape, 1, values, busy=range(3, nb, nb // 5)), _mixed(O, shape, 2, values, busy=range(0, nb, nb // 16)),
                _mixed(O, shape, 4, values, busy=range(1, nb, nb // 9)), _by_rule(O, shape, 1), _by_rule(O, shape, 2, (4, 2, 0, 1, 3))]
    return [_by_rule(O, shape, 1), _by_rule(O, shape, 2), _mixed(O, shape, 2, values, busy=range(2, nb, 17)),
            _mixed(O, shape, 6, values, busy=range(6, nb, 17))]


_SETS = {}


def _set(O, name, tol):
    """(volumes, oracle builds, kinds per brick, epochs) of one shape's set, made once: the busy bricks, then a constant
    brick and an all-noise brick"""
    if (name, tol) not in _SETS:
        shape = SHAPES[name]
        ep = 2 if tol == 1 else 1
        nb = shape[0] * shape[1] * shape[2] // 4096
        rng = np.random.default_rng(77)
        noise = _from_leaves(O, np.concatenate([_noise_box(rng) for _ in range(nb)]).astype(np.uint8), shape)
        vols = _volumes(O, shape, tol) + [np.full(shape, 77, np.uint8), noise]
        vols = [np.ascontiguousarray(v) for v in vols]
        refs = _refs(O, vols, tol, ep)
        kinds = [_kinds(O, v, r) for v, r in zip(vols[:-2], refs[:-2])]
        kinds += [[("brick", 0)] * nb, [(k, 0) for k in _box_classes(O, vols[-1], refs[-1])]]
        assert all(k == "busy" for k, _ in kinds[-1])
        _SETS[(name, tol)] = (vols, refs, kinds, ep)
    return _SETS[(name, tol)]


def _region_kinds(O, shape, kinds):
    """per brick, per region: the eight kinds along x"""
    return [[[k[b][0] for b in r] for r in _regions(O, shape)] for k in kinds]


def _cuts(ref):
    D, M = ref.origTreeDepth, ref.maxTreeDepth
    return [M, M - 1, D + 4, D + 1, D, D - 1, D - 2, D - 3]


def _want(ref, cut):
    return ref.levelCut() if cut == ref.maxTreeDepth else ref.levelCutProgressive(cut)


def _with(bs, switch, fn):
    bs.set_switch(switch, 1)
    try:
        return fn()
    finally:
        bs.set_switch(switch, 0)


def _against(bs, vols, refs, cuts, what):
    """decode at every cut: the uniform path against the parsed path, k_decode_quad and the oracle"""
    n, shape = len(vols), vols[0].shape
    for cut in cuts:
        got = bs.decode(cut_depth=cut)
        assert (got == _with(bs, "no_uniform_decode", lambda: bs.decode(cut_depth=cut))).all(), (what, cut)
        assert (got == _with(bs, "decode_quad", lambda: bs.decode(cut_depth=cut))).all(), (what, cut)
        got = got.cpu().numpy().reshape((n,) + shape)
        for b, ref in enumerate(refs):
            assert np.array_equal(got[b], _want(ref, cut)), (what, b, cut)


# ---------------------------------------------------------------- the cases ----
@pytest.mark.parametrize("name", list(SHAPES))
def test_every_kind_every_cut(vr, oracle, name):
    """Regions of eight live uniform boxes, live uniform alternating with busy, live uniform beside one-token boxes,
    the two longest strings and a shorter one, a constant and an all-noise brick in the same launch: every cut the
    kernel serves, and per-brick cuts through decode_lod."""
    shape = SHAPES[name]
    seen, lens = set(), set()
    for tol in (1, 2):
        vols, refs, kinds, ep = _set(oracle, name, tol)
        for brick in _region_kinds(oracle, shape, kinds):
            for r in brick:
                if all(k == "live" for k in r):
                    seen.add("eight live")
                if all(k == ("busy", "live")[i % 2] for i, k in enumerate(r)):
                    seen.add("alternating")
                if "live" in r and "one" in r:
                    seen.add("live beside one-token")
        lens |= {n for k in kinds for kk, n in k if kk == "live"}
    print("%s: %r, live uniform lengths %r" % (name, sorted(seen), sorted(lens)))
    assert seen == {"eight live", "alternating", "live beside one-token"}, seen
    assert {12287, 36863} <= lens and min(lens) < 12287, sorted(lens)
    for tol in (1, 2):
        vols, refs, kinds, ep = _set(oracle, name, tol)
        n = len(vols)
        bs = _make(vr, n, shape, tol, ep).build(np.stack(vols))
        for b, ref in enumerate(refs):
            assert np.array_equal(bs.tree(b), ref.tree), (tol, b)
        cuts = _cuts(refs[0])
        _against(bs, vols, refs, cuts, (name, tol))
        lod = [cuts[(3 * b + tol) % len(cuts)] for b in range(n)]
        run = lambda: bs.decode_lod(np.array(lod, np.int32), out=bs.decode(cut_depth=0))
        got = run()
        assert (got == _with(bs, "no_uniform_decode", run)).all(), (name, tol)
        assert (got == _with(bs, "decode_quad", run)).all(), (name, tol)
        got = got.cpu().numpy().reshape((n,) + shape)
        for b, ref in enumerate(refs):
            assert np.array_equal(got[b], _want(ref, lod[b])), (name, tol, b, lod[b])


def _walks(region_kinds):
    """kind -> kind steps of every wave position over the regions a workgroup walks (128x64x64, 512 bricks: four
    workgroups per brick, workgroup i takes regions i, i + 4, i + 8, i + 12)"""
    dead = {"short": "dead", "one": "dead", "none": "dead", "brick": "dead"}
    steps = set()
    for brick in region_kinds:
        assert len(brick) == 16
        for i in range(4):
            for w in range(8):
                seq = [dead.get(brick[i + 4 * j][w], brick[i + 4 * j][w]) for j in range(4)]
                steps |= set(zip(seq, seq[1:]))
    return steps


def test_pipeline_across_regions(vr, oracle):
    """512 bricks of 128x64x64: a workgroup decodes four regions, one more than it has index slots, and a wave meets
    live uniform, busy and dead boxes in every order; the next region's requests are issued while the current one is
    decoded, so a miscounted wait of either path would show in the other's voxels."""
    import torch
    shape = SHAPES["128x64x64"]
    vols, refs, kinds, ep = _set(oracle, "128x64x64", 1)
    extra = np.ascontiguousarray(_by_rule(oracle, shape, 3, (1, 0, 3, 2, 4)))
    eref = _refs(oracle, [extra], 1, ep)[0]
    vols, refs, kinds = vols + [extra], refs + [eref], kinds + [_kinds(oracle, extra, eref)]
    assert len(vols) == 8
    steps = _walks(_region_kinds(oracle, shape, kinds))
    print("steps of a wave from region to region: %r" % sorted(steps))
    assert {("live", "busy"), ("busy", "live"), ("live", "dead"), ("dead", "live")} <= steps, sorted(steps)
    n = 512
    order = [(i + i // 8) % 8 for i in range(n)]
    dev = torch.from_numpy(np.stack(vols)).cuda()[torch.tensor(order, device="cuda")].contiguous()
    bs = _make(vr, n, shape, 1, ep).build(dev.reshape(-1))
    got = bs.decode()
    assert torch.equal(got, _with(bs, "no_uniform_decode", bs.decode))
    assert torch.equal(got, _with(bs, "decode_quad", bs.decode))
    got = got.reshape((n,) + shape)
    for b in range(8):
        assert order[b] == b
        assert np.array_equal(got[b].cpu().numpy(), refs[b].levelCut()), b
    # the rotated repeats equal their first copies
    first = got[:8]
    for i in range(8, n, 8):
        assert torch.equal(got[i:i + 8], first[torch.tensor(order[i:i + 8], device="cuda")]), i


def _three_cuts(bs, refs, vols, what):
    D, M = refs[0].origTreeDepth, refs[0].maxTreeDepth
    out = {}
    for cut in (M, D, D - 3):
        got = bs.decode(cut_depth=cut).cpu().numpy().reshape((len(vols),) + vols[0].shape)
        for b, ref in enumerate(refs):
            assert np.array_equal(got[b], _want(ref, cut)), (what, b, cut)
        out[cut] = got
    return out


def test_no_stale_flag(vr, oracle):
    """Rebuilds on one handle between sets whose boxes change kind: every build clears the flags of the one before.
    A: the tolerance-1 set; B: the same bricks one place on, so that every brick slot gets another volume."""
    shape = SHAPES["128x64x64"]
    A, RA, KA, ep = _set(oracle, "128x64x64", 1)
    B, RB, KB = A[1:] + A[:1], RA[1:] + RA[:1], KA[1:] + KA[:1]
    dead = {"short": "one", "none": "one", "brick": "one"}
    flips = {(dead.get(a[0], a[0]), dead.get(b[0], b[0])) for ka, kb in zip(KA, KB) for a, b in zip(ka, kb)}
    print("kinds of a box in A and in B: %r" % sorted(flips))
    assert {("live", "busy"), ("busy", "live"), ("live", "one"), ("one", "live"), ("busy", "one"), ("one", "busy")} <= flips, sorted(flips)
    sets = {"A": (A, RA), "B": (B, RB)}
    bs = _make(vr, len(A), shape, 1, ep)
    for name in "ABAB":
        V, R = sets[name]
        bs.build(np.stack(V))
        out = _three_cuts(bs, R, V, "rebuild " + name)
        fresh = _make(vr, len(V), shape, 1, ep).build(np.stack(V))
        for cut, got in out.items():
            assert np.array_equal(got, fresh.decode(cut_depth=cut).cpu().numpy().reshape(got.shape)), (name, cut)
    # A on the closed-form path, then B through k_prune_emit12 alone on the same handle: no box of B may read 1
    bs = _make(vr, len(A), shape, 1, ep).build(np.stack(A))
    _three_cuts(bs, RA, A, "A")
    bs.set_switch("no_uniform_blocks", 1)
    bs.build(np.stack(B))
    _three_cuts(bs, RB, B, "B with no_uniform_blocks after A")


def test_installed_stream_after_a_build(vr, oracle):
    """The oracle's stream of a brick of B against a handle that has just built A.  vr_brickset_set_tree installs
    streams into a fresh set only and refuses a built one (VR_ERR_STATE), so the flags of a build can never meet an
    installed stream: the refusal is asserted, the handle still decodes A, and the same stream installed into a
    fresh handle -- which has no flags -- decodes to the oracle's voxels at every cut of the kernel."""
    shape = SHAPES["128x64x64"]
    A, RA, KA, ep = _set(oracle, "128x64x64", 1)
    a, b = 0, 3
    assert any(x[0] == "live" and y[0] != "live" for x, y in zip(KA[a], KA[b]))
    bs = _make(vr, 1, shape, 1, ep).build(A[a])
    ref = RA[b]
    with pytest.raises(Exception):
        bs.set_tree(0, ref.tree, ref.numActiveNodes, ref.distanceMap)
    _three_cuts(bs, [RA[a]], [A[a]], "A after the refused install")
    fs = _make(vr, 1, shape, 1, ep)
    fs.set_tree(0, ref.tree, ref.numActiveNodes, ref.distanceMap)
    for cut in _cuts(ref):
        assert np.array_equal(fs.decode(cut_depth=cut).cpu().numpy().reshape(shape), _want(ref, cut)), cut


def test_midrange_tree_untouched(vr, oracle):
    """A MidRangeTree set (variant 2) at 128x64x64: no flag is written for either stream; decode and decode_range
    equal the oracle."""
    shape = SHAPES["128x64x64"]
    A, _, _, ep = _set(oracle, "128x64x64", 1)
    vols = [A[0], A[3], A[5]]
    refs = _refs(oracle, vols, 1, ep, midrange=True)
    bs = _make(vr, len(vols), shape, 1, ep, midrange=True).build(np.stack(vols))
    dec = bs.decode().cpu().numpy().reshape((len(vols),) + shape)
    rng = bs.decode_range().cpu().numpy().reshape((len(vols),) + shape)
    for b, ref in enumerate(refs):
        assert np.array_equal(bs.tree(b), ref.tree), b
        assert np.array_equal(dec[b], ref.levelCut()), b
        assert np.array_equal(rng[b], ref.levelCutRange()), b
