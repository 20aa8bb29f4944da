"""Constant 4096-leaf boxes in k_pyramid12 and the on-demand leaf fill (k_fill_const_leaves), against the CPU oracle,
a fresh handle and -- where stated -- the same build with `no_skip_blocks` on (the pyramid path that writes every byte).

With SkipBlocks on, a box whose 4096 voxels are one value leaves k_pyramid12 after its loads: levels D-12 .. D-2 get the
broadcast value, levels D-1 and D stay unwritten.  A box the level loop then skips (its depth-(D-2) truths equal their
parents' reconstruction) is never read there; every other constant box of a busy brick gets the two levels from
k_fill_const_leaves before level D-1 starts.  Everything the host can see must stay what it was: stream bytes,
distance map, info and decoded voxels are compared bit for bit.

Which class a box falls in -- constant brick, skipped, filled, busy -- is computed here from the oracle's own truth heap
and reconstruction (`_census`), and the cases assert that the classes they are about really occur.

Shapes are the smallest with the path: D >= 14 and four x splits among the bottom twelve levels."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

S14 = (16, 32, 32)          # (z, y, x): D = 14, 4 boxes
S15 = (32, 32, 32)          # D = 15, 8 boxes
S15W = (16, 32, 64)         # D = 15, x wider than y


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


# ---------------------------------------------------------------- geometry, read off the oracle's pyramid ----
_ORDER = {}


def _leaf_order(O, shape):
    """voxel index (x fastest) of every leaf rank of a `shape` brick"""
    if shape not in _ORDER:
        z, y, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
        idx = 0
        for c, mul in ((z, shape[1] * shape[2]), (y, shape[2]), (x, 1)):
            t = O.OracleTree(c.astype(np.uint8), tolerance=1, max_epochs=1).build(1)
            n = 1 << t.origTreeDepth
            idx = idx + np.asarray(t.temp)[n - 1:2 * n - 1].astype(np.int64) * mul
        assert np.array_equal(np.sort(idx), np.arange(idx.size))
        _ORDER[shape] = idx
    return _ORDER[shape]


def _from_leaves(O, leaves, shape):
    vol = np.empty(leaves.size, np.uint8)
    vol[_leaf_order(O, shape)] = leaves
    return vol.reshape(shape)


def _box_geom(O, shape, box):
    """(origin (x, y, z), extents (ex, ey, ez)) of the voxels under depth-(D-12) node `box`"""
    vi = _leaf_order(O, shape)[box * 4096:(box + 1) * 4096]
    x, y, z = vi % shape[2], (vi // shape[2]) % shape[1], vi // (shape[2] * shape[1])
    o = (int(x.min()), int(y.min()), int(z.min()))
    e = (int(x.max()) - o[0] + 1, int(y.max()) - o[1] + 1, int(z.max()) - o[2] + 1)
    assert e[0] * e[1] * e[2] == 4096 and e[0] >= 16
    return o, e


def _thread_voxel(O, shape, box, t, byte):
    """(z, y, x) of byte `byte` of the 16-byte x-run that thread `t` of the box's k_pyramid12 workgroup loads"""
    (ox, oy, oz), (ex, ey, ez) = _box_geom(O, shape, box)
    nxs = ex // 16
    xs, y, z = t % nxs, (t // nxs) % ey, t // (nxs * ey)
    assert z < ez
    return oz + z, oy + y, ox + xs * 16 + byte


def _census(O, vol, ref):
    """box classes of one brick: dict(constant_brick, skipped, filled, busy) -- numbers of 4096-leaf boxes"""
    D = ref.origTreeDepth
    nb = 1 << (D - 12)
    if int(vol.min()) == int(vol.max()):
        return dict(constant_brick=nb, skipped=0, filled=0, busy=0)
    leaves = vol.reshape(-1)[_leaf_order(O, vol.shape)].reshape(nb, 4096)
    const = (leaves == leaves[:, :1]).all(axis=1)
    # skipped: every depth-(D-2) truth of the box equals its parent's reconstruction; the truths are the box's value
    n3 = 1 << (D - 3)
    par = np.asarray(ref.recon_all)[n3 - 1:2 * n3 - 1].reshape(nb, 512)
    exact = (par == leaves[:, :1]).all(axis=1)
    return dict(constant_brick=0, skipped=int((const & exact).sum()), filled=int((const & ~exact).sum()),
                busy=int((~const).sum()))


def _add(a, b):
    return {k: a[k] + b[k] for k in a}


# ---------------------------------------------------------------- comparison ----
def _refs(O, vols, tol, ep, midrange=False):
    return [O.OracleTree(np.ascontiguousarray(v), tolerance=tol, max_epochs=ep, midrange=midrange).build() for v in vols]


def _outputs(bs, n, shape, midrange):
    out = dict(dec=bs.decode().cpu().numpy().reshape(n, *shape))
    if midrange:
        out["dec_range"] = bs.decode_range().cpu().numpy().reshape(n, *shape)
    for b in range(n):
        out["tree%d" % b] = bs.tree(b)
        out["dmap%d" % b] = bs.distance_map(b)
        info = bs.info(b)
        out["info%d" % b] = np.array([info[k] for k in sorted(info)], np.float64)
        if midrange:
            out["treeR%d" % b] = bs.tree_range(b)
            out["dmapR%d" % b] = bs.distance_map_range(b)
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, what)


def _against_oracle(bs, vols, refs, midrange, what):
    n, shape = len(vols), vols[0].shape
    out = _outputs(bs, n, shape, midrange)
    for b, ref in enumerate(refs):
        info = bs.info(b)
        assert list(out["dmap%d" % b]) == list(ref.distanceMap), (b, what)
        assert info["num_active_nodes"] == ref.numActiveNodes, (b, what)
        assert info["num_reverts"] == ref.numReverts, (b, what)
        assert np.array_equal(out["tree%d" % b], ref.tree), (b, what)
        assert np.array_equal(out["dec"][b], ref.levelCut()), (b, what)
        if midrange:
            assert list(out["dmapR%d" % b]) == list(ref.distanceMap_range), (b, what)
            assert np.array_equal(out["treeR%d" % b], ref.tree_range), (b, what)
            assert np.array_equal(out["dec_range"][b], ref.levelCutRange()), (b, what)
    return out


def _make(vr, n, shape, tol, ep, midrange=False, switches=(), concurrency=None):
    bs = vr.BrickSet(n, shape[::-1], tol, ep, variant=2) if midrange else vr.BrickSet(n, shape[::-1], tol, ep)
    for name in switches:
        bs.set_switch(name, 1)
    if concurrency is not None:
        bs.set_concurrency(concurrency)
    return bs


def _check(vr, O, vols, tol, ep, midrange=False, refs=None, old_path=True):
    """One fresh handle against the oracle and, with `old_path`, against a build with no_skip_blocks on."""
    vols = [np.ascontiguousarray(v) for v in vols]
    what = (tol, ep, midrange)
    refs = refs if refs is not None else _refs(O, vols, tol, ep, midrange)
    bs = _make(vr, len(vols), vols[0].shape, tol, ep, midrange).build(np.stack(vols))
    out = _against_oracle(bs, vols, refs, midrange, what)
    if old_path:
        off = _make(vr, len(vols), vols[0].shape, tol, ep, midrange, switches=("no_skip_blocks",)).build(np.stack(vols))
        _same(out, _outputs(off, len(vols), vols[0].shape, midrange), what)
    census = dict(constant_brick=0, skipped=0, filled=0, busy=0)
    for v, r in zip(vols, refs):
        census = _add(census, _census(O, v, r))
    print("boxes %r  %r" % (census, what))
    return refs, out, census


# ---------------------------------------------------------------- volumes ----
def _noise_box(rng, amp=12):
    """4096 leaves with structure at every scale: each of the twelve levels moves its nodes by up to +-amp, so the
    level distances stay well above 1 all the way down and a constant box beside it that starts a little off its
    value is not pulled onto it (plain noise has one midrange everywhere above the leaves: every distance above them
    drops to 1 and every constant box comes out exact)."""
    v = np.full(1, 128, np.int64)
    for _ in range(12):
        v = np.repeat(v, 2) + rng.integers(-amp, amp + 1, 2 * v.size)
    return np.clip(v, 0, 255)


def _mixed(O, shape, seed, values, busy=(0,)):
    """Boxes `busy` are noise, the others constant with values drawn from `values`."""
    rng = np.random.default_rng(seed)
    nb = shape[0] * shape[1] * shape[2] // 4096
    leaves = np.repeat(rng.choice(values, nb), 4096).reshape(nb, 4096)
    for b in busy:
        leaves[b] = _noise_box(rng)
    return _from_leaves(O, leaves.reshape(-1).astype(np.uint8), shape)


# values around the noise box's midrange: some constant boxes come out exact at depth D-3, others do not
MIX_VALUES = [128, 129, 130, 131, 90, 200, 0, 255]


def _mixed_set(O):
    """the mixed volume of the sweeps: S15 bricks with one or two busy boxes, and constant bricks between them"""
    return [_mixed(O, S15, 1, MIX_VALUES), np.full(S15, 8, np.uint8), _mixed(O, S15, 2, MIX_VALUES, busy=(3, 6)),
            _mixed(O, S15, 3, [128, 131]), np.full(S15, 247, np.uint8), _mixed(O, S15, 4, MIX_VALUES, busy=(7,))]


# ---------------------------------------------------------------- the cases ----
@pytest.mark.parametrize("shape", [S14, S15, S15W], ids=["32x32x16", "32x32x32", "64x32x16"])
def test_constant_bricks(vr, oracle, shape):
    """Constant bricks of 0, 1, 8, 247, 255, alone and between busy bricks: nothing reads their level arrays."""
    for v in (0, 1, 8, 247, 255):
        _, _, census = _check(vr, oracle, [np.full(shape, v, np.uint8)], 1, 2, old_path=False)
        assert census["constant_brick"] == shape[0] * shape[1] * shape[2] // 4096
    rng = np.random.default_rng(5)
    vols = []
    for v in (0, 1, 8, 247, 255):
        vols += [np.full(shape, v, np.uint8), rng.integers(0, 256, shape, dtype=np.uint8)]
    vols.append(_mixed(oracle, shape, 6, MIX_VALUES))
    _check(vr, oracle, vols, 1, 2)


@pytest.mark.parametrize("shape", [S14, S15, S15W], ids=["32x32x16", "32x32x32", "64x32x16"])
def test_one_busy_box_among_constant_ones(vr, oracle, shape):
    """Both classes of constant box in one set: reproduced exactly at depth D-3 (skipped) and not (filled)."""
    vols = [_mixed(oracle, shape, s, MIX_VALUES, busy=(b,)) for s, b in ((1, 0), (2, 1), (3, 3), (4, 2))]
    _, _, census = _check(vr, oracle, vols, 1, 2)
    assert census["skipped"] > 0 and census["filled"] > 0 and census["busy"] == len(vols), census


def _almost_positions(O, shape, box):
    """the deviating voxel: first and last byte of the box, a middle lane of each wave's x-runs, each wave's last lane"""
    pos = [_thread_voxel(O, shape, box, 0, 0), _thread_voxel(O, shape, box, 255, 15)]
    for w in range(4):
        pos.append(_thread_voxel(O, shape, box, 64 * w + 17, 5))
        pos.append(_thread_voxel(O, shape, box, 64 * w + 63, 15))
        pos.append(_thread_voxel(O, shape, box, 64 * w + 63, 0))
    return pos


@pytest.mark.parametrize("shape,box", [(S14, 2), (S15, 5), (S15W, 0)], ids=["32x32x16", "32x32x32", "64x32x16"])
def test_almost_constant_box(vr, oracle, shape, box):
    """A constant box with one voxel off by 1 must take the full path: wherever the voxel sits, the build equals the
    oracle's of THAT volume -- and, checked here on the oracle, differs from the all-constant one's, so a box taken
    for constant would show."""
    base = _mixed(oracle, shape, 11, [100, 101, 103, 140], busy=())
    v = int(base[_thread_voxel(oracle, shape, box, 0, 0)])
    base[base == v] = 100        # (the box under test, and any other of its value)
    const_ref = _refs(oracle, [base], 1, 2)[0]
    vols = []
    for p in _almost_positions(oracle, shape, box):
        for delta in (-1, 1):
            vol = base.copy()
            vol[p] = 100 + delta
            vols.append(vol)
    refs = _refs(oracle, vols, 1, 2)
    differ = sum(not (np.array_equal(r.tree, const_ref.tree) and np.array_equal(r.levelCut(), const_ref.levelCut())) for r in refs)
    print("almost-constant volumes whose oracle result differs from the constant one's: %d of %d" % (differ, len(refs)))
    assert differ >= len(refs) // 2
    _, _, census = _check(vr, oracle, vols, 1, 2, refs=refs)
    assert census["busy"] == len(vols), census


def test_rebuilds_on_one_handle(vr, oracle):
    """A, B, A on one handle: boxes flip between constant, skipped, filled and busy, bricks between constant and not.
    Every rebuild equals a fresh handle and the oracle: a stale byte of an unwritten level would show here."""
    A = _mixed_set(oracle)
    B = [np.full(S15, 8, np.uint8), _mixed(oracle, S15, 21, MIX_VALUES, busy=(5,)), np.full(S15, 131, np.uint8),
         np.random.default_rng(22).integers(0, 256, S15, dtype=np.uint8), _mixed(oracle, S15, 23, [90, 200], busy=(0, 1)),
         _mixed(oracle, S15, 24, [128, 129], busy=())]
    sets = {"A": (A, _refs(oracle, A, 1, 2)), "B": (B, _refs(oracle, B, 1, 2))}
    for name, (V, R) in sets.items():
        census = dict(constant_brick=0, skipped=0, filled=0, busy=0)
        for v, r in zip(V, R):
            census = _add(census, _census(oracle, v, r))
        print("boxes %s %r" % (name, census))
        assert all(census[k] > 0 for k in census), (name, census)
    bs = _make(vr, len(A), S15, 1, 2)
    for name in "ABAB":
        V, R = sets[name]
        bs.build(np.stack(V))
        out = _against_oracle(bs, V, R, False, "rebuild " + name)
        fresh = _make(vr, len(V), S15, 1, 2).build(np.stack(V))
        _same(out, _outputs(fresh, len(V), S15, False), "rebuild %s against a fresh handle" % name)


@pytest.mark.parametrize("shape", [S14, S15], ids=["32x32x16", "32x32x32"])
def test_midrange_tree(vr, oracle, shape):
    """Variant 2: both streams' bytes and distance maps, decode and decode_range; the half-range stream of a
    constant box is 0 at every level and takes the same pyramid path and its own fill."""
    vols = [_mixed(oracle, shape, s, MIX_VALUES, busy=(b,)) for s, b in ((1, 0), (2, 1), (3, 3))] + [np.full(shape, 8, np.uint8)]
    _, _, census = _check(vr, oracle, vols, 1, 2, midrange=True)
    assert census["skipped"] > 0 and census["filled"] > 0, census
    bs = _make(vr, len(vols), shape, 1, 2, midrange=True)
    refs = _refs(oracle, vols, 1, 2, midrange=True)
    for V, R in ((vols, refs), (vols[::-1], refs[::-1]), (vols, refs)):      # and rebuilt on one handle
        bs.build(np.stack(V))
        _against_oracle(bs, V, R, True, "midrange rebuild")


@pytest.fixture(scope="module")
def sixty_four(oracle):
    rng = np.random.default_rng(31)
    vols = []
    for b in range(64):
        kind = b % 4
        if kind == 0:
            vols.append(np.full(S14, int(rng.integers(0, 256)), np.uint8))
        elif kind == 3:
            vols.append(rng.integers(0, 256, S14, dtype=np.uint8))
        else:
            vols.append(_mixed(oracle, S14, 100 + b, MIX_VALUES, busy=(b % 4,)))
    return vols, _refs(oracle, vols, 1, 2)


@pytest.mark.parametrize("streams", [1, 2, 4])
def test_set_concurrency(vr, oracle, sixty_four, streams):
    """64 bricks of 32x32x16 (a range needs 16 bricks to fork): the fill runs per brick range on the range's stream."""
    vols, refs = sixty_four
    bs = _make(vr, 64, S14, 1, 2, concurrency=streams).build(np.stack(vols))
    out = _against_oracle(bs, vols, refs, False, streams)
    one = _make(vr, 64, S14, 1, 2, concurrency=1).build(np.stack(vols))
    _same(out, _outputs(one, 64, S14, False), streams)
    census = dict(constant_brick=0, skipped=0, filled=0, busy=0)
    for v, r in zip(vols, refs):
        census = _add(census, _census(oracle, v, r))
    assert all(census[k] > 0 for k in census), census


@pytest.mark.parametrize("tol", [1, 2])
@pytest.mark.parametrize("ep", [1, 2, 3])
def test_tolerance_epoch_sweep(vr, oracle, tol, ep):
    """The mixed volume under tolerance {1, 2} x max_epochs {1, 2, 3}: reverted epochs included."""
    vols = _mixed_set(oracle)
    _, _, census = _check(vr, oracle, vols, tol, ep)
    assert census["filled"] > 0 and census["busy"] > 0 and census["constant_brick"] > 0, census
