"""GPU parity of the level loop's lane-uniform fast paths (k_fill16: one pair per lane, replicated; k_est_summ: the
candidate chains in closed form) against the CPU oracle: tree bytes, distanceMap, numActiveNodes, reverts and decoded
voxels, bit for bit.

A wave takes the fast path when every lane's run of consecutive nodes (16 in k_fill16, 32 in k_est_summ) has one truth
value and one parent-reconstruction value, and some truth differs from its parent's reconstruction (otherwise the older
exact shortcut takes it).  Whether a case gets there is decided here BY CONSTRUCTION OF THE INPUT, and the
construction is checked rather than trusted: `_fast_path_waves` counts such waves from the oracle's own truth heap and
reconstruction (which the GPU build reproduces bit for bit), with the kernels' wave geometry -- 1024 consecutive nodes
per k_fill16 wave on levels >= 12, two 1024-node segments per k_est_summ wave from node 4096 on.  The cases of constant
16^3 blocks (the first three: block roots off by 1, by the tolerance, by a large amount), the clamp values, the run
patterns and the mixed set assert a non-zero count for both kernels.  The two-constant plane bricks cannot: their
mixed nodes all have the midrange as truth, so every pure node's parent is exact but for one rounding step and the
level after it is exact again -- long before level 12.  They pin the exact shortcut beside block boundaries."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SHAPE = (64, 64, 64)        # depth 18: levels 12 .. 18 run k_fill16, 13 .. 18 k_est_summ; 64 blocks of 4096 leaves


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _fast_path_waves(O, vol, ref):
    """(k_fill16 waves, k_est_summ waves) that are lane-uniform in every lane and not exact, summed over the levels."""
    D = ref.origTreeDepth
    temp = np.asarray(O.OracleTree(vol.copy(), tolerance=1, max_epochs=1).build(1).temp)      # the pyramid: every level's truths
    recon = np.asarray(ref.recon_all)
    assert temp.size == recon.size == (2 << D) - 1
    fill = est = 0
    for d in range(12, D + 1):
        n = 1 << d
        t = temp[n - 1:2 * n - 1].astype(np.int16)
        p = np.repeat(recon[n // 2 - 1:n - 1].astype(np.int16), 2)

        def waves(lo, lane):
            tt, pp = t[lo:].reshape(-1, 64, lane), p[lo:].reshape(-1, 64, lane)
            uni = ((tt == tt[:, :, :1]) & (pp == pp[:, :, :1])).all(axis=(1, 2))
            return int((uni & (tt != pp).any(axis=(1, 2))).sum())

        fill += waves(0, 16)
        if n > 4096:
            est += waves(4096, 32)
    return fill, est


def _check(vr, O, vol, tol, ep, switches=(), midrange=False, fast=True):
    z, y, x = vol.shape
    ref = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep, midrange=midrange).build()
    bs = vr.BrickSet(1, (x, y, z), tol, ep, variant=2) if midrange else vr.BrickSet(1, (x, y, z), tol, ep)
    for name in switches:
        bs.set_switch(name, 1)
    bs.build(vol.copy())
    info, what = bs.info(0), (tol, ep, switches, midrange)
    fill, est = _fast_path_waves(O, vol, ref)
    print("fast-path waves: k_fill16 %d, k_est_summ %d  %r" % (fill, est, what))
    if fast:
        assert fill > 0 and est > 0, what
    assert list(bs.distance_map(0)) == list(ref.distanceMap), what
    assert info["num_active_nodes"] == ref.numActiveNodes, what
    assert np.array_equal(bs.tree(0), ref.tree), what
    assert info["num_reverts"] == ref.numReverts, what
    assert np.array_equal(bs.decode().cpu().numpy().reshape(vol.shape), ref.levelCut()), what
    if midrange:
        assert list(bs.distance_map_range(0)) == list(ref.distanceMap_range), what
        assert np.array_equal(bs.tree_range(0), ref.tree_range), what
    return ref, bs


def _boxes(lv):
    return np.repeat(np.repeat(np.repeat(lv, 16, 0), 16, 1), 16, 2).astype(np.int64)


def _blocks(rng, base, others, spikes=60, spike=37):
    """64 constant 16^3 blocks: `base`, a third of them drawn from `others`, and `spikes` single voxels moved by
    `spike`: the nodes above them keep the level distances away from what would make the constant blocks exact, and
    cost one lane of a wave each."""
    lv = np.full((4, 4, 4), base, np.int64)
    pick = rng.random(lv.shape) < 0.34
    lv[pick] = rng.choice(others, int(pick.sum()))
    vol = _boxes(lv).reshape(-1)
    at = rng.choice(vol.size, spikes, replace=False)
    vol[at] += np.where(vol[at] > 127, -spike, spike)
    return np.clip(vol, 0, 255).astype(np.uint8).reshape(SHAPE)


def _leaf_order(O):
    """voxel index (x fastest) of every leaf rank of a SHAPE brick, read off the oracle's pyramid of coordinate bricks"""
    z, y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), np.arange(SHAPE[2]), indexing="ij")
    idx = 0
    for c, mul in ((z, SHAPE[1] * SHAPE[2]), (y, SHAPE[2]), (x, 1)):
        t = O.OracleTree(c.astype(np.uint8), tolerance=1, max_epochs=1).build(1)
        n = 1 << t.origTreeDepth
        idx = idx + np.asarray(t.temp)[n - 1:2 * n - 1].astype(np.int64) * mul
    assert np.array_equal(np.sort(idx), np.arange(idx.size))
    return idx


def _from_leaves(O, leaves):
    vol = np.empty(leaves.size, np.uint8)
    vol[_leaf_order(O)] = leaves
    return vol.reshape(SHAPE)


# ---- constant blocks whose block-root reconstruction misses by 1, by the tolerance, by a large amount ----
@pytest.mark.parametrize("delta", [1, 3, 120], ids=["off_by_1", "off_by_tolerance", "off_by_large"])
def test_constant_blocks_inexact(vr, oracle, delta):
    rng = np.random.default_rng({1: 0, 3: 3, 120: 2}[delta])      # seeds under which _fast_path_waves finds waves
    _check(vr, oracle, _blocks(rng, 100, [100 + delta, 100 - delta if delta < 100 else 100 + delta // 2]), 3, 2)


@pytest.mark.parametrize("plane", [16, 32, 5, 41], ids=lambda p: "z%d" % p)
def test_two_constants_split_by_a_plane(vr, oracle, plane):
    """Plane on a block boundary (16, 32) and inside the blocks (5, 41): exact shortcut and mixed waves side by side."""
    vol = np.full(SHAPE, 40, np.uint8)
    vol[plane:] = 201
    _check(vr, oracle, vol, 1, 2, fast=False)
    _check(vr, oracle, np.ascontiguousarray(vol.transpose(2, 1, 0)), 1, 2, fast=False)


def test_clamp_values(vr, oracle):
    """Blocks of 0, 1, 254, 255: h = 0 or 1, the clamp decides (forced counts, steps cut short)."""
    for base, seed in ((0, 0), (1, 2), (254, 2), (255, 0)):
        _check(vr, oracle, _blocks(np.random.default_rng(seed), base, [0, 1, 254, 255]), 1, 2)


def test_every_second_run_constant(vr, oracle):
    """Lane-uniform lanes beside noisy ones in every wave (every second 16-leaf run is noise): no wave may branch.  The
    other half of the brick is constant blocks, which do."""
    rng = np.random.default_rng(21)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    leaves = np.repeat(rng.integers(90, 111, n // 4096), 4096)
    leaves[n // 2 + rng.choice(n // 2, 40, replace=False)] += 37        # (spikes, as in _blocks)
    runs = leaves[:n // 2].reshape(-1, 2, 16)
    runs[:, 1, :] = rng.integers(60, 140, (runs.shape[0], 16))
    _check(vr, oracle, _from_leaves(oracle, leaves.astype(np.uint8)), 1, 2)


def test_one_non_uniform_lane(vr, oracle):
    """Constant blocks; in some waves of the leaf level exactly one lane's run holds one different voxel."""
    rng = np.random.default_rng(22)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    leaves = np.repeat(rng.integers(90, 111, n // 4096), 4096)
    for w in rng.choice(n // 1024, 40, replace=False):
        leaves[w * 1024 + 16 * int(rng.integers(0, 64)) + int(rng.integers(0, 16))] += 37
    _check(vr, oracle, _from_leaves(oracle, leaves.astype(np.uint8)), 1, 2)


@pytest.mark.parametrize("tol", [0, 1, 3])
@pytest.mark.parametrize("ep", [1, 2, 3])
def test_tolerance_epoch_sweep(vr, oracle, tol, ep):
    rng = np.random.default_rng({1: 0, 2: 4, 3: 5}[ep])
    _check(vr, oracle, _blocks(rng, 120, [100, 119, 121, 124, 200]), tol, ep)


def test_skip_blocks_on_and_off(vr, oracle):
    rng = np.random.default_rng(4)
    vol = _blocks(rng, 100, [99, 101, 104, 30])
    _, on = _check(vr, oracle, vol, 1, 2)
    _, off = _check(vr, oracle, vol, 1, 2, switches=("no_skip_blocks",))
    assert np.array_equal(on.tree(0), off.tree(0))


def test_midrange_tree(vr, oracle):
    rng = np.random.default_rng(4)
    _check(vr, oracle, _blocks(rng, 100, [99, 101, 104, 30]), 1, 2, midrange=True)


def test_mixed_set(vr, oracle):
    """Constant, constant-block, uniform-run and noisy bricks in one set: each matches its own oracle tree."""
    rng = np.random.default_rng(77)
    n = SHAPE[0] * SHAPE[1] * SHAPE[2]
    leaves = np.repeat(rng.integers(0, 256, n // 16), 16)
    vols = [np.full(SHAPE, 77, np.uint8), _blocks(rng, 100, [99, 103, 220]), _from_leaves(oracle, leaves.astype(np.uint8)),
            rng.integers(0, 256, SHAPE, dtype=np.uint8), _blocks(rng, 254, [255, 0, 250])]
    bs = vr.BrickSet(len(vols), SHAPE[::-1], 1, 2)
    bs.build(np.stack(vols))
    dec = bs.decode().cpu().numpy().reshape(len(vols), *SHAPE)
    fast = [0, 0]
    for b, v in enumerate(vols):
        ref = oracle.OracleTree(v.copy(), tolerance=1, max_epochs=2).build()
        f = _fast_path_waves(oracle, v, ref)
        fast = [fast[0] + f[0], fast[1] + f[1]]
        assert list(bs.distance_map(b)) == list(ref.distanceMap), b
        assert bs.info(b)["num_active_nodes"] == ref.numActiveNodes, b
        assert bs.info(b)["num_reverts"] == ref.numReverts, b
        assert np.array_equal(bs.tree(b), ref.tree), b
        assert np.array_equal(dec[b], ref.levelCut()), b
    print("fast-path waves: k_fill16 %d, k_est_summ %d" % tuple(fast))
    assert fast[0] > 0 and fast[1] > 0
