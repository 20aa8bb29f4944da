"""GPU parity of the estimator's first round (k_est_summ<true>: byte-packed quads of nodes, exact sums, SUFFICIENT
bounds A' >= A and B' <= B; k_est_walk's budget of node-by-node segments) against the CPU oracle and against the exact
first round (switch est_exact_bounds).

The records only steer which segments the exact walk visits, so a wrong sum or an insufficient bound shows up as a wrong
distance on some level: tree bytes, distanceMap, numActiveNodes, reverts and decoded voxels are compared bit for bit, with
the oracle and between the two paths.  The cases aim at what the quad path adds: the byte compare's high bit (pd >= 128),
forced nodes in most lanes (truths at 0-5 and 250-255), thresholds that drift through several windows, skipped constant
boxes beside busy ones, and a brick whose running mean sits on a threshold boundary for a whole level, on which the
budget has to trip.  est_exact_segments (segments walked node by node) must stay within the exact path's count plus the
budget per estimator level wherever the data are not built to defeat the bounds."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

BUDGET = 8                  # EST_R0_BUDGET (csrc/brickset.h)
PAIRS = [(0, 1), (1, 2), (3, 2), (6, 4)]
SHAPES = [(32, 32, 32), (64, 64, 64), (128, 64, 64)]


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _depth(shape):
    return int(np.log2(shape[0] * shape[1] * shape[2]))


def _est_levels(shape):
    """Levels the segment summaries serve: those with more than 4096 nodes."""
    return max(0, _depth(shape) - 12)


def _total_segments(shape):
    return sum((1 << d) // 1024 - 4 for d in range(13, _depth(shape) + 1))


def _build(vr, vol, tol, ep, exact):
    z, y, x = vol.shape
    bs = vr.BrickSet(1, (x, y, z), tol, ep)
    if exact:
        bs.set_switch("est_exact_bounds", 1)
    bs.build(vol.copy())
    return bs


def _same(a, b, what):
    ia, ib = a.info(0), b.info(0)
    assert list(a.distance_map(0)) == list(b.distance_map(0)), what
    assert ia["num_active_nodes"] == ib["num_active_nodes"], what
    assert ia["num_reverts"] == ib["num_reverts"], what
    assert np.array_equal(a.tree(0), b.tree(0)), what
    assert np.array_equal(a.decode().cpu().numpy(), b.decode().cpu().numpy()), what


def _check(vr, O, vol, tol, ep, adversarial=False):
    """Oracle parity of the quad path, byte identity with the exact path, and the walked-segment counts (new, exact)."""
    what = (vol.shape, tol, ep)
    ref = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep).build()
    new, old = _build(vr, vol, tol, ep, False), _build(vr, vol, tol, ep, True)
    info = new.info(0)
    assert list(new.distance_map(0)) == list(ref.distanceMap), what
    assert info["num_active_nodes"] == ref.numActiveNodes, what
    assert np.array_equal(new.tree(0), ref.tree), what
    assert info["num_reverts"] == ref.numReverts, what
    assert np.array_equal(new.decode().cpu().numpy().reshape(vol.shape), ref.levelCut()), what
    _same(new, old, what)
    n, e = info["est_exact_segments"], old.info(0)["est_exact_segments"]
    print("est_exact_segments %r: quads %d, exact bounds %d" % (what, n, e))
    assert 0 <= n <= _total_segments(vol.shape), what          # finite: no segment is walked twice
    if not adversarial:
        assert n <= e + BUDGET * _est_levels(vol.shape), what
    return n, e


def _drift(rng, shape, amps):
    """Slabs of very different noise amplitude: the threshold leaves the candidate windows inside a level."""
    z = shape[0]
    amp = np.array(amps * (z // len(amps) + 1))[:z]
    rng.shuffle(amp)
    vol = np.zeros(shape, np.int64) + 128
    for i in range(z):
        if amp[i]:
            vol[i] += rng.integers(-amp[i] // 2, amp[i] // 2 + 1, shape[1:])
    return np.clip(vol, 0, 255).astype(np.uint8)


def _blocky(rng, shape, busy):
    """Constant 16^3 boxes (SkipBlocks passes over them) with a fraction `busy` of noisy ones."""
    z, y, x = shape
    lv = rng.integers(0, 256, (z // 16, y // 16, x // 16))
    vol = np.repeat(np.repeat(np.repeat(lv, 16, 0), 16, 1), 16, 2).astype(np.int64)
    noisy = rng.random(lv.shape) < busy
    mask = np.repeat(np.repeat(np.repeat(noisy, 16, 0), 16, 1), 16, 2)
    vol = np.where(mask, vol + rng.integers(-30, 31, shape), vol)
    return np.clip(vol, 0, 255).astype(np.uint8)


def _saturated(rng, shape, stray):
    lo_hi = np.where(rng.random(shape) < 0.5, rng.integers(0, 6, shape), rng.integers(250, 256, shape))
    return np.where(rng.random(shape) < stray, rng.integers(0, 256, shape), lo_hi).astype(np.uint8)


@pytest.mark.parametrize("shape", SHAPES)
def test_drifting_threshold(vr, oracle, shape):
    rng = np.random.default_rng(shape[0] + 1)
    _check(vr, oracle, _drift(rng, shape, [0, 60, 2, 120, 0, 8, 200, 1, 30]), 1, 2)


@pytest.mark.parametrize("tol,ep", PAIRS)
def test_tolerance_epoch_pairs(vr, oracle, tol, ep):
    rng = np.random.default_rng(200 + 10 * tol + ep)
    _check(vr, oracle, _drift(rng, (64, 64, 64), [0, 90, 4, 160, 1, 12]), tol, ep)


@pytest.mark.parametrize("shape", SHAPES)
def test_truths_near_0_and_255(vr, oracle, shape):
    """Forced nodes (pd > h) in most lanes: the any-forced slack of A and the forced bit of the indicator."""
    rng = np.random.default_rng(shape[0] + 2)
    _check(vr, oracle, _saturated(rng, shape, 0.05), 1, 2)


@pytest.mark.parametrize("shape", SHAPES)
def test_random_bytes_pd_above_127(vr, oracle, shape):
    """Uniform random bytes: pd >= 128 in many nodes, the high bit of the byte compare."""
    rng = np.random.default_rng(shape[0] + 3)
    _check(vr, oracle, rng.integers(0, 256, shape, dtype=np.uint8), 1, 2)


@pytest.mark.parametrize("shape,pair", [((32, 32, 32), (0, 1)), ((64, 64, 64), (3, 2)), ((128, 64, 64), (1, 2))])
def test_two_valued_1_254(vr, oracle, shape, pair):
    rng = np.random.default_rng(shape[0] + 4)
    _check(vr, oracle, np.where(rng.random(shape) < 0.5, 1, 254).astype(np.uint8), *pair)


@pytest.mark.parametrize("shape,busy", [((64, 64, 64), 0.2), ((64, 64, 64), 0.8), ((128, 64, 64), 0.5)])
def test_constant_boxes_beside_noisy_ones(vr, oracle, shape, busy):
    rng = np.random.default_rng(int(busy * 100) + shape[0])
    _check(vr, oracle, _blocky(rng, shape, busy), 1, 2)


def test_five_bricks_in_one_set(vr, oracle):
    rng = np.random.default_rng(78)
    shape = (64, 64, 64)
    vols = [_drift(rng, shape, [0, 60, 2, 120, 0, 8, 200, 1]), _blocky(rng, shape, 0.3),
            np.where(rng.random(shape) < 0.5, 1, 254).astype(np.uint8), rng.integers(0, 256, shape, dtype=np.uint8),
            _saturated(rng, shape, 0.1)]
    sets = []
    for exact in (False, True):
        bs = vr.BrickSet(len(vols), shape[::-1], 1, 2)
        if exact:
            bs.set_switch("est_exact_bounds", 1)
        bs.build(np.stack(vols))
        sets.append(bs)
    new, old = sets
    dec, dec_old = (s.decode().cpu().numpy().reshape(len(vols), *shape) for s in sets)
    assert np.array_equal(dec, dec_old)
    for b, v in enumerate(vols):
        ref = oracle.OracleTree(v.copy(), tolerance=1, max_epochs=2).build()
        for s in sets:
            assert list(s.distance_map(b)) == list(ref.distanceMap), b
            assert s.info(b)["num_active_nodes"] == ref.numActiveNodes, b
            assert s.info(b)["num_reverts"] == ref.numReverts, b
            assert np.array_equal(s.tree(b), ref.tree), b
        assert np.array_equal(dec[b], ref.levelCut()), b
        n, e = new.info(b)["est_exact_segments"], old.info(b)["est_exact_segments"]
        print("brick %d est_exact_segments: quads %d, exact bounds %d" % (b, n, e))
        assert 0 <= n <= e + BUDGET * _est_levels(shape), b


def _leaf_order(O, shape):
    """Flat voxel index of every leaf, in the order of the leaf level: read from the oracle's truth heap of three
    volumes that hold the voxel's own coordinates."""
    z, y, x = shape
    grids = np.meshgrid(np.arange(z), np.arange(y), np.arange(x), indexing="ij")
    coords = []
    for g in grids:
        t = O.OracleTree(g.astype(np.uint8), tolerance=0, max_epochs=1).build()
        coords.append(np.array(t.temp, np.int64))
    flat = (coords[0] * y + coords[1]) * x + coords[2]
    assert np.array_equal(np.sort(flat), np.arange(z * y * x))
    return flat


def test_mean_on_a_threshold_boundary_trips_the_budget(vr, oracle):
    """Leaves 128 -+ a in sibling pairs, a = 9, 7, 9, 7, ... in leaf order: every parent is reproduced exactly (128), the
    leaf level's pd runs 9, 9, 7, 7 and every node counts, so S - 8 C runs +1, +2, +1, 0 around its value s0 at the
    period's start.  floor(S / (2C + 1)) >= 4 <=> S - 8 C >= 4: one pair with a = 8 in place of a 7 at the very start
    makes s0 = 2, and the threshold alternates between 3 and 4 inside EVERY segment of the level.  No hypothesis holds
    over a whole segment, so the exact first round walks all of them (its window, [T - 1, T + 2], never loses a
    threshold of 3 or 4; the levels above have pd = 0 throughout and walk nothing).  The quad path fails wherever the
    exact one does, so its first round must run out of budget; the result still has to be the oracle's."""
    shape = (64, 64, 64)
    order = _leaf_order(oracle, shape)
    n = order.size
    a = np.where((np.arange(n // 2) & 1) == 0, 9, 7)
    a[1] = 8
    leaves = np.empty(n, np.int64)
    leaves[0::2] = 128 - a
    leaves[1::2] = 128 + a
    vol = np.empty(n, np.uint8)
    vol[order] = leaves
    new, exact = _check(vr, oracle, vol.reshape(shape), 1, 2, adversarial=True)
    assert exact > BUDGET + 1          # more true failures in the first round than the budget: the quad path trips
