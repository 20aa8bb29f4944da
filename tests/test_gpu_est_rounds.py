"""GPU parity of the estimator's round plan (est_round_plan: prefix rounds that end inside a level, a one-candidate
bulk round, quad records in every round in front of the exact ones, one budget of node-by-node segments per brick and
level) against the CPU oracle, against the same data built with exact records (switch est_exact_bounds) and against the
old schedule (switch est_old_schedule: every round over the whole level).

The plan only steers which segments the exact walk visits and under which hypothesis, so a guard that looks past a
round's limit, a stale record or stale control state shows up as a wrong start distance on some level: tree bytes,
distanceMap, numActiveNodes, reverts and decoded voxels are compared bit for bit.  The volumes of est_rounds_cases have
their threshold changes at known segments of the leaf level (tests/test_est_round_plan.py asserts that on the oracle's
side): none, one inside the first prefix round, one in the last segment of a round, in the first of the next and one
further on, monotone drifts with more changes than rounds, and a mean on a threshold boundary, on which the level's
budget has to trip.  est_exact_segments (segments walked node by node) must stay within the exact records' count plus
the budget per estimator level wherever the data are not built to defeat the bounds; every case prints both counts."""
import numpy as np
import pytest

import est_rounds_cases as EC

pytestmark = pytest.mark.gpu

BUDGET = 8                  # EST_QUAD_BUDGET (csrc/brickset.h)
S64, S128 = (64, 64, 64), (128, 64, 64)


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


_ORDER = {}


def _order(O, shape):
    if shape not in _ORDER:
        _ORDER[shape] = EC.leaf_order(O, shape)
    return _ORDER[shape]


def _depth(shape):
    return int(np.log2(shape[0] * shape[1] * shape[2]))


def _est_levels(shape):
    return max(0, _depth(shape) - 12)


def _total_segments(shape):
    return sum((1 << d) // 1024 - 4 for d in range(13, _depth(shape) + 1))


def _build(vr, vol, tol, ep, switch=None, variant=None):
    z, y, x = vol.shape
    bs = vr.BrickSet(1, (x, y, z), tol, ep) if variant is None else vr.BrickSet(1, (x, y, z), tol, ep, variant)
    if switch:
        bs.set_switch(switch, 1)
    bs.build(vol.copy())
    return bs


def _same(a, b, what):
    ia, ib = a.info(0), b.info(0)
    assert list(a.distance_map(0)) == list(b.distance_map(0)), what
    assert ia["num_active_nodes"] == ib["num_active_nodes"], what
    assert ia["num_reverts"] == ib["num_reverts"], what
    assert np.array_equal(a.tree(0), b.tree(0)), what
    assert np.array_equal(a.decode().cpu().numpy(), b.decode().cpu().numpy()), what


def _check(vr, O, vol, tol=1, ep=2, adversarial=False):
    what = (vol.shape, tol, ep)
    ref = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep).build()
    new, exact, old = _build(vr, vol, tol, ep), _build(vr, vol, tol, ep, "est_exact_bounds"), _build(vr, vol, tol, ep, "est_old_schedule")
    info = new.info(0)
    assert list(new.distance_map(0)) == list(ref.distanceMap), what
    assert info["num_active_nodes"] == ref.numActiveNodes, what
    assert np.array_equal(new.tree(0), ref.tree), what
    assert info["num_reverts"] == ref.numReverts, what
    assert np.array_equal(new.decode().cpu().numpy().reshape(vol.shape), ref.levelCut()), what
    _same(new, exact, what)
    _same(new, old, what)
    n, e, o = info["est_exact_segments"], exact.info(0)["est_exact_segments"], old.info(0)["est_exact_segments"]
    print("est_exact_segments %r: round plan %d, exact records %d, old schedule %d" % (what, n, e, o))
    assert 0 <= n <= _total_segments(vol.shape), what          # finite: no segment is walked twice
    if not adversarial:
        assert n <= e + BUDGET * _est_levels(vol.shape), what
    return n, e


def _noise_slabs(rng, shape, amps):
    z = shape[0]
    amp = np.array(amps * (z // len(amps) + 1))[:z]
    rng.shuffle(amp)
    vol = np.zeros(shape, np.int64) + 128
    for i in range(z):
        if amp[i]:
            vol[i] += rng.integers(-amp[i] // 2, amp[i] // 2 + 1, shape[1:])
    return np.clip(vol, 0, 255).astype(np.uint8)


def _blocky(rng, shape, busy):
    z, y, x = shape
    lv = rng.integers(0, 256, (z // 16, y // 16, x // 16))
    vol = np.repeat(np.repeat(np.repeat(lv, 16, 0), 16, 1), 16, 2).astype(np.int64)
    mask = np.repeat(np.repeat(np.repeat(rng.random(lv.shape) < busy, 16, 0), 16, 1), 16, 2)
    vol = np.where(mask, vol + rng.integers(-30, 31, shape), vol)
    return np.clip(vol, 0, 255).astype(np.uint8)


def _saturated(rng, shape, stray):
    lo_hi = np.where(rng.random(shape) < 0.5, rng.integers(0, 6, shape), rng.integers(250, 256, shape))
    return np.where(rng.random(shape) < stray, rng.integers(0, 256, shape), lo_hi).astype(np.uint8)


def _paired(O, shape, a):
    return EC.paired_volume(shape, _order(O, shape), a)


# ---------------------------------------------------------------- known trajectories ----
@pytest.mark.parametrize("shape", [S64, S128])
def test_constant_threshold(vr, oracle, shape):
    n, e = _check(vr, oracle, _paired(oracle, shape, EC.constant(shape[0] * shape[1] * shape[2] // 2)))
    assert e == 0


@pytest.mark.parametrize("where", ["prefix", "l0-1", "l0", "l0+1", "l1-1", "l1", "l1+1", "end"])
@pytest.mark.parametrize("shape", [S64, S128])
def test_one_change_at_a_known_segment(vr, oracle, shape, where):
    """The threshold goes from 4 to 5 once: inside the first prefix round, around both round limits (on 128x64x64 they
    are 35 and 131: inside a walk step of 256 segments, and at every place of a lane's group of four) and near the end."""
    (l0, l1), nseg = EC.limits(_depth(shape))
    seg = {"prefix": 10, "l0-1": l0 - 1, "l0": l0, "l0+1": l0 + 1, "l1-1": l1 - 1, "l1": l1, "l1+1": l1 + 1, "end": nseg - 2}[where]
    n, e = _check(vr, oracle, _paired(oracle, shape, EC.one_change(shape[0] * shape[1] * shape[2] // 2, seg)))
    assert e >= 1


@pytest.mark.parametrize("first,then", [(9, 40), (40, 22)], ids=["up", "down"])
@pytest.mark.parametrize("shape", [S64, S128])
def test_monotone_drift(vr, oracle, shape, first, then):
    """More threshold changes than rounds, the last of them in the bulk: the exact rounds walk a remainder."""
    _check(vr, oracle, _paired(oracle, shape, EC.drift(shape[0] * shape[1] * shape[2] // 2, first, then)))


def test_mean_on_a_threshold_boundary_trips_the_budget(vr, oracle):
    """No hypothesis holds over a whole segment of the leaf level: the quad rounds give up and the exact rounds finish the
    brick.  Every segment fails under exact records too and is walked once in whichever round reaches it, so the count
    says nothing about WHICH budget tripped: that is test_false_alarms_spend_one_budget_per_level's business."""
    shape = S64
    new, exact = _check(vr, oracle, _paired(oracle, shape, EC.boundary(shape[0] * shape[1] * shape[2] // 2)), adversarial=True)
    assert exact > BUDGET + 1
    assert new <= exact + BUDGET + 1          # the quad rounds walked no more than the budget before they gave up


@pytest.mark.parametrize("shape", [S64, S128])
def test_false_alarms_spend_one_budget_per_level(vr, oracle, shape):
    """The threshold is 4 at every node of the leaf level, so no exact record fails, but the mean stays inside the quad
    bound's slack of the boundary and EVERY quad record fails (est_rounds_cases.near_boundary; asserted on the oracle's
    side in tests/test_est_round_plan.py).  The levels above walk nothing.  The quad rounds walk segments node by node
    until the budget is spent, BUDGET + 1 of them; with ONE budget per brick and level that is all the brick ever
    walks.  A budget per round would let each of the four quad rounds walk BUDGET + 1 again (the first prefix round
    alone has 15 segments at 64^3)."""
    (l0, l1), nseg = EC.limits(_depth(shape))
    assert l0 - EC.HEAD_SEGS > BUDGET + 1               # the first quad round can spend the budget by itself
    new, exact = _check(vr, oracle, _paired(oracle, shape, EC.near_boundary(shape[0] * shape[1] * shape[2] // 2)), adversarial=True)
    assert exact == 0
    assert new == BUDGET + 1


# ---------------------------------------------------------------- contents ----
@pytest.mark.parametrize("shape", [(16, 16, 32), (32, 32, 32), S64, S128], ids=["32x16x16", "32", "64", "128x64x64"])
@pytest.mark.parametrize("kind", ["saturated", "random", "slabs"])
def test_contents(vr, oracle, shape, kind):
    """Truths at 0-5 and 250-255 (windows clamped at 0), random bytes (candidates above 127), slabs of very different
    noise; 32x16x16 is D = 13: one estimator level of four segments behind the head, no prefix round."""
    rng = np.random.default_rng(shape[0] + shape[2] + len(kind))
    vol = {"saturated": lambda: _saturated(rng, shape, 0.05), "random": lambda: rng.integers(0, 256, shape, dtype=np.uint8),
           "slabs": lambda: _noise_slabs(rng, shape, [0, 60, 2, 120, 0, 8, 200, 1, 30])}[kind]()
    _check(vr, oracle, vol)


@pytest.mark.parametrize("shape,busy", [(S64, 0.2), (S128, 0.5)])
def test_constant_boxes_beside_noisy_ones(vr, oracle, shape, busy):
    rng = np.random.default_rng(int(busy * 100) + shape[0])
    _check(vr, oracle, _blocky(rng, shape, busy))


# ---------------------------------------------------------------- sets ----
def _five(O, rng, shape, flip):
    n2 = shape[0] * shape[1] * shape[2] // 2
    (l0, l1), nseg = EC.limits(_depth(shape))
    vols = [_paired(O, shape, EC.one_change(n2, l0 if flip else l1)), _blocky(rng, shape, 0.3),
            _paired(O, shape, EC.boundary(n2)), rng.integers(0, 256, shape, dtype=np.uint8),
            _paired(O, shape, EC.drift(n2, 9, 40) if flip else EC.drift(n2, 40, 22))]
    return vols[::-1] if flip else vols


@pytest.fixture(scope="module")
def five(oracle):
    rng = np.random.default_rng(79)
    out = {}
    for name, flip in (("A", False), ("B", True)):
        vols = _five(oracle, rng, S64, flip)
        out[name] = (vols, [oracle.OracleTree(v.copy(), tolerance=1, max_epochs=2).build() for v in vols])
    return out


def _set_equals_refs(bs, refs, shape, what):
    dec = bs.decode().cpu().numpy().reshape(len(refs), *shape)
    for b, ref in enumerate(refs):
        assert list(bs.distance_map(b)) == list(ref.distanceMap), (what, b)
        assert bs.info(b)["num_active_nodes"] == ref.numActiveNodes, (what, b)
        assert bs.info(b)["num_reverts"] == ref.numReverts, (what, b)
        assert np.array_equal(bs.tree(b), ref.tree), (what, b)
        assert np.array_equal(dec[b], ref.levelCut()), (what, b)


_FIVE_COUNTS = {}


def _five_counts(vr, five, name):
    """est_exact_segments per brick of set `name` under est_exact_bounds and under est_old_schedule (fresh handles, each
    held to the oracle bit for bit), once per module."""
    if name not in _FIVE_COUNTS:
        vols, refs = five[name]
        got = []
        for sw in ("est_exact_bounds", "est_old_schedule"):
            bs = vr.BrickSet(5, S64[::-1], 1, 2)
            bs.set_switch(sw, 1)
            bs.build(np.stack(vols))
            _set_equals_refs(bs, refs, S64, (name, sw))
            got.append([bs.info(b)["est_exact_segments"] for b in range(5)])
        _FIVE_COUNTS[name] = got
    return _FIVE_COUNTS[name]


@pytest.mark.parametrize("conc", [1, 2, 4])
def test_five_bricks_a_b_a_on_one_handle(vr, five, conc):
    """Bricks that leave the rounds at different stages (one spends its budget, one never walks, one changes at a limit),
    at every concurrency, rebuilt as A, B, A on one handle: control state of the build before must not leak.  Every
    build equals the oracle, as do the same sets built under est_exact_bounds and est_old_schedule; every brick but the
    boundary one (built to defeat the bounds) stays within the exact records' count + the budget per estimator level."""
    bs = vr.BrickSet(5, S64[::-1], 1, 2)
    bs.set_concurrency(conc)
    for name in ("A", "B", "A"):
        vols, refs = five[name]
        bs.build(np.stack(vols))
        _set_equals_refs(bs, refs, S64, (conc, name))
        exact, old = _five_counts(vr, five, name)
        for b in range(5):
            n = bs.info(b)["est_exact_segments"]
            print("conc %d build %s brick %d est_exact_segments: round plan %d, exact records %d, old schedule %d" %
                  (conc, name, b, n, exact[b], old[b]))
            assert 0 <= n <= _total_segments(S64), (conc, name, b)
            if b != 2:                      # brick 2 of A and of B (the middle of five, reversed or not): EC.boundary
                assert n <= exact[b] + BUDGET * _est_levels(S64), (conc, name, b)


def test_midrange_set(vr, oracle):
    """variant 2: both streams go through the same rounds, each with its own records and control blocks."""
    rng = np.random.default_rng(80)
    vols = [_noise_slabs(rng, S64, [0, 90, 4, 160, 1, 12]), _paired(oracle, S64, EC.drift(S64[0] ** 3 // 2, 9, 40)), _blocky(rng, S64, 0.5)]
    sets = []
    for sw in (None, "est_exact_bounds", "est_old_schedule"):
        bs = vr.BrickSet(len(vols), S64[::-1], 1, 2, 2)
        if sw:
            bs.set_switch(sw, 1)
        bs.build(np.stack(vols))
        sets.append(bs)
    decs = [s.decode().cpu().numpy().reshape(len(vols), *S64) for s in sets]
    for b, v in enumerate(vols):
        ref = oracle.OracleTree(v.copy(), tolerance=1, max_epochs=2, guarded=True, midrange=True).build()
        for s, dec in zip(sets, decs):
            assert np.array_equal(s.tree(b), ref.tree) and np.array_equal(s.tree_range(b), ref.tree_range), b
            assert list(s.distance_map(b)) == list(ref.distanceMap) and list(s.distance_map_range(b)) == list(ref.distanceMap_range), b
            assert s.info(b)["num_active_nodes"] == ref.numActiveNodes, b
            assert np.array_equal(dec[b], ref.levelCut()), b
        n, e, o = (s.info(b)["est_exact_segments"] for s in sets)
        print("midrange brick %d est_exact_segments: round plan %d, exact records %d, old schedule %d" % (b, n, e, o))
        assert 0 <= n <= e + BUDGET * _est_levels(S64), b


def test_general_extents(vr, oracle):
    """48 x 40 x 24 voxels (no power of two): D = 14, the two deepest levels go through the rounds."""
    shape = (24, 40, 48)
    rng = np.random.default_rng(81)
    for vol in (rng.integers(0, 256, shape, dtype=np.uint8), _noise_slabs(rng, shape, [0, 60, 2, 120, 0, 8])):
        ref = oracle.OracleTree(vol.copy(), tolerance=1, max_epochs=2).build()
        assert ref.origTreeDepth >= 13
        counts = []
        for sw in (None, "est_exact_bounds", "est_old_schedule"):
            bs = _build(vr, vol, 1, 2, sw)
            assert list(bs.distance_map(0)) == list(ref.distanceMap), sw
            assert bs.info(0)["num_active_nodes"] == ref.numActiveNodes and bs.info(0)["num_reverts"] == ref.numReverts, sw
            assert np.array_equal(bs.tree(0), ref.tree), sw
            assert np.array_equal(bs.decode().cpu().numpy().reshape(shape), ref.levelCut()), sw
            counts.append(bs.info(0)["est_exact_segments"])
        n, e, o = counts
        print("general extents est_exact_segments: round plan %d, exact records %d, old schedule %d" % (n, e, o))
        assert 0 <= n <= e + BUDGET * (ref.origTreeDepth - 12)          # levels 13 .. D have more than 4096 nodes
