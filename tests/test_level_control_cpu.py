"""The level loop's control decisions at every level class, on the CPU oracle alone.

tests/levelcases.py builds volumes that make a chosen level of the encoder's gradient-descent loop (R.cpp:206-384; on
the GPU k_control / k_level_end in kd_encode.hip) take a chosen decision, and reads the decisions back off the oracle's
own trace.  This module asserts that census -- which case reaches which (decision, level class) cell -- so that
tests/test_gpu_level_control.py, which compares the HIP codec with the oracle on the same cases bit for bit, is known to
exercise the revert on the LDS-staged path, the second revert of a level, the three alt-plane selections and the rest,
instead of meeting them by luck.  It also pins the oracle itself to the reference codec on the new volumes."""
import numpy as np
import pytest

import levelcases as L


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref/libvkref.so is not built: no reference sources at %s" % oracle.ref_dir())
    return oracle


def _reached(oracle, name):
    vol, tree = L.built(oracle, name)
    return L.cells(oracle, L.CASES[name], tree, vol)


# ---- the tools ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(16, 16, 16), (16, 32, 64), (8, 2, 32), (1, 4, 2), (64, 64, 128)], ids=str)
def test_leaf_order_is_the_oracles(oracle, shape):
    """leaf_order's arithmetic against the oracle's own pyramid: coordinate volumes, whose leaf truths are the leaves'
    coordinates (the method of test_gpu_const_boxes._leaf_order)."""
    z, y, x = np.meshgrid(np.arange(shape[0]), np.arange(shape[1]), np.arange(shape[2]), indexing="ij")
    idx = 0
    for c, mul in ((z, shape[1] * shape[2]), (y, shape[2]), (x, 1)):
        t = oracle.OracleTree(c.astype(np.uint8), tolerance=1, max_epochs=1).build(1)
        n = 1 << t.origTreeDepth
        idx = idx + np.asarray(t.temp)[n - 1:2 * n - 1].astype(np.int64) * mul
    assert np.array_equal(idx, L.leaf_order(shape))


def test_level_classes_at_their_edges():
    """The thresholds of compress_stream / k_control (kd_encode.hip): EST_HEAD = 4096 nodes, 256 partials of 1024 nodes
    for the LDS stage, more than 64 chunks of 64 partials for the second trip."""
    assert L.level_class(23, 12) == ("wave",) and L.level_class(23, 13) == ("mem",)
    assert L.level_class(23, 17) == ("mem",) and L.level_class(23, 18) == ("staged",)
    assert L.level_class(23, 22) == ("staged",) and L.level_class(23, 23) == ("staged2", "leafless_leaf", "bigleaf")
    assert L.level_class(18, 18) == ("staged", "leafless_leaf", "bigleaf")
    assert L.level_class(17, 17) == ("mem", "leafless_leaf") and L.level_class(11, 11) == ("wave",)
    assert L.level_class(12, 12, max_epochs=0) == ("wave",)
    assert L.level_class(18, 15, 3) == ("mem",) and L.level_class(18, 16, 3) == ("mem", "skip")
    assert L.level_class(18, 18, 3) == ("staged", "skip", "leafless_leaf", "bigleaf")
    assert L.level_class(13, 13, 3) == ("mem", "leafless_leaf")             # (no SkipBlocks below D = 14)
    assert L.level_class(13, 4, general=True) == ("wave", "general")
    for cls, (x, y, z) in L.SMALLEST.items():
        D = L.depth_of((x, y, z)) if not L.is_general((x, y, z)) else 1
        assert any(cls in L.level_class(D, d, 1, L.is_general((x, y, z))) for d in range(D + 1)), cls


@pytest.mark.parametrize("name", list(L.CASES))
def test_decisions_agree_with_the_tree(oracle, name):
    """decisions() restates the trace: its final distance is distanceMap[d] at every level, its reverts add up to
    numReverts, and every level's list ends in exactly one exit."""
    vol, tree = L.built(oracle, name)
    dec = L.decisions(tree)
    D = tree.origTreeDepth
    assert sorted(dec) == list(range(D + 1))
    assert [dec[d]["distance"] for d in range(D + 1)] == list(tree.distanceMap[:D + 1])
    mid_only = sum(r["reverts"] for r in dec.values())
    assert mid_only == tree.numReverts
    for d, r in dec.items():
        exits = [e for e in r["events"] if e in ("break_err", "break_same", "epoch_limit", "exit_small_step")]
        assert len(exits) == 1 and r["events"][-1] == exits[0], (d, r["events"])
        assert r["events"].count("fill") >= 1


# ---- the census -----------------------------------------------------------------------------------------------------
def test_census(oracle):
    """Every cell that CENSUS claims is reached by the named case, at a level of the named class that is at least as
    large as the cell asks.  Prints the table: cell, case, levels."""
    bad = []
    print()
    print("%-18s %-14s %-13s %s" % ("decision", "level class", "case", "levels"))
    for (dec, cls), (name, min_level) in L.CENSUS.items():
        if name is None:
            print("%-18s %-14s %-13s" % (dec, cls, "UNREACHED"))
            continue
        reached = _reached(oracle, name)
        levels = [d for d in reached.get((dec, cls), []) if d >= min_level]
        print("%-18s %-14s %-13s %s" % (dec, cls, name, levels))
        if not levels:
            bad.append("%s at %s: %s reaches instead %r" % (dec, cls, name, sorted(
                (k, v) for k, v in reached.items() if k[0] == dec or k[1] == cls)))
    assert not bad, "\n".join(bad)


def test_required_cells_are_claimed_or_listed_unreached():
    """Every cell the census has to hold is in it; the unreached ones are at most a quarter and each has its record."""
    missing = [c for c in L.REQUIRED if c not in L.CENSUS]
    assert not missing, missing
    unreached = [c for c in L.REQUIRED if L.CENSUS[c][0] is None]
    print("required cells: %d, unreached: %r" % (len(L.REQUIRED), unreached))
    assert 4 * len(unreached) <= len(L.REQUIRED)
    for dec, _ in unreached:
        assert dec in L.UNREACHED
    assert set(L.CASES[a]._replace(variant=0) for a in L.GUARD_PAIR) == {L.CASES[L.GUARD_PAIR[0]]}


def test_unreached_cells_are_still_unreached(oracle):
    """The standing record of levelcases.UNREACHED: no committed case, at any level of any class, takes a decision
    that the table lists as unreached.  The day a new volume does, this fails and the cell gets its case."""
    for name in L.CASES:
        for (dec, cls), levels in _reached(oracle, name).items():
            assert dec not in L.UNREACHED, (name, dec, cls, levels)


def test_guard_changes_the_work_not_the_result(oracle):
    """The :333 guard skips the central difference of the last epoch.  One reverting case both ways: fewer central
    differences in the trace, the same distances, stream and decoded voxels."""
    (_, a), (_, b) = (L.built(oracle, n) for n in L.GUARD_PAIR)
    assert L.CASES[L.GUARD_PAIR[1]].variant == L.GUARDED and a.numReverts >= 1
    ndf = [sum(r["kind"] == L.DF for r in t.trace()) for t in (a, b)]
    assert ndf[1] < ndf[0], ndf
    assert a.numActiveNodes == b.numActiveNodes and a.numReverts == b.numReverts
    assert np.array_equal(a.distanceMap, b.distanceMap) and np.array_equal(a.tree, b.tree)
    assert np.array_equal(a.levelCut(), b.levelCut())


def test_near_tie(oracle):
    """Only where currentError and what it is compared with agree to one part in 2^40 can the order of the double sum
    change a decision.  The searches met one such comparison at a level of 2^18 nodes, and it is an exact tie: the
    second epoch's error of NEAR_TIE's level equals the first's bit for bit, so `currentError > previousError` is
    false by nothing, and any kernel that sums in another order reverts there."""
    name, level = L.NEAR_TIE
    _, tree = L.built(oracle, name)
    gaps = [(abs(a - b) / b, kind) for d, kind, a, b in L.comparisons(tree) if d == level]
    print("comparisons at level %d of %s: %r" % (level, name, gaps))
    assert level >= 18 and min(gaps)[0] < 2.0 ** -40 and min(gaps)[1] == "revert"
    assert L.decisions(tree)[level]["reverts"] == 0


# ---- the sets the GPU module builds -----------------------------------------------------------------------------------
def test_batched_sets_hold_a_revert_beside_an_inactive_brick(oracle):
    """Every shape's cases go into one BrickSet on the GPU.  In each set of more than one case some brick reverts at a
    level, in an epoch, in which another brick's loop has already ended: one launch of k_control takes both paths."""
    for (shape, tol, ep), names in L.case_sets().items():
        decs = {n: L.decisions(L.built(oracle, n)[1]) for n in names}
        hits = L.revert_beside_inactive(decs)
        print("%r: %d cases, %d (level, epoch, reverting, inactive) pairs, first %r" % (shape, len(names), len(hits), hits[:1]))
        assert len(names) < 2 or hits, shape


def test_handle_reuse_cases_differ(oracle):
    a, b = (L.built(oracle, n)[1] for n in L.REUSE)
    assert L.alt_epoch(a) != L.alt_epoch(b) and None not in (L.alt_epoch(a), L.alt_epoch(b))
    assert a.numReverts != b.numReverts


# ---- the oracle itself, on the new volumes ------------------------------------------------------------------------------
_SMALL = [n for n, c in L.CASES.items() if L.depth_of(L._pow2_above(c.shape)) <= 18 and c.variant == L.PLAIN]


@pytest.mark.parametrize("midrange", [False, True], ids=["kd", "mid"])
@pytest.mark.parametrize("name", _SMALL)
def test_ref_reproduces_the_cases(ref, name, midrange):
    """The reference codec, built in place, on every case up to 64^3: stream bytes, distance map(s), numActiveNodes."""
    c = L.CASES[name]
    vol, tree = L.built(ref, name)
    o = L.oracle_tree(ref, c, vol, midrange=True) if midrange else tree
    r = ref.RefTree(vol.copy(), tolerance=c.tolerance, max_epochs=c.max_epochs, midrange=midrange).build()
    assert r.numActiveNodes == o.numActiveNodes
    assert np.array_equal(r.distanceMap, o.distanceMap) and np.array_equal(r.tree, o.tree)
    if midrange:
        assert np.array_equal(r.distanceMap_range, o.distanceMap_range) and np.array_equal(r.tree_range, o.tree_range)
