"""The HIP level loop (k_control, k_level_end and the fills and estimators around them, kd_encode.hip) on the cases of
tests/levelcases.py, against the CPU oracle, bit for bit.

tests/test_level_control_cpu.py asserts on the oracle which decision -- revert, second revert, clamped step, the
three alt-plane selections, ... -- every case takes at which class of level: one wave, partials from memory, partials
staged in LDS, the chunk loop's second trip, levels with skipped blocks, the leafless leaf level, general extents.
Here every case is built alone, as a MidRangeTree, inside one batched set per shape (so that one launch of k_control
holds bricks that decide differently), with the level loop split over streams, and again on a used handle.  Nothing
is compared with a tolerance and no level is left out.  A wrong decision at level d first shows as a wrong distance at
d, so a mismatch names that level, its class and what the oracle decided there."""
import numpy as np
import pytest

import levelcases as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


_MID = {}


def _mid_tree(O, name):
    if name not in _MID:
        _MID[name] = L.oracle_tree(O, L.CASES[name], L.built(O, name)[0], midrange=True)
    return _MID[name]


def _dims(shape):
    return shape[::-1]          # (z, y, x) -> (x, y, z)


def _blame(O, name, got, ref, stream=0):
    """the first level whose distance differs: its class and the oracle's decisions there"""
    D = ref.origTreeDepth
    want = list(ref.distanceMap_range if stream else ref.distanceMap)
    for d, (g, w) in enumerate(zip(got, want)):
        if g != w:
            if d > D:
                return "%s: chain level %d: distance %d, oracle %d" % (name, d, g, w)
            ev = L.decisions(ref, L.CASES[name].max_epochs, stream)[d]["events"]
            return "%s%s: level %d %r: distance %d, oracle %d; the oracle's loop there: %r" % (
                name, " (half-range stream)" if stream else "", d, L.class_of_level(O, name, d), g, w, ev)
    return None


def _check_brick(O, bs, b, name, ref, dec, what, midrange=False):
    """everything test_gpu_codec.check_case compares, for brick b of a set"""
    info = bs.info(b)
    assert info["orig_tree_depth"] == ref.origTreeDepth and info["max_tree_depth"] == ref.maxTreeDepth, (name, what)
    bad = _blame(O, name, list(bs.distance_map(b)), ref)
    assert bad is None, (bad, what)
    if midrange:
        bad = _blame(O, name, list(bs.distance_map_range(b)), ref, 1)
        assert bad is None, (bad, what)
    # every distance agrees: what differs now comes from a level's reconstruction or codes.  The message carries the
    # levels the oracle reverted at (the buffer roles) and the leaf level's loop (the alt planes, the final distances)
    dd = L.decisions(ref, L.CASES[name].max_epochs)
    D = ref.origTreeDepth
    hint = (name, what, "reverts at %r" % [(d, L.class_of_level(O, name, d)) for d in dd if dd[d]["reverts"]],
            "leaf level: %r" % dd[D]["events"])
    assert info["num_reverts"] == ref.numReverts, ("num_reverts", info["num_reverts"], ref.numReverts) + hint
    assert info["num_active_nodes"] == ref.numActiveNodes, ("num_active_nodes",) + hint
    assert np.array_equal(bs.tree(b), ref.tree), ("stream bytes",) + hint
    if midrange:
        assert np.array_equal(bs.tree_range(b), ref.tree_range), ("half-range stream bytes",) + hint
    assert info["zero_run_rewrites"] == 0 and ref.zeroRunRewrites == 0, ("zero_run_rewrites",) + hint
    st = ref.leaf_stats()
    assert info["max_error_before"] == st["max_before"] and info["max_error_after"] == st["max_after"], ("max error",) + hint
    assert abs(info["mean_l1_after"] - st["l1_after"]) < 1e-12, ("mean L1",) + hint
    assert np.array_equal(dec, ref.levelCut()), ("decoded voxels",) + hint


def _check_cuts(bs, b, n, shape, ref, name):
    D = ref.origTreeDepth
    for cut in (D, D - 3):
        got = bs.decode(cut_depth=cut).cpu().numpy().reshape(n, *shape)[b]
        assert np.array_equal(got, ref.levelCutProgressive(cut)), (name, cut)


def _outputs(bs, b, dec):
    return dict(tree=bs.tree(b).tobytes(), dmap=tuple(bs.distance_map(b)), info=bs.info(b), dec=dec.tobytes())


def _single(vr, O, name, vol=None, tol=1, ep=5):
    """one brick alone on a fresh handle: (set, outputs)"""
    if vol is None:
        c = L.CASES[name]
        vol, tol, ep, variant = L.built(O, name)[0], c.tolerance, c.max_epochs, c.variant
    else:
        variant = 0
    bs = vr.BrickSet(1, _dims(vol.shape), tol, ep, variant).build(vol.copy())
    return bs, _outputs(bs, 0, bs.decode().cpu().numpy())


# ---- every case alone --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(L.CASES))
def test_case_alone(vr, oracle, name):
    """One brick, one set.  The f23 cases are the one place the workload's own 256 x 256 x 128 brick is needed: only
    its leaf level has more than 64 chunks of partials, so only there does k_control's chunk loop make a second
    trip."""
    vol, ref = L.built(oracle, name)
    bs, out = _single(vr, oracle, name)
    _check_brick(oracle, bs, 0, name, ref, np.frombuffer(out["dec"], np.uint8).reshape(vol.shape), "alone")
    _check_cuts(bs, 0, 1, vol.shape, ref, name)


_MIDRANGE = [n for n, c in L.CASES.items() if c.variant == L.PLAIN and L.depth_of(L._pow2_above(c.shape)) <= 19]


@pytest.mark.parametrize("name", _MIDRANGE)
def test_case_as_midrange_tree(vr, oracle, name):
    """Variant 2 on every case up to 128 x 64 x 64 (the 256 x 256 x 128 ones are left out for their time: two oracle
    level loops of 2^23 leaves each): both streams, both distance maps and the reverts of both loops.  The half-range
    stream runs a level loop of its own, with its own control blocks, beside the mid stream's."""
    c = L.CASES[name]
    vol, _ = L.built(oracle, name)
    ref = _mid_tree(oracle, name)
    bs = vr.BrickSet(1, _dims(vol.shape), c.tolerance, c.max_epochs, 2).build(vol.copy())
    _check_brick(oracle, bs, 0, name, ref, bs.decode().cpu().numpy().reshape(vol.shape), "midrange", midrange=True)
    assert np.array_equal(bs.decode_range().cpu().numpy().reshape(vol.shape), ref.levelCutRange())
    assert np.array_equal(bs.packed4(0), ref.convertToByteArray())


# ---- batched -----------------------------------------------------------------------------------------------------------
_SETS = L.case_sets()
_SET_IDS = ["%dx%dx%d" % _dims(k[0]) for k in _SETS]
CONST = 77


def _set_volumes(O, key):
    names = _SETS[key]
    return names + ["const"], [L.built(O, n)[0] for n in names] + [np.full(key[0], CONST, np.uint8)]


def _set_refs(O, key):
    shape, tol, ep = key
    const = O.OracleTree(np.full(shape, CONST, np.uint8), tolerance=tol, max_epochs=ep).build()
    return [L.built(O, n)[1] for n in _SETS[key]] + [const]


@pytest.mark.parametrize("key", list(_SETS), ids=_SET_IDS)
def test_batched_set(vr, oracle, key):
    """All cases of one shape in ONE set, and a constant brick: in one launch of k_control bricks of the same level
    revert, go on, are already inactive or never started.  Each brick equals the oracle and its own single-brick
    build."""
    shape, tol, ep = key
    names, vols = _set_volumes(oracle, key)
    if len(names) > 2:        # the census: a reverting brick beside one whose loop has ended, at one level and epoch
        hits = L.revert_beside_inactive({n: L.decisions(L.built(oracle, n)[1]) for n in names[:-1]})
        print("revert beside an inactive brick: %d, first %r" % (len(hits), hits[:1]))
        assert hits
    assert names[-1] == "const" and int(vols[-1].min()) == int(vols[-1].max())
    n = len(vols)
    bs = vr.BrickSet(n, _dims(shape), tol, ep).build(np.stack(vols))
    dec = bs.decode().cpu().numpy().reshape(n, *shape)
    for b, (name, ref) in enumerate(zip(names, _set_refs(oracle, key))):
        if name == "const":
            assert bs.info(b)["num_active_nodes"] == ref.numActiveNodes and np.array_equal(bs.tree(b), ref.tree)
            assert list(bs.distance_map(b)) == list(ref.distanceMap) and np.array_equal(dec[b], ref.levelCut())
        else:
            _check_brick(oracle, bs, b, name, ref, dec[b], "batched")
        _, alone = _single(vr, oracle, name, vols[b], tol, ep)
        got = _outputs(bs, b, dec[b])
        for k in alone:
            assert got[k] == alone[k], (name, k, "batched against alone")


@pytest.mark.parametrize("key", [k for k in _SETS if L.depth_of(L._pow2_above(k[0])) <= 19],
                         ids=[i for i, k in zip(_SET_IDS, _SETS) if L.depth_of(L._pow2_above(k[0])) <= 19])
def test_batched_set_across_level_loop_streams(vr, oracle, key):
    """The same sets with the level loop split over 2 and 4 brick ranges (set_concurrency; a range needs 16 bricks to
    fork, so the set is repeated to 64 bricks, turned by one brick each time so that the ranges cut it elsewhere).
    Every brick equals its single-brick build.  The 256 x 256 x 128 set is left out: 64 such bricks."""
    shape, tol, ep = key
    names, vols = _set_volumes(oracle, key)
    alone = {name: _single(vr, oracle, name, v, tol, ep)[1] for name, v in zip(names, vols)}
    order = []
    turn = 0
    while len(order) < 64:
        order += [(i + turn) % len(names) for i in range(len(names))]
        turn += 1
    order = order[:64]
    stack = np.stack([vols[i] for i in order])
    for streams in (2, 4):
        bs = vr.BrickSet(64, _dims(shape), tol, ep).set_concurrency(streams).build(stack)
        dec = bs.decode().cpu().numpy().reshape(64, *shape)
        for b, i in enumerate(order):
            got = _outputs(bs, b, dec[b])
            for k in got:
                if got[k] != alone[names[i]][k]:
                    bad = _blame(oracle, names[i], list(got["dmap"]), L.built(oracle, names[i])[1]) if names[i] != "const" else None
                    raise AssertionError((streams, b, names[i], k, bad))


# ---- a used handle -----------------------------------------------------------------------------------------------------
def test_rebuilds_on_one_handle(vr, oracle):
    """A, B, A on one handle.  A's last leaf epoch reads the minus plane and its loop reverts once, B's reads the plus
    plane and reverts three times (asserted on the CPU): Ctrl carries altValid, altSel, pendingEqual and the buffer
    roles from level to level, and none of it may reach the next build.  The third build equals the first byte for
    byte, and both equal the oracle."""
    a, b = L.REUSE
    (va, ra), (vb, rb) = L.built(oracle, a), L.built(oracle, b)
    assert L.alt_epoch(ra) != L.alt_epoch(rb) and ra.numReverts != rb.numReverts
    c = L.CASES[a]
    bs = vr.BrickSet(1, _dims(va.shape), c.tolerance, c.max_epochs)
    outs = []
    for name, vol, ref in ((a, va, ra), (b, vb, rb), (a, va, ra)):
        bs.build(vol.copy())
        dec = bs.decode().cpu().numpy().reshape(vol.shape)
        _check_brick(oracle, bs, 0, name, ref, dec, "rebuild")
        outs.append(_outputs(bs, 0, dec))
    assert outs[0] == outs[2]
    assert outs[0]["tree"] != outs[1]["tree"]
