"""The cases of tests/prunecases.py really contain what test_gpu_prune_chain.py needs them for -- asserted here on the
CPU oracle's own code arrays (the BFS codes after the level loop, `build(2)`, and after the prune, `build(3)`), so that
the GPU test cannot pass by never reaching a path of k_prune_emit12's upper levels or of its top-down spine.

Classes, over the bricks of all cases of a shape:
  * for every in-block level lq (depth D-12+lq) a node that the bottom-up rule turns into a pruned token -- code 0, both
    children pruned -- while its parent stays live.  lq = 0 (the whole box becomes the single token 3) needs a parent
    above the box: the shapes with D > 12.  At D = 12 the box root is the tree root and a brick pruned there is a
    constant brick, which never reaches the kernel.
  * threads of every jmin 0 .. 8 whose spine ends at every possible level: alive through level 7, a 3 met at every
    lq >= jmin, and (jmin >= 1) a pruned parent.
  * a box whose depth-(D-6) entries are dead for some 64-leaf groups and live, behind spine tokens (preDs > 0), for others.
  * a multi-box brick where heap nodes 1 .. 3 of two boxes that share a code byte both change (the cset3 write-back).

Dropped from the issue's list, with the reason asserted below: "a node that was already 3 from the level loop next to a
live one".  The level loop writes codes 0, 1, 2 only (encode_node), so no build produces it in the mid stream's launch.
The `code == 3` input exists in the RANGE launch alone, which reads the codes the first launch has already pruned; what
it meets there is exactly the first class -- a pruned node beside a live sibling -- asserted per level here and run by
the MidRangeTree cases of the GPU test."""
import numpy as np
import pytest

import prunecases as pc


@pytest.fixture(scope="module")
def census(oracle):
    """per shape: the classes found over all of its cases"""
    out = {}
    for shape in pc.SHAPES:
        D = pc.depth_of(shape)
        nb = 1 << (D - 12)
        c = dict(bottom_up=set(), pruned_beside_live=set(), spine=set(), dead_parent=set(), mixed_ds=0, shared_byte=0,
                 pre3=0, planted_pruned=0, planted=0, whole_box_noncst=0)
        for tol, ep in pc.PARAMS:
            vols, plants = pc.case(oracle, shape, tol, ep)
            for br, vol in enumerate(vols):
                pre, post = pc.prune_codes(oracle, vol, tol, ep)
                c["pre3"] += int((pre == 3).sum())
                leaves = vol.reshape(-1)[pc.leaf_order(oracle, shape)].reshape(nb, 4096)
                for lq in range(8):
                    d = D - 12 + lq
                    if d == 0:
                        continue
                    k = np.arange((1 << d) - 1, (2 << d) - 1)
                    now3 = post[k] == 3
                    kids = (post[2 * k + 1] == 3) & (post[2 * k + 2] == 3)
                    par_live = post[(k - 1) >> 1] != 3
                    if (now3 & (pre[k] == 0) & kids & par_live).any():
                        c["bottom_up"].add(lq)
                    sib = ((k - 1) ^ 1) + 1
                    if (now3 & (post[sib] != 3)).any():
                        c["pruned_beside_live"].add(lq)
                for b, bx, lq, i in plants:
                    if b == br:
                        c["planted"] += 1
                        c["planted_pruned"] += int(post[(1 << (D - 12 + lq)) - 1 + (bx << lq) + i] == 3)
                        if lq == 0 and leaves[bx].min() != leaves[bx].max():
                            c["whole_box_noncst"] += int(post[(1 << (D - 12)) - 1 + bx] == 3)
                for bx in range(nb):
                    ds = set()
                    for t in range(256):
                        jmin, dead, end, pre_ds, alive_ds = pc.spine(post, D, bx, t)
                        if dead:
                            c["dead_parent"].add(jmin)
                        else:
                            c["spine"].add((jmin, end))
                        if t % 4 == 0:
                            ds.add("live" if alive_ds and pre_ds > 0 else ("live0" if alive_ds else "dead"))
                    c["mixed_ds"] += int("live" in ds and "dead" in ds)
                for lq in (0, 1):
                    d = D - 12 + lq
                    if d < 2:
                        continue
                    k = np.arange((1 << d) - 1, (2 << d) - 1)
                    ch = (pre[k] != post[k]).reshape(-1, 4)            # four nodes to a code byte
                    for row in ch:
                        boxes = {int(j) >> lq for j in np.nonzero(row)[0]}
                        c["shared_byte"] += int(len(boxes) > 1)
        out[shape] = c
    return out


@pytest.mark.parametrize("shape", pc.SHAPES, ids=["16x16x16", "32x32x16", "32x32x32"])
def test_bottom_up_prune_at_every_level(census, shape):
    c = census[shape]
    want = set(range(8)) if pc.depth_of(shape) > 12 else set(range(1, 8))
    assert c["bottom_up"] >= want, c["bottom_up"]
    assert c["pruned_beside_live"] >= want, c["pruned_beside_live"]
    # the value search settled: nearly every planted subtree is one pruned token
    assert c["planted_pruned"] >= 0.9 * c["planted"], (c["planted_pruned"], c["planted"])


@pytest.mark.parametrize("shape", pc.SHAPES, ids=["16x16x16", "32x32x16", "32x32x32"])
def test_level_loop_writes_no_pruned_token(census, shape):
    """why "already 3 from the level loop" is not a class of these cases (module docstring)"""
    assert census[shape]["pre3"] == 0


@pytest.mark.parametrize("shape", pc.SHAPES, ids=["16x16x16", "32x32x16", "32x32x32"])
def test_spine_ends_at_every_level(census, shape):
    c = census[shape]
    lowest = 0 if pc.depth_of(shape) > 12 else 1
    want = {(jmin, None) for jmin in range(9)} | {(jmin, lq) for jmin in range(8) for lq in range(max(jmin, lowest), 8)}
    assert c["spine"] >= want, sorted(want - c["spine"], key=str)
    # (jmin = 1: the parent is the box root, which only the shapes with D > 12 can prune)
    assert c["dead_parent"] >= set(range(lowest + 1, 9)), c["dead_parent"]
    assert c["mixed_ds"] > 0


def test_whole_box_pruned_on_the_full_path(census):
    """lq = 0 through k_prune_emit12 itself in a default build: a box that is not constant (leaves off by one, within
    tolerance 2) and still becomes the single token 3"""
    assert census[pc.S14]["whole_box_noncst"] > 0 and census[pc.S15]["whole_box_noncst"] > 0


def test_shared_code_bytes_change_together(census):
    assert census[pc.S15]["shared_byte"] > 0
