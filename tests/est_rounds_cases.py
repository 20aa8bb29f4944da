"""Volumes for the estimator's round plan (tests/test_est_round_plan.py, tests/test_gpu_est_rounds.py) whose threshold
trajectory on the leaf level is known in advance.

Construction: leaves 128 -+ a in sibling pairs, a per pair in leaf order (1 <= a <= 60: no node is forced).  Every level
above the leaves is 128 throughout and reproduced exactly, so its pd is 0 and its estimator walks nothing; the leaf
level's pd is a, a, per pair.  leaf_thresholds() restates the running-mean rule (counted <=> pd > 0 and S < pd (2C + 1),
in order) and returns the threshold floor(S / (2C + 1)) at every segment start.  With a = 9 up to pair k and 11 behind
it the threshold is 4, then 5 from node ~4k on, and never anything else: ONE change, placed in a chosen segment.
"""
import numpy as np

SEG, HEAD_SEGS = 1024, 4


def limits(level):
    """Python restatement of est_round_plan's prefix limits (tests/test_est_round_plan.py pins it to the program)."""
    nseg = (1 << level) // SEG
    out, at = [], HEAD_SEGS
    for shift in (4, 2):
        pre = (nseg - HEAD_SEGS) >> shift
        if pre >= 8 and HEAD_SEGS + pre > at:
            at = HEAD_SEGS + pre
            out.append(at)
    return out, nseg


def leaf_order(O, shape):
    """Flat voxel index of every leaf, in the order of the leaf level."""
    z, y, x = shape
    grids = np.meshgrid(np.arange(z), np.arange(y), np.arange(x), indexing="ij")
    coords = [np.array(O.OracleTree(g.astype(np.uint8), tolerance=0, max_epochs=1).build().temp, np.int64) for g in grids]
    flat = (coords[0] * y + coords[1]) * x + coords[2]
    assert np.array_equal(np.sort(flat), np.arange(z * y * x))
    return flat


def paired_volume(shape, order, a):
    a = np.asarray(a, np.int64)
    assert a.size * 2 == order.size and a.min() >= 1 and a.max() <= 60
    leaves = np.empty(order.size, np.int64)
    leaves[0::2] = 128 - a
    leaves[1::2] = 128 + a
    vol = np.empty(order.size, np.uint8)
    vol[order] = leaves
    return vol.reshape(shape)


def leaf_state(a):
    """(S, C) in front of every node of the leaf level (index n: behind the last) for pd = a, a per pair.  A count mask
    that reproduces itself under the rule is the in-order result (induction over the nodes)."""
    pd = np.repeat(np.asarray(a, np.int64), 2)
    m = pd > 0
    for _ in range(64):
        s = np.cumsum(pd * m) - pd * m
        c = np.cumsum(m) - m
        m2 = (pd > 0) & (s < pd * (2 * c + 1))
        if np.array_equal(m2, m):
            break
        m = m2
    else:
        raise AssertionError("no fixed point")
    S = np.concatenate([[0], np.cumsum(pd * m)])
    C = np.concatenate([[0], np.cumsum(m)])
    return S, C


def leaf_thresholds(a):
    """Threshold at the start of every segment of the leaf level (index nseg: at the level's end)."""
    S, C = leaf_state(a)
    at = np.arange(0, S.size, SEG)
    return S[at] // (2 * C[at] + 1)


def changes(T):
    """[(segment the change happens in, old, new)] behind the head"""
    return [(s, int(T[s]), int(T[s + 1])) for s in range(HEAD_SEGS, len(T) - 1) if T[s] != T[s + 1]]


def one_change(npairs, seg):
    """a: threshold 4 up to somewhere inside segment `seg`, 5 behind it."""
    for k in range(max(1, seg * SEG // 4 - 64), (seg + 1) * SEG // 4 + 64, 8):      # (C0 = 2k nodes of 9: the mean passes 5 at node ~4k)
        a = np.full(npairs, 9)
        a[k:] = 11
        ch = changes(leaf_thresholds(a))
        if ch == [(seg, 4, 5)]:
            return a
        if ch and ch[0][0] > seg:
            break
    raise AssertionError("no switch point puts the change into segment %d" % seg)


def constant(npairs):
    return np.full(npairs, 9)


def drift(npairs, first, then):
    """pd `first` over the first sixteenth of the level, `then` behind it: the mean runs monotonically from first / 2
    towards then / 2, fast at first and ever slower, its last steps far inside the bulk (drift(9, 40): up; drift(40, 22):
    down -- 22 stays above the threshold, so every node counts)."""
    a = np.full(npairs, then)
    a[:npairs // 16] = first
    return a


def near_boundary(npairs):
    """pd 9, 9, 7, 7, ... with three 8s for 7s at the very start: every node counts and S - 8 C runs 6, 7, 8, 7 behind
    the head, so floor(S / (2C + 1)) = 4 at EVERY node (>= 4 <=> S - 8 C >= 4) and no exact record ever fails -- but the
    mean stays within 4 units of the boundary, inside the slack 3 (Th - 1) = 9 of the quad records' bound A', so every
    quad record fails.  The false alarms are spread evenly over the level: every quad round meets them."""
    a = np.where((np.arange(npairs) & 1) == 0, 9, 7)
    a[[1, 3, 5]] = 8
    return a


def boundary(npairs):
    """the threshold alternates between 3 and 4 inside every segment (tests/test_gpu_est_quads.py's construction)"""
    a = np.where((np.arange(npairs) & 1) == 0, 9, 7)
    a[1] = 8
    return a
