"""Case volumes for the upper prune levels of k_prune_emit12 (depths D-12 .. D-5 of a 4096-leaf box) and its top-down
spine, shared by test_prune_chain_cpu.py (which asserts on the oracle that the cases contain what they are for) and
test_gpu_prune_chain.py (which builds them on the GPU).

A brick is noise with structure at every scale, and in it PLANTED subtrees: node i of in-block level lq (depth
D-12+lq, 2^(12-lq) leaves) of a box gets the value its parent is reconstructed with.  Its truth then equals its parent's
reconstruction, so its code is "keep" and so is every code below it, its leaves are exact, and the bottom-up prune
(R.cpp:596-629) turns it into one pruned token -- while its noisy sibling keeps the parent alive.  With tolerance 2 some
planted subtrees carry single leaves that are off by one instead of being constant: within tolerance, so pruned all the
same, but not a constant box for k_pyramid12.  The parent's reconstruction depends on the level distances, which depend
a little on the planted values, so the value is found by rebuilding the oracle until nothing moves.

The plants are chosen so that every (jmin, lq) pair occurs: a pruned node at level lq that is the leftmost level-lq
descendant of a RIGHT child at level jmin (of the box root for jmin = 0) -- what the thread whose spine starts at jmin
meets at level lq."""
import numpy as np

S12 = (16, 16, 16)          # (z, y, x): D = 12, one box, every in-block level present
S14 = (16, 32, 32)          # D = 14, four boxes
S15 = (32, 32, 32)          # D = 15, eight boxes
SHAPES = [S12, S14, S15]
BRICKS = {S12: 10, S14: 3, S15: 2}      # bricks the (jmin, lq) plants are spread over
PARAMS = [(1, 0), (1, 1), (1, 2), (2, 0), (2, 1), (2, 2)]       # (tolerance, max_epochs); max_epochs 0 builds with a leaf level

_ORDER = {}


def leaf_order(O, shape):
    """voxel index (x fastest) of every leaf rank of a `shape` brick, read off the oracle's pyramid"""
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


def from_leaves(O, leaves, shape):
    vol = np.empty(leaves.size, np.uint8)
    vol[leaf_order(O, shape)] = leaves
    return vol.reshape(shape)


def depth_of(shape):
    return int(np.log2(shape[0] * shape[1] * shape[2]) + 0.5)


def noise_leaves(rng, D, amp=12):
    """2^D leaves with structure at every scale: every level moves its nodes by up to +-amp"""
    v = np.full(1, 128, np.int64)
    for _ in range(D):
        v = np.repeat(v, 2) + rng.integers(-amp, amp + 1, 2 * v.size)
    return np.clip(v, 0, 255)


def plan(shape):
    """[(brick, box, lq, i)]: the planted nodes of the shape's case, the same for every (tolerance, max_epochs)"""
    D = depth_of(shape)
    nb = 1 << (D - 12)
    rng = np.random.default_rng(1000 + D)
    combos = sorted(((jmin, lq) for jmin in range(8) for lq in range(jmin, 8)), key=lambda c: c[1])
    bins = {(br, bx): [] for br in range(BRICKS[shape]) for bx in range(nb)}     # planted leaf ranges per box
    plants = []
    for jmin, lq in combos:
        if lq == 0 and nb == 1:
            continue            # the only box's root is the tree's root: a brick pruned there is a constant brick
        odd = list(rng.permutation(np.arange(1, 1 << jmin, 2))) if jmin else [0]
        placed = False
        for (br, bx), used in bins.items():
            for ip in odd:
                i = int(ip) << (lq - jmin)
                lo, hi = i << (12 - lq), (i + 1) << (12 - lq)
                sib = ((i ^ 1) << (12 - lq), ((i ^ 1) + 1) << (12 - lq))
                if lq == 0:
                    # a whole box: its sibling box stays noise
                    if used or bins[(br, bx ^ 1)]:
                        continue
                elif (any(lo < h and l < hi for l, h in used) or any(sib[0] < h and l < sib[1] for l, h in used)
                      or sum(h - l for l, h in used) + hi - lo > 2048):
                    continue
                used.append((lo, hi))
                plants.append((br, bx, lq, i))
                placed = True
                break
            if placed:
                break
        assert placed, (shape, jmin, lq)
    if shape == S15:
        # one more brick for the write-back of codes that share a byte with a neighbouring box's (heap nodes 1 .. 3):
        # level-1 nodes of boxes 0 and 1, the roots of boxes 4 and 6
        br = BRICKS[shape]
        plants += [(br, 0, 1, 1), (br, 1, 1, 0), (br, 4, 0, 0), (br, 6, 0, 0)]
    return plants


def num_bricks(shape):
    return BRICKS[shape] + (1 if shape == S15 else 0)


_CASES = {}


def case(O, shape, tol, ep):
    """(volumes, plants) of one case: num_bricks(shape) bricks of `shape`"""
    key = (shape, tol, ep)
    if key in _CASES:
        return _CASES[key]
    D = depth_of(shape)
    plants = plan(shape)
    vols = []
    for br in range(num_bricks(shape)):
        rng = np.random.default_rng(77 * D + br)
        leaves = noise_leaves(rng, D)
        mine = [(bx, lq, i) for b, bx, lq, i in plants if b == br]
        for _ in range(8):
            vol = from_leaves(O, leaves.astype(np.uint8), shape)
            rec = np.asarray(O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep).build(2).recon_all)
            moved = False
            for k, (bx, lq, i) in enumerate(mine):
                d = D - 12 + lq
                g = (bx << lq) + i
                c = int(rec[(1 << (d - 1)) - 1 + (g >> 1)])
                seg = np.full(1 << (12 - lq), c, np.int64)
                if tol == 2 and k % 2 == 0:        # within tolerance, not constant: single leaves off by one
                    seg[5::16] = c + 1 if c < 255 else c - 1
                lo = (g << (12 - lq))
                if not np.array_equal(leaves[lo:lo + seg.size], seg):
                    leaves[lo:lo + seg.size] = seg
                    moved = True
            if not moved:
                break
        vols.append(from_leaves(O, leaves.astype(np.uint8), shape))
    _CASES[key] = (vols, plants)
    return _CASES[key]


# ---------------------------------------------------------------- what the oracle's code arrays say about a case ----
def codes_of(tree_bits, n):
    """the first n 2-bit BFS codes of an oracle tree array (node k: bits 2 (k & 3) of byte k >> 2)"""
    b = np.asarray(tree_bits)
    return ((np.repeat(b, 4)[:n] >> (2 * (np.arange(n) & 3))) & 3).astype(np.uint8)


def prune_codes(O, vol, tol, ep):
    """(codes the level loop left, codes after the prune), BFS order, all 2^(D+1) - 1 nodes"""
    a = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep).build(2)
    b = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep).build(3)
    n = a.numOrigNodes
    return codes_of(a.tree, n), codes_of(b.tree, n)


def spine(post, D, box, t):
    """k_prune_emit12's top-down walk of thread t of a box, on the pruned codes: (jmin, parent pruned, level of the first
    3 met or None, preDs, aliveAtDs)"""
    jmin = 8 - ((t & -t).bit_length() - 1) if t else 0
    at = lambda lq: int(post[(1 << (D - 12 + lq)) - 1 + (box << lq) + (t >> (8 - lq))])
    if jmin > 0 and at(jmin - 1) == 3:
        return jmin, True, None, 0, 0
    ns = pre = alive_ds = 0
    for lq in range(jmin, 8):
        if lq == 6:
            pre, alive_ds = ns, 1
        ns += 1
        if at(lq) == 3:
            return jmin, False, lq, pre, alive_ds
    return jmin, False, None, pre, alive_ds
