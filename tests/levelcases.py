"""The level loop's control decisions, read off the oracle, and volumes built to make a chosen level take a chosen one.

Plain Python and NumPy plus the oracle module, which every function takes as an argument (`O`); no project code is
imported.  tests/test_level_control_cpu.py asserts on the CPU which decision every case of CASES takes at which level
class; tests/test_gpu_level_control.py then compares the HIP codec with the oracle on the same cases, bit for bit.

The loop is R.cpp:206-384 (oracle/kdtree_oracle.c compress_gradient_descent); on the GPU it is k_control and
k_level_end in volumerenderer_amd/csrc/kd_encode.hip, launched by compress_stream there.
"""
import collections

import numpy as np

# kinds of OracleTree.trace() records (kdtree_oracle.c vko_trace_rec)
START, FILL, REVERT, BREAK_ERR, BREAK_SAME, DF = range(6)

DECISIONS = ("fill", "break_err", "break_same", "revert", "revert_then_fill", "revert_final",
             "second_revert", "exit_small_step",
             "epoch_limit", "step_clamped", "distance_clamped")
ALT = ("alt_minus", "alt_plus", "alt_neither")

Case = collections.namedtuple("Case", "maker shape profile seed tolerance max_epochs variant")
PLAIN, GUARDED, MIDRANGE = 0, 1, 2       # `variant`: what vr.BrickSet takes


# ------------------------------------------------------------------------------------------------ the trace ----
def _levels(tree, stream=0):
    """the trace records by level; a MidRangeTree's trace holds the half-range stream's loop (stream 1) behind the
    mid stream's"""
    by, k = collections.defaultdict(list), -1
    for r in tree.trace():
        if r["kind"] == START and r["depth"] == 0:
            k += 1
        if k == stream:
            by[r["depth"]].append(r)
    return by


def decisions(tree, max_epochs=None, stream=0):
    """{level: dict(events=[...], distance=final distance, reverts=n, epochs=epoch counter at the exit, revert_epochs)} from
    tree.trace() and max_epochs alone (`tree.max_epochs` where the argument is not given: oracle_tree() sets it).

    The names, in the order the loop took them at the level:
      fill              a fill pass ran (kind 1)
      distance_clamped  ... at distance 0 or 255: the values the loop head's clamp (R.cpp:284) produces and at which
                        the central difference's own clamp binds (R.cpp:334, k_fill16's distM / distP)
      break_err         currentError < 1 (kind 3)
      revert            error above the previous epoch's (kind 2)
      second_revert     a revert at a level that has reverted before
      revert_then_fill  a revert with epochs left that is followed by another fill
      revert_final      the level ends, behind a revert, with a reconstruction that is not its last fill's: the
                        snapshot the swap brought back (or, behind a second revert, the first reverted fill:
                        recon.swap at R.cpp:329 exchanges, it does not restore).  Only here does the buffer swap of a
                        revert show: behind a later fill it does not, since that fill rewrites the buffer and the
                        distance recorded for it, whichever buffer it is; nor behind two reverts of fills at one
                        distance.  Worked out by following the contents of recon and reconPreviousEpoch.
      step_clamped      a central difference whose step is +-4 (kind 5, |-1.25 df| >= 4)
      break_same        the new distance equals the old one (kind 4)
      exit_small_step   the loop ended before the epoch limit with neither kind 3 nor kind 4 recorded: only the while
                        condition's |previousStepSize| < 0.5 is left
      epoch_limit       the epoch counter reached max_epochs
    The final distance is the loop's currentDistance at the exit: distanceMap[d]."""
    E = tree.max_epochs if max_epochs is None else max_epochs
    out = {}
    for d, recs in sorted(_levels(tree, stream).items()):
        ev, reverts, epoch, dist = [], 0, 0, recs[0]["distance"]
        recon_d = snap_d = last_fill_d = None       # the distance behind the contents of recon / reconPreviousEpoch
        for i, r in enumerate(recs):
            k = r["kind"]
            if k == START:
                dist = r["distance"]
            elif k == FILL:
                ev.append("fill")
                dist = recon_d = last_fill_d = r["distance"]
                if dist in (0.0, 255.0):
                    ev.append("distance_clamped")
                epoch = r["epoch"] + 1          # (a break leaves the counter where it is: set back below)
            elif k == BREAK_ERR:
                ev.append("break_err")
                epoch = r["epoch"]
            elif k == BREAK_SAME:
                ev.append("break_same")
                dist = r["distance"]
                epoch = r["epoch"]
            elif k == REVERT:
                reverts += 1
                ev.append("revert" if reverts == 1 else "second_revert")
                dist = r["distance"]
                if r["epoch"] + 1 < E and any(x["kind"] == FILL for x in recs[i + 1:]):
                    ev.append("revert_then_fill")
                recon_d, snap_d = snap_d, recon_d             # recon.swap(reconPreviousEpoch), R.cpp:329
            elif k == DF:
                snap_d = recon_d                              # reconPreviousEpoch = recon, R.cpp:364
                if abs(r["step"]) >= 4.0:
                    ev.append("step_clamped")
        if reverts and recon_d != last_fill_d:
            ev.insert(len(ev) - ev[::-1].index("revert" if reverts == 1 else "second_revert"), "revert_final")
        if E > 0:
            if "break_err" not in ev and "break_same" not in ev:
                ev.append("epoch_limit" if epoch >= E else "exit_small_step")
        out[d] = dict(events=ev, distance=int(dist), reverts=reverts, epochs=epoch,
                      revert_epochs=[r["epoch"] for r in recs if r["kind"] == REVERT])
    return out


def alt_epoch(tree, max_epochs=None):
    """Which of k_control's three selections the LAST epoch of the leaf level falls under: "alt_minus", "alt_plus",
    "alt_neither", or None where the leaf level never reaches its last epoch with a fill.  Meaningful for leafless
    builds (D >= 12, max_epochs >= 1: host_plan.cpp BuildPlan::leafless).

    Reads: the kind-1 (fill) records of depth D, their `epoch` and `distance`.  Every epoch that is entered and does
    not stop at "same distance" runs a fill, so the fill of epoch max_epochs-1 is the last epoch's and the fill of
    epoch max_epochs-2 is the one in front of it (a revert at epoch max_epochs-2 comes behind that epoch's fill).
    k_control, at the end of every real fill (altSel == 0) that has an epoch behind it (`c.epoch + 1 < maxEpochs`, so
    k_fill16 also left the minus / plus partials), sets altValid and altDist = that fill's distance -- reverted or
    not; at the loop head of the last epoch (`c.epoch + 1 >= maxEpochs`, the test at `leaflessLeaf && c.active &&
    c.altValid`) it compares the new distance nd with altDist: max(0, altDist-1) -> altSel 1 (the minus plane),
    min(255, altDist+1) -> altSel 2 (the plus plane), anything else -- altDist itself after a revert included -- a
    fill of its own.  nd is the last fill record's distance, altDist the one before's: that is the restatement."""
    E = tree.max_epochs if max_epochs is None else max_epochs
    D = tree.origTreeDepth
    fills = {r["epoch"]: r["distance"] for r in _levels(tree).get(D, []) if r["kind"] == FILL}
    if E < 2 or E - 1 not in fills or E - 2 not in fills:
        return None
    nd, a = int(fills[E - 1]), int(fills[E - 2])
    if nd != a and nd == max(0, a - 1):
        return "alt_minus"
    if nd != a and nd == min(255, a + 1):
        return "alt_plus"
    return "alt_neither"


def comparisons(tree):
    """Every comparison of the running double that decides something: (level, "revert" | "one", a, b) with a the
    epoch's currentError and b what it is compared with (the previous epoch's error at R.cpp:323, 1.0 at R.cpp:319)."""
    out = []
    for d, recs in _levels(tree).items():
        cur = None                              # currentError as the epoch in front left it
        for r in recs:
            if r["kind"] == FILL:
                out.append((d, "one", r["error"], 1.0))
                if r["epoch"] != 0 and cur is not None and r["error"] >= 1.0:
                    out.append((d, "revert", r["error"], cur))
                cur = r["error"]
            elif r["kind"] == REVERT:
                cur = r["error"]                # (the previous epoch's, restored)
    return out


def nearest_tie(tree, min_level=0):
    """(relative gap, level, kind) of the closest comparison at a level >= min_level, or None"""
    best = None
    for d, kind, a, b in comparisons(tree):
        if d >= min_level and b > 0:
            g = abs(a - b) / b
            if best is None or g < best[0]:
                best = (g, d, kind)
    return best


# ------------------------------------------------------------------------------------------- level classes ----
CLASSES = ("wave", "mem", "staged", "staged2", "skip", "leafless_leaf", "bigleaf", "general")

# smallest brick (x, y, z) that has a level of the class
SMALLEST = {"wave": (1, 1, 1), "mem": (32, 16, 16), "staged": (64, 64, 64), "staged2": (256, 256, 128),
            "skip": (32, 32, 16), "leafless_leaf": (16, 16, 16), "bigleaf": (64, 64, 64), "general": (3, 1, 1)}


def level_class(D, d, nblocks_skipped=0, general=False, max_epochs=1):
    """The classes of level d of a depth-D brick, as compress_stream / encode_launch (kd_encode.hip) launch it from build_level (host_plan.cpp); a
    tuple, the size class first.

    By the level's size n = 2^d (exactly one):
      wave     n <= 4096 (EST_HEAD): the start distance is k_est_head's one wave alone, and k_control's wave reads at
               most four partials (FILL_NODES_PER_BLOCK = 1024) from memory.  (The fill is k_fill below 4096 nodes and
               k_fill16 at 4096.)
      mem      4096 < n < 2^18: k_est_summ / k_est_walk rounds, k_fill16 with one chunk per workgroup, fewer than 256
               partials, read from memory in one or two chunks of 64.
      staged   2^18 <= n < 2^23: nblk >= 256, a multiple of 256 and <= CTL_STAGE_BLOCKS: the partials go through LDS;
               k_fill16 takes 4 (n < 2^21) or FILL_ITERS chunks per workgroup.
      staged2  n == 2^23: staged, and nchunk = 128 > 64: the chunk loop of k_control makes a second trip.  Only the leaf
               level of a 256 x 256 x 128 brick.
    On top of it:
      skip           d in D-2 .. D of a brick in which the level loop skips constant 4096-leaf blocks (SkipBlocks:
                     `nblocks_skipped` > 0, see skipped_blocks()): level D-2 sets the skip bits, D-1 and D pass over
                     the blocks.
      leafless_leaf  d == D of a leafless build (D >= 12, max_epochs >= 1): k_fill16<false>, the alt planes.
      bigleaf        d == D >= 18: the leaf level of a brick whose leaf level is staged.
      general        any level of a brick whose extents are not powers of two (k_pyramid<true> through srcIdx, no
                     k_pyramid12, no SkipBlocks).
    Out of scope, because they need a brick deeper than 256 x 256 x 128's 23 levels: levels of more than
    CTL_STAGE_BLOCKS partials (n >= 2^24: read from memory again, more than two trips)."""
    n = 1 << d
    out = ["wave" if n <= 4096 else "mem" if n < (1 << 18) else "staged" if n < (1 << 23) else "staged2"]
    assert d <= 23, "out of scope"
    if nblocks_skipped and not general and D >= 14 and d >= D - 2:
        out.append("skip")
    if d == D and D >= 12 and max_epochs >= 1:
        out.append("leafless_leaf")
    if d == D and D >= 18:
        out.append("bigleaf")
    if general:
        out.append("general")
    return tuple(out)


def is_general(shape):
    return any(s & (s - 1) for s in shape)


def skipped_blocks(tree, vol, tolerance, max_epochs, variant=PLAIN):
    """How many 4096-leaf blocks the level loop skips (BuildPlan::skipBlocks and k_fill16's level D-2 test): the
    block is one value and every depth-(D-3) node above it is reconstructed to exactly that value."""
    D = tree.origTreeDepth
    if D < 14 or tolerance < 1 or max_epochs < 1 or is_general(vol.shape) or int(vol.min()) == int(vol.max()):
        return 0
    nb = 1 << (D - 12)
    leaves = vol.reshape(-1)[leaf_order(vol.shape)].reshape(nb, 4096)
    const = (leaves == leaves[:, :1]).all(axis=1)
    n3 = 1 << (D - 3)
    par = np.asarray(tree.recon_all)[n3 - 1:2 * n3 - 1].reshape(nb, 512)
    return int((const & (par == leaves[:, :1]).all(axis=1)).sum())


# ------------------------------------------------------------------------------------------------- volumes ----
_ORDER = {}


def depth_of(shape):
    return sum(int(s).bit_length() - 1 for s in shape)


def leaf_order(shape):
    """voxel index (x fastest) of every leaf rank of a power-of-two `shape` = (z, y, x) brick: the split axis of depth
    k is k % 3 (x, y, z), passed on while that axis has one cell left (R.cpp:151-159)"""
    if shape not in _ORDER:
        ext = [shape[2], shape[1], shape[0]]
        assert not is_general(shape)
        D, axes, e = depth_of(shape), [], list(ext)
        for depth in range(D):
            sd, i = depth % 3, 0
            while e[sd] == 1:
                i += 1
                sd = (depth + i) % 3
            axes.append(sd)
            e[sd] //= 2
        r = np.arange(1 << D, dtype=np.int64)
        c = [np.zeros_like(r) for _ in range(3)]
        for depth, sd in enumerate(axes):
            c[sd] = c[sd] * 2 + ((r >> (D - 1 - depth)) & 1)
        _ORDER[shape] = c[0] + ext[0] * (c[1] + ext[1] * c[2])
    return _ORDER[shape]


def _draw(rng, spec, n):
    """one level's moves for n children (n/2 sibling pairs):
      an int a              uniform in [-a, a], every child on its own
      (a, b, p)             +-a with probability p, else +-b, every child on its own
      ("pair", a, b, p)     the two siblings move by +m and -m (the parent's midrange stays where it was and both are m
                            away from it), m = a with probability p, else b
      ("ord", a, b, f)      as "pair", but by place: m = a in the first fraction f of the level, b behind it.  The start
                            distance is a running mean in node order (R.cpp:254-266), so this is what puts it away from
                            the distance the fill wants"""
    if isinstance(spec, (int, np.integer)):
        return rng.integers(-spec, spec + 1, n) if spec else np.zeros(n, np.int64)
    if spec[0] in ("pair", "ord"):
        _, a, b, q = spec
        h = n // 2
        first = rng.random(h) < q if spec[0] == "pair" else np.arange(h) < int(q * h)
        m = np.where(first, a, b) * rng.choice((-1, 1), h)
        return np.stack([m, -m], axis=1).reshape(-1)
    a, b, p = spec
    mag = np.where(rng.random(n) < p, a, b)
    return mag * rng.choice((-1, 1), n)


def heap_leaves(D, profile, seed, start=128):
    """2^D leaves from a heap: one value, and each level moves its two children by a draw from the level's entry of
    `profile` (entry k: the move from depth k to depth k+1; missing entries are 0), clipped to 0 .. 255 at every
    level.  A level's truths are the midranges of its boxes, so they follow the heap's values as far as the
    amplitudes below the level are small."""
    rng = np.random.default_rng(seed)
    v = np.full(1, start, np.int64)
    for spec in expand(profile, D):
        v = np.clip(np.repeat(v, 2) + _draw(rng, spec, 2 * v.size), 0, 255)
    return v.astype(np.uint8)


def runs(profile):
    """a profile as ((first level, entry), ...): each entry holds until the next pair's level"""
    out, last = [], object()
    for k, e in enumerate(profile):
        if e != last:
            out.append((k, e))
            last = e
    return tuple(out)


def expand(profile, D):
    """the D entries of a profile given either way (runs() form, or entry by entry)"""
    if profile and all(isinstance(e, tuple) and len(e) == 2 for e in profile):
        at, cur, out = dict(profile), 0, []
        for k in range(D):
            cur = at.get(k, cur)
            out.append(cur)
        return out
    return list(profile) + [0] * (D - len(profile))


def _pow2_above(shape):
    return tuple(1 << (int(s) - 1).bit_length() for s in shape)


def make_volume(case):
    """uint8 [z][y][x] of a case.  Makers:
      heap       profile = per-level entries of heap_leaves
      heap_flat  profile = (entries, flat_depth, flat_every): as heap, and every `flat_every`-th pair of depth
                 `flat_depth` nodes (two siblings) is flattened to one value, the left one's heap value: constant 4096-leaf
                 blocks, beside busy ones, that their ancestors reproduce exactly (SkipBlocks)
      heap_crop  a general-extents `shape`: the heap volume of the enclosing power-of-two shape, cropped
      start      profile = (start value, entries): as heap, from another root value (0 and 255 saturate)
      const      one value, `seed`"""
    shape = tuple(case.shape)
    if case.maker == "const":
        return np.full(shape, case.seed, np.uint8)
    full = _pow2_above(shape)
    D = depth_of(full)
    if case.maker == "heap_flat":
        entries, fd, every = case.profile
        assert fd <= D - 13
        rng = np.random.default_rng(case.seed)
        v = np.full(1, 128, np.int64)
        for k, spec in enumerate(expand(entries, D)):
            v = np.clip(np.repeat(v, 2) + _draw(rng, spec, 2 * v.size), 0, 255)
            if k + 1 == fd:
                keep = v.copy()
        v = v.reshape(1 << fd, -1)
        for node in range(0, 1 << fd, 2 * every):
            v[node:node + 2] = keep[node]
        leaves = v.reshape(-1).astype(np.uint8)
    elif case.maker == "start":
        leaves = heap_leaves(D, case.profile[1], case.seed, case.profile[0])
    else:
        assert case.maker in ("heap", "heap_crop")
        leaves = heap_leaves(D, case.profile, case.seed)
    vol = np.empty(leaves.size, np.uint8)
    vol[leaf_order(full)] = leaves
    vol = vol.reshape(full)
    return np.ascontiguousarray(vol[:shape[0], :shape[1], :shape[2]])


def oracle_tree(O, case, vol=None, midrange=None):
    """The oracle's build of a case (the MidRangeTree one where the case's variant says so, or `midrange` does)."""
    vol = make_volume(case) if vol is None else vol
    mr = case.variant == MIDRANGE if midrange is None else midrange
    t = O.OracleTree(vol.copy(), tolerance=case.tolerance, max_epochs=case.max_epochs, midrange=mr,
                     guarded=mr or case.variant == GUARDED).build()
    t.max_epochs = case.max_epochs
    return t


def cells(O, case, tree=None, vol=None):
    """{(decision, class): [levels]} that a case reaches, the alt_epoch selection under ("alt_*", "leafless_leaf")"""
    vol = make_volume(case) if vol is None else vol
    tree = oracle_tree(O, case, vol) if tree is None else tree
    D = tree.origTreeDepth
    nskip = skipped_blocks(tree, vol, case.tolerance, case.max_epochs, case.variant)
    out = collections.defaultdict(list)
    for d, rec in decisions(tree).items():
        for cls in level_class(D, d, nskip, is_general(vol.shape), case.max_epochs):
            for e in set(rec["events"]):
                out[(e, cls)].append(d)
    a = alt_epoch(tree)
    if a and D >= 12:
        out[(a, "leafless_leaf")].append(D)
    return dict(out)


# ------------------------------------------------------------------------------------------------- the cases ----
S12, S15, S18, S19, S23 = (16, 16, 16), (32, 32, 32), (64, 64, 64), (64, 64, 128), (128, 256, 256)     # (z, y, x)
S13G = (24, 16, 40)           # general extents: D = 4 + 4 + 5 = 13


def _pair(c):
    return ("pair", c, c, 1.0)


def _case(maker, shape, profile, seed, variant=PLAIN):
    return Case(maker, shape, profile, seed, 1, 5, variant)      # one setting, so that a shape's cases batch into one set


# Found by search() on the CPU oracle (tolerance 1, five epochs), then -- for the leaf level of the 64^3 cases -- moved
# to the other shapes by hand: the entry that makes a level take a decision keeps doing so at that level of a deeper
# brick.  What each case reaches is asserted by tests/test_level_control_cpu.py against CENSUS below.
CASES = {
    # 32^3 (D = 15): levels 13 .. 15 read their partials from memory
    "m13": _case("heap", S15, ((0, _pair(4)), (12, ("ord", 3, 32, 0.077)), (13, 0)), 648366895),
    "m13e": _case("heap", S15, ((0, _pair(1)), (12, ("pair", 2, 30, 0.966)), (13, 0)), 230979756),
    "m15": _case("heap", S15, ((0, _pair(1)), (14, ("pair", 28, 25, 0.52))), 469833999),
    "w2": _case("heap", S15, ((0, 2), (5, (53, 1, 0.36)), (6, 2), (9, (50, 20, 0.55)), (10, 0), (14, 2)), 101290013),
    "dc": _case("heap", S15, ((0, _pair(4)), (2, ("pair", 13, 4, 0.958)), (3, 0), (10, ("pair", 14, 22, 0.478)), (11, 0)),
                711251474),
    # 64^3 (D = 18): the leaf level is staged in LDS, leafless, and the smallest "big" leaf level
    "l18a": _case("heap", S18, ((0, _pair(2)), (17, ("ord", 2, 10, 0.374))), 97552358),
    "l18a_guarded": _case("heap", S18, ((0, _pair(2)), (17, ("ord", 2, 10, 0.374))), 97552358, GUARDED),
    "l18b": _case("heap", S18, ((0, _pair(2)), (17, ("pair", 29, 26, 0.83))), 706148684),
    "l18c": _case("heap", S18, ((0, _pair(3)), (17, ("ord", 6, 24, 0.72))), 141665702),
    "l18d": _case("heap", S18, ((0, _pair(1)), (17, ("ord", 11, 39, 0.308))), 399304128),
    "l18e": _case("heap", S18, ((0, _pair(3)), (17, ("pair", 36, 20, 0.673))), 507391014),
    # ... with constant 4096-leaf blocks that the level loop skips
    "k18a": _case("heap_flat", S18, (((0, _pair(2)), (17, ("ord", 15, 29, 0.455))), 5, 3), 461993652),
    "k18b": _case("heap_flat", S18, (((0, _pair(4)), (17, ("ord", 22, 39, 0.205))), 5, 2), 1056309622),
    "k18c": _case("heap_flat", S18, (((0, _pair(3)), (17, ("ord", 38, 33, 0.126))), 5, 3), 189464858),
    "k17a": _case("heap_flat", S18, (((0, _pair(3)), (16, ("pair", 21, 31, 0.2)), (17, 0)), 5, 3), 465826134),
    "k17b": _case("heap_flat", S18, (((0, _pair(4)), (17, ("pair", 4, 7, 0.185))), 5, 3), 324084908),
    # ... and the tie: at level 18 the second epoch's error EQUALS the first's, bit for bit (see NEAR_TIE)
    "tie18": _case("heap_flat", S18, (((0, _pair(3)), (17, ("ord", 30, 30, 0.355))), 5, 3), 704686211),
    # 128 x 64 x 64 (D = 19): level 18 is staged and not the leaf level
    "s19a": _case("heap", S19, ((0, _pair(4)), (17, ("pair", 23, 36, 0.572)), (18, ("pair", 14, 14, 0.314))), 247450236),
    "s19b": _case("heap", S19, ((0, _pair(1)), (17, ("ord", 4, 38, 0.496)), (18, 2)), 82893332),
    "s19c": _case("heap", S19, ((0, _pair(4)), (17, ("ord", 18, 15, 0.908)), (18, 0)), 272998379),
    # 256 x 256 x 128 (D = 23), the workload's own brick: the only shape whose leaf level has 8192 partials, so that
    # k_control's chunk loop makes its second trip
    "f23a": _case("heap", S23, ((0, _pair(2)), (22, ("ord", 2, 10, 0.374))), 97552358),
    "f23b": _case("heap", S23, ((0, _pair(2)), (22, ("pair", 29, 26, 0.83))), 706148684),
    "f23d": _case("heap", S23, ((0, _pair(3)), (22, ("pair", 36, 20, 0.673))), 507391014),
    "f23c": _case("heap", S23, ((0, _pair(2)), (22, 0)), 5),          # (flat leaf level: done in its first epoch)
    # 40 x 16 x 24: general extents (D = 13), cut out of the 64 x 16 x 32 heap volume
    "g13a": _case("heap_crop", S13G, ((0, _pair(4)), (11, ("pair", 10, 14, 0.572)), (12, 0), (14, ("pair", 21, 14, 0.457))),
                  370823722),
    "g13b": _case("heap_crop", S13G, ((0, _pair(4)), (4, ("pair", 4, 33, 0.942)), (5, 1)), 954019354),
}


# (decision, class) -> (case, smallest level that counts): the census tests/test_level_control_cpu.py asserts.  The
# classes of a decision's row are the ones the issue behind these tests asks for; a None case is a cell no volume
# reached (UNREACHED says what was tried).
_B = 10        # "a level of >= 2^10 nodes"
CENSUS = {
    ("revert", "wave"): ("m13", 0), ("revert", "mem"): ("m13", 13), ("revert", "staged"): ("s19a", 18),
    ("revert", "bigleaf"): ("l18a", 18), ("revert", "skip"): ("k18a", 16), ("revert", "staged2"): ("f23a", 23),
    ("revert_then_fill", "wave"): ("m13", 0), ("revert_then_fill", "mem"): ("m13", 13),
    ("revert_then_fill", "staged"): ("s19a", 18), ("revert_then_fill", "bigleaf"): ("l18a", 18),
    ("revert_then_fill", "skip"): ("k18a", 16), ("revert_then_fill", "staged2"): ("f23a", 23),
    ("revert_final", "wave"): ("l18c", 0), ("revert_final", "mem"): ("s19a", 13), ("revert_final", "staged"): ("s19c", 18),
    ("revert_final", "bigleaf"): ("l18e", 18), ("revert_final", "skip"): ("k18c", 18),
    ("revert_final", "staged2"): ("f23d", 23),
    ("step_clamped", "wave"): ("w2", 0), ("step_clamped", "mem"): ("m13", 13), ("step_clamped", "staged"): ("s19b", 18),
    ("step_clamped", "bigleaf"): ("l18a", 18), ("step_clamped", "skip"): ("k18b", 16),
    ("step_clamped", "staged2"): ("f23a", 23),
    ("second_revert", "mem"): ("m15", _B), ("second_revert", "staged"): ("l18b", 18), ("second_revert", "skip"): ("k17b", 16),
    ("second_revert", "staged2"): ("f23b", 23),
    ("exit_small_step", "mem"): (None, _B),
    ("distance_clamped", "mem"): ("dc", _B),
    ("break_err", "mem"): ("m13", 13), ("break_err", "staged"): ("f23a", 18),
    ("epoch_limit", "wave"): ("w2", 0), ("epoch_limit", "mem"): ("m13e", 13), ("epoch_limit", "staged"): ("s19b", 18),
    ("epoch_limit", "staged2"): ("f23a", 23), ("epoch_limit", "skip"): ("tie18", 16),
    ("epoch_limit", "leafless_leaf"): ("l18a", 12), ("epoch_limit", "bigleaf"): ("l18a", 18),
    ("epoch_limit", "general"): ("g13b", 0),
    ("break_same", "wave"): ("m13", 0), ("break_same", "mem"): ("m15", 13), ("break_same", "staged"): ("s19a", 18),
    ("break_same", "staged2"): ("f23b", 23), ("break_same", "skip"): ("k18b", 16),
    ("break_same", "leafless_leaf"): ("l18b", 12), ("break_same", "bigleaf"): ("l18b", 18),
    ("break_same", "general"): ("g13a", 0),
    ("alt_minus", "leafless_leaf"): ("l18a", 12), ("alt_plus", "leafless_leaf"): ("l18c", 12),
    ("alt_neither", "leafless_leaf"): ("l18d", 12),
}
GUARD_PAIR = ("l18a", "l18a_guarded")       # one reverting case, unguarded and guarded
REUSE = ("l18a", "l18c")                    # A, B of the rebuilds on one handle: other alt selection, other revert count
NEAR_TIE = ("tie18", 18)                    # (case, level): the revert comparison there is a tie

# What the issue requires a claim for (its "these cells must be claimed"); CENSUS holds more: the 256 x 256 x 128 leaf
# level for every kind of revert, and revert_final -- the one decision after which the revert's buffer swap is visible
# at all -- in every class.  (The first set of cases had reverts at staged levels and still passed with the swap taken
# out there: each was followed by a fill, or by a second revert of a fill at the same distance.)
REQUIRED = [(dec, cls) for dec in ("revert", "revert_then_fill", "step_clamped")
            for cls in ("wave", "mem", "staged", "bigleaf", "skip")] + \
           [("second_revert", "mem"), ("exit_small_step", "mem"), ("distance_clamped", "mem"), ("break_err", "mem")] + \
           [(dec, cls) for dec in ("epoch_limit", "break_same")
            for cls in ("wave", "mem", "staged", "staged2", "skip", "leafless_leaf", "bigleaf", "general")] + \
           [(a, "leafless_leaf") for a in ALT]

UNREACHED = {
    "exit_small_step": """No level of any volume left the loop through |previousStepSize| < 0.5, and none can: previousStepSize is
    only ever set at the loop head (R.cpp:278-283), beside currentDistance = round(clamp(previousDistance +
    previousStepSize)).  previousDistance is an integer (a rounded value or 0), so a step below 0.5 gives the same
    distance and the loop breaks there (R.cpp:287, "same distance") before the while condition reads the step.  Tried
    on the CPU oracle: search() over 2000 heap volumes of 32^3 (five epochs), 1000 of 64^3 (eight epochs), 1000
    heap_flat volumes of 64^3 (three epochs), seeds 0, 0 and 1, beside the ~2700 volumes of the searches that found
    CASES: not one.  k_control's `fabs(c.previousStepSize) >= 0.5` is therefore dead code that must stay, being the
    reference's."""
}

_BUILT = {}


def built(O, name):
    """(volume, oracle tree) of case `name`, built once"""
    if name not in _BUILT:
        vol = make_volume(CASES[name])
        _BUILT[name] = (vol, oracle_tree(O, CASES[name], vol))
    return _BUILT[name]


def case_sets():
    """{(shape, tolerance, max_epochs): [names]}: the plain cases of one shape and setting, which build in one BrickSet"""
    out = collections.OrderedDict()
    for name, c in CASES.items():
        if c.variant == PLAIN:
            out.setdefault((tuple(c.shape), c.tolerance, c.max_epochs), []).append(name)
    return out


def revert_beside_inactive(decs):
    """decs: {name: decisions()} of the bricks of one set.  [(level, epoch, reverting brick, inactive brick)]: at that
    level the first brick reverts in an epoch in which the second one's loop has already ended (its epoch counter
    stopped below), so one launch of k_control holds both."""
    out = []
    for a, da in decs.items():
        for d, ra in da.items():
            for e in ra["revert_epochs"]:
                for b, db in decs.items():
                    if b != a and d in db and db[d]["epochs"] < e and "epoch_limit" not in db[d]["events"]:
                        out.append((d, e, a, b))
    return out


def class_of_level(O, name, d):
    vol, tree = built(O, name)
    c = CASES[name]
    return level_class(tree.origTreeDepth, d, skipped_blocks(tree, vol, c.tolerance, c.max_epochs, c.variant),
                       is_general(vol.shape), c.max_epochs)


def random_profile(rng, D, level=None):
    """the search's draw.  Half the time a background amplitude with one or two two-population levels; otherwise a
    target: the levels above `level` (drawn if not given) move in sibling pairs by one amount each, so each is
    reproduced exactly by its own distance, the move INTO `level` is a two-population "pair" or "ord" entry, and the
    levels below are flat or nearly so."""
    if level is None and rng.random() < 0.5:
        bg = int(rng.choice((0, 1, 2, 3, 6, 12)))
        prof = [bg] * D
        for _ in range(int(rng.integers(1, 3))):
            k = int(rng.integers(2, D))
            prof[k] = (int(rng.integers(2, 60)), int(rng.integers(0, 30)), round(float(rng.random()), 2))
            if rng.random() < 0.5:
                for j in range(k + 1, D):
                    prof[j] = int(rng.choice((0, 0, 1, 2)))
        return tuple(prof)
    L = int(rng.integers(3, D + 1)) if level is None else level
    c = int(rng.integers(1, 5))
    prof = [("pair", c, c, 1.0)] * (L - 1)
    a, b = int(rng.integers(1, 40)), int(rng.integers(1, 40))
    prof.append((str(rng.choice(("pair", "ord"))), a, b, round(float(rng.random()), 3)))
    below = int(rng.choice((0, 0, 1, 2)))
    if below == 0 and rng.random() < 0.5 and L < D:
        k = int(rng.integers(L, D))
        prof += [0] * (k - L) + [("pair", int(rng.integers(1, 30)), int(rng.integers(1, 30)), round(float(rng.random()), 3))]
    prof += [below] * (D - len(prof))
    return tuple(prof)


def search(O, shape, n, seed=0, tolerance=1, epochs=(2, 3, 5, 8), want=None, maker="heap", level=None):
    """`n` random cases of `shape` on the CPU oracle: {cell: (Case, levels)} of the first case reaching each cell, the
    closest comparison met (nearest_tie, levels of >= 2^18 nodes) and the number tried.  With `want` (a set of cells)
    it stops once all are found.  How CASES was found; the test modules do not run it."""
    rng = np.random.default_rng(seed)
    D = depth_of(_pow2_above(shape))
    found, tie = {}, None
    for i in range(n):
        prof = runs(random_profile(rng, D, level))
        if maker == "heap_flat":
            prof = (prof, D - 13, int(rng.integers(1, 4)))
        case = Case(maker, shape, prof, int(rng.integers(0, 1 << 30)), tolerance, int(rng.choice(epochs)), PLAIN)
        vol = make_volume(case)
        tree = oracle_tree(O, case, vol)
        for cell, levels in cells(O, case, tree, vol).items():
            found.setdefault(cell, (case, levels))
        t = nearest_tie(tree, 18)
        if t and (tie is None or t[0] < tie[0]):
            tie = t + (case,)
        if want and all(w in found for w in want):
            return found, tie, i + 1
    return found, tie, n
