"""Many-brick sets: a case builder for the batch axis (test infrastructure only).

Every codec kernel runs over a batch of B bricks, and what a large B can break -- a carry between scan rounds, a brick
range that is one off, a list entry in the wrong row -- corrupts SOME bricks of a set.  The sets built here make that
visible at any B for the cost of a few dozen oracle runs:

  - PERIOD distinct brick contents per shape; brick b holds content (b + rot) % PERIOD.  PERIOD is coprime with 16, 32, 64
    and 1024, so brick b never equals bricks b +- 1, 16, 32, 64 or 1024: a result that lands on a neighbour, a brick range
    shifted by a part, a wave or a scan round, is a mismatch.
  - every fourth content (0, 4, .. 36) is a constant brick (the closed-form paths), the others are not, so both kinds sit
    within SEAM_WINDOW bricks on each side of any seam.
  - the oracle runs once per content and settings (Expect); the expected result of a B-brick set is those results tiled.

Shapes are (X, Y, Z) as vr_brickset_create takes them; volumes are [Z][Y][X] arrays."""
import json
import math
import os

import numpy as np

PERIOD = 37
STEPS = (1, 16, 32, 64, 1024)       # distances at which two bricks of a set must differ
SEAM_WINDOW = 4                     # bricks on each side of a seam that must hold a constant and a non-constant brick
CONST_EVERY = 4

# the shapes, the smallest on each code path
FUSED = (16, 16, 16)                # D = 12: the smallest fused build (k_prune_emit12, the compact streams)
UNFUSED = (8, 8, 8)                 # D = 9: k_prune_leaf, k_prune_level, k_emit_count, k_emit_write
GENERAL = (12, 6, 5)                # general extents: the table-driven kernels
TINY = (2, 2, 2)                    # the brick-count limit only

# B of the (16,16,16) sets and what each is there for (DESIGN.md repeats this table)
FUSED_B = {
    1: "the single-brick set every other test builds, as the base line",
    31: "below the level-loop split at two parts (B < 32)",
    32: "the first B that splits in two; ranges 0..16, 16..32",
    33: "two parts of unequal length, 2 does not divide B",
    63: "below the split at four parts (B < 64), three parts of 21",
    64: "the first B that splits in four; one wave of the offset scan, full",
    65: "the offset scan's second wave; four parts of 16, 16, 16 and 17 bricks",
    67: "a prime: no part count divides it",
    1023: "one scan round of k_brick_offsets, one brick short of full",
    1024: "one full scan round, the carry written and never read",
    1025: "the second scan round: one brick past the carry",
    2049: "the third scan round: a carry of a carry",
    3000: "a ragged third round, 2 * 1024 + 952",
}
OTHER_B = (33, 1025)                # the unfused and general-extent sets
MIDRANGE_B = (65, 1025)
CONCURRENCY = (1, 2, 3, 4)

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


# ---- geometry, restated from vrhip.h ---------------------------------------------------------------------------------
def depth(dims):
    """origTreeDepth: the sum of the floors of the three log2."""
    return sum(int(v).bit_length() - 1 for v in dims)


def max_depth(dims):
    return depth(dims) + 7


def index_depth(dims):
    """Ds: the depth of the decode index (4x4x4-voxel subtrees: K = min(D, 6) levels above the leaves)."""
    D = depth(dims)
    return D - min(D, 6)


def is_general(dims):
    return any(v & (v - 1) or v > 1024 for v in dims)


_TILE_OK = {}


def _tile_ok(dims):
    """TilePlan::ok of a power-of-two shape, from the golden plans (tests/golden/decode_plans.json)."""
    if not _TILE_OK:
        for p in json.load(open(os.path.join(GOLD, "decode_plans.json")))["plans"]:
            _TILE_OK[tuple(p[:3])] = bool(p[3][0])
    return _TILE_OK[tuple(dims)]


def decode_class(dims, cut):
    """What a per-brick decode does with a brick cut at `cut`: ("skip",) or (kernel, scalars from above the index level).
    The kernel is DecodePlan::kernel's choice (kd_decode.hip) for a built set with no debugging switch."""
    if cut < 0:
        return ("skip",)
    D = depth(dims)
    if is_general(dims):
        k = "general"
    elif not _tile_ok(dims):
        k = "lane"
    else:
        k = "region" if cut >= D - 3 else "fine"
    return (k, cut < index_depth(dims))


def decode_classes(dims):
    """Every class a per-brick decode of this shape has."""
    return {decode_class(dims, c) for c in range(-1, max_depth(dims) + 1)}


def cut_pool(dims):
    """A cut of every class and at every edge: skipped, the root, above / at the index level, around D, the grown-branch
    levels."""
    D, M, Ds = depth(dims), max_depth(dims), index_depth(dims)
    return sorted({c for c in (-1, 0, 3, Ds - 1, Ds, D - 3, D - 1, D, M - 1, M) if -1 <= c <= M})


def cut_pattern(dims, B, rot=0):
    """cuts[b] cycles through cut_pool: the period (9 or 10) is coprime with PERIOD, so over 37 * 10 bricks every content
    meets every cut, and every class's list holds every tenth brick or so -- hundreds of non-contiguous bricks at B = 1025."""
    pool = cut_pool(dims)
    assert math.gcd(len(pool), PERIOD) == 1
    return np.array([pool[(b + rot) % len(pool)] for b in range(B)], np.int32)


def uniform_cuts(dims):
    """The cuts of the uniform decode: the root, either side of the index level, D, and full depth."""
    D, M, Ds = depth(dims), max_depth(dims), index_depth(dims)
    return sorted({c for c in (0, Ds - 1, Ds, D, M) if 0 <= c <= M})


# ---- the level-loop split, restated from encode() (kd_encode.hip) ----------------------------------------------------
def parts_of(B, concurrency, midrange=False):
    parts = min(int(concurrency), 4)
    if midrange or B < 16 * parts or parts < 2:
        parts = 1
    return parts


def part_bounds(B, parts):
    return [B * p // parts for p in range(parts + 1)]


def seams(B, midrange=False):
    """Every brick index s of a B-brick set at which something changes between bricks s - 1 and s: the level-loop ranges
    for every concurrency tested, a wave (64) and a round (1024) of the offset scan, a staged pool pass (32)."""
    s = set()
    for c in CONCURRENCY:
        s.update(part_bounds(B, parts_of(B, c, midrange))[1:-1])
    s.update(k for k in (32, 64, 1024, 2048) if k < B)
    return sorted(s)


# ---- contents --------------------------------------------------------------------------------------------------------
def rm_like(shape, seed):
    """The smooth interface field of tests/test_gpu_lod.py, on any extents."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    h = shape[0] / 2 + 3 * np.sin(x * 0.4 + seed) + 2 * np.cos(y * 0.23 + 2 * seed)
    v = 128 + 120 * np.tanh((z - h) / 3.0) + rng.integers(0, 3, shape)
    return np.clip(v, 0, 255).astype(np.uint8)


def sphere(shape, seed, noise_mask):
    rng = np.random.default_rng(seed)
    c = rng.uniform(-0.15, 0.15, 3)
    g = np.meshgrid(*[(np.arange(s) + 0.5) / s - 0.5 - c[i] for i, s in enumerate(shape)], indexing="ij")
    r = np.sqrt(sum(a * a for a in g)) * 2.0
    v = np.clip(255.0 * (1.0 - r), 0, 255).astype(np.int64)
    if noise_mask:
        v = v + (rng.integers(0, 256, shape) & noise_mask)
    return np.clip(v, 0, 255).astype(np.uint8)


def one_voxel(shape, base, value, where):
    """A constant brick with one other voxel.  At extents that are not powers of two a leaf reads the min corner of a box
    of several cells (vrhip.h), so most voxels are never read: there "last" is x = X / 2 of the first row and "middle"
    (X / 2, Y / 2, Z / 2), min corners of the first splits' upper halves, which every deeper level keeps."""
    v = np.full(shape, base, np.uint8)
    flat = v.reshape(-1)
    pow2 = all(s & (s - 1) == 0 for s in shape)
    flat[{"first": 0, "last": flat.size - 1 if pow2 else shape[2] // 2,
          "middle": shape[2] // 2 + shape[2] * (shape[1] // 2 + shape[1] * (shape[0] // 2))}[where]] = value
    return v


CONSTANTS = (0, 255, 1, 254, 77, 128, 200, 16, 3, 100)       # contents 0, 4, 8 .. 36


def _others(shape):
    """The 27 non-constant contents, in the order they are dealt between the constants."""
    rng = np.random.default_rng(sum(shape) * 1000 + shape[2])
    out = []
    for k in range(5):
        out.append(("noise%d" % k, rng.integers(0, 256, shape, dtype=np.uint8)))
    for k in range(8):
        v = rm_like(shape, k + 1)
        out.append(("rm_like%d" % k, v if k % 2 == 0 else v[::-1, :, ::-1].copy()))
    for k in range(5):
        out.append(("sphere%d" % k, sphere(shape, 40 + k, (0, 7, 3, 0, 15)[k])))
    out.append(("one_voxel_first", one_voxel(shape, 0, 255, "first")))
    out.append(("one_voxel_last", one_voxel(shape, 255, 0, "last")))
    out.append(("one_voxel_middle", one_voxel(shape, 90, 91, "middle")))
    out.append(("one_voxel_far", one_voxel(shape, 60, 200, "last")))
    out.append(("small_0_1", rng.integers(0, 2, shape, dtype=np.uint8)))
    out.append(("small_0_3", rng.integers(0, 4, shape, dtype=np.uint8)))
    out.append(("small_0_7", rng.integers(0, 8, shape, dtype=np.uint8)))
    out.append(("small_ramp", (rm_like(shape, 12) >> 5).astype(np.uint8)))
    out.append(("small_sphere", (sphere(shape, 50, 0) >> 6).astype(np.uint8)))
    assert len(out) == PERIOD - len(CONSTANTS)
    # mix the kinds along the order: neighbours in the set are of different kinds
    order = [(i * 7) % len(out) for i in range(len(out))]
    assert sorted(order) == list(range(len(out)))
    return [out[i] for i in order]


_CONTENTS = {}


def contents(dims):
    """(names, volumes): the PERIOD contents of a shape, volumes a (PERIOD, Z, Y, X) uint8 array, pairwise different.  On
    extents too small for a generator to give distinct fields (2x2x2) a repeat is replaced by noise."""
    dims = tuple(int(v) for v in dims)
    if dims not in _CONTENTS:
        shape = (dims[2], dims[1], dims[0])
        rest = iter(_others(shape))
        rng = np.random.default_rng(dims[0] + 7)
        names, vols = [], []
        for i in range(PERIOD):
            if i % CONST_EVERY == 0:
                n, v = "const%d" % CONSTANTS[i // CONST_EVERY], np.full(shape, CONSTANTS[i // CONST_EVERY], np.uint8)
            else:
                n, v = next(rest)
                while v.min() == v.max() or any(np.array_equal(v, w) for w in vols):
                    n, v = n + "_noise", rng.integers(0, 256, shape, dtype=np.uint8)
            names.append(n)
            vols.append(v)
        _CONTENTS[dims] = (names, np.stack(vols))
    return _CONTENTS[dims]


def is_constant(i):
    """Content i (brick b holds content (b + rot) % PERIOD) is a constant brick."""
    return i % PERIOD % CONST_EVERY == 0


def content_of(B, rot=0):
    return (np.arange(B) + rot) % PERIOD


def voxels(dims, B, rot=0):
    """The B bricks of a set, back to back: a (B, Z*Y*X) uint8 array."""
    return contents(dims)[1].reshape(PERIOD, -1)[content_of(B, rot)]


def check_builder(dims, B, midrange=False):
    """The conditions the sets rest on (the CPU module asserts them for every set the GPU module builds)."""
    assert all(math.gcd(PERIOD, k) == 1 for k in (16, 32, 64, 1024))
    assert all(k % PERIOD for k in STEPS)
    vols = contents(dims)[1]
    for i in range(PERIOD):
        assert (vols[i].min() == vols[i].max()) == is_constant(i), i
        for j in range(i):
            assert not np.array_equal(vols[i], vols[j]), (i, j)
    c = content_of(B)
    for k in STEPS:
        assert not np.any(c[k:] == c[:-k]) if k < B else True
    for s in seams(B, midrange):
        # (a side the set's end cuts short -- brick 1024 of 1025 -- holds what it can; the seam as a whole still has both)
        both = set()
        for side in (range(max(s - SEAM_WINDOW, 0), s), range(s, min(s + SEAM_WINDOW, B))):
            kinds = {is_constant(c[b]) for b in side}
            assert kinds == {True, False} or (kinds and len(side) < SEAM_WINDOW), (B, s, list(side))
            both |= kinds
        assert both == {True, False}, (B, s)


# ---- the oracle's results, once per content ------------------------------------------------------------------------
class Expect:
    """The oracle's results for the PERIOD contents of one shape and one setting; tiled() spreads any of them over B."""

    def __init__(self, O, dims, tolerance=1, max_epochs=2, midrange=False):
        self.dims = tuple(int(v) for v in dims)
        self.tolerance, self.max_epochs, self.midrange = tolerance, max_epochs, midrange
        self.D, self.M = depth(dims), max_depth(dims)
        vols = contents(dims)[1]
        self.trees = [O.OracleTree(v.copy(), tolerance=tolerance, max_epochs=max_epochs, midrange=midrange,
                                   guarded=midrange).build() for v in vols]
        assert all((t.origTreeDepth, t.maxTreeDepth) == (self.D, self.M) for t in self.trees)
        self.num_active = np.array([t.numActiveNodes for t in self.trees], np.int64)
        self.tree = [t.tree.copy() for t in self.trees]
        self.dmap = [t.distanceMap.copy() for t in self.trees]
        if midrange:
            self.tree_range = [t.tree_range.copy() for t in self.trees]
            self.dmap_range = [t.distanceMap_range.copy() for t in self.trees]
        self._cut, self._cut_range = {}, {}

    def cut(self, c):
        """(PERIOD, V): every content decoded at cut c (-1 or M: the reference's levelCut)."""
        c = self.M if c < 0 else int(c)
        if c not in self._cut:
            self._cut[c] = np.stack([(t.levelCut() if c == self.M else t.levelCutProgressive(c)).reshape(-1).copy()
                                     for t in self.trees])
        return self._cut[c]

    def cut_range(self, c):
        c = self.M if c < 0 else int(c)
        if c not in self._cut_range:
            self._cut_range[c] = np.stack([t.levelCutRange(c).reshape(-1).copy() for t in self.trees])
        return self._cut_range[c]

    def decode(self, B, c=-1, rot=0):
        return self.cut(c)[content_of(B, rot)]

    def decode_range(self, B, c=-1, rot=0):
        return self.cut_range(c)[content_of(B, rot)]

    def decode_lod(self, B, cuts, fill, rot=0):
        """(B, V): brick b at cuts[b], a skipped brick all `fill`."""
        V = self.cut(-1).shape[1]
        out = np.full((B, V), fill, np.uint8)
        who = content_of(B, rot)
        for c in sorted(set(int(q) for q in cuts)):
            if c >= 0:
                m = np.asarray(cuts) == c
                out[m] = self.cut(c)[who[m]]
        return out


# ---- the compact stream layout (vrhip.h: the streams of all bricks back to back, 16-byte aligned, one spare word) -----
def compact_bytes(num_active):
    """Bytes brick b's contiguous stream takes in the compact buffer: ceil(numActive / 16) words and a spare one, rounded
    up to 16 bytes."""
    n = int(num_active)
    return (((n + 15) // 16 + 1) * 4 + 15) // 16 * 16


def compact_offsets(num_active):
    """offsets[b] for b = 0 .. B (the last is the total), one brick after the other."""
    off = [0]
    for n in num_active:
        off.append(off[-1] + compact_bytes(n))
    return off


def compact_offsets_in_rounds(num_active, round_size=1024, wave=64):
    """The same offsets the way k_brick_offsets (kd_encode.hip) finds them: rounds of 1024 bricks with a carry, each round
    an inclusive scan per wave of 64 plus the totals of the waves before."""
    B = len(num_active)
    off, carry = [0] * (B + 1), 0
    for base in range(0, B, round_size):
        sizes = [compact_bytes(num_active[b]) if b < B else 0 for b in range(base, base + round_size)]
        incl, part = [], []
        for w in range(0, round_size, wave):
            run = 0
            for t in range(w, w + wave):
                run += sizes[t]
                incl.append(run)
            part.append(run)
        before = 0
        for t in range(round_size):
            before = carry + sum(part[:t // wave])
            if base + t < B:
                off[base + t] = before + incl[t] - sizes[t]
        carry = before + incl[round_size - 1]
    off[B] = carry
    return off
