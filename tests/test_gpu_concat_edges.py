"""k_concat12 -- the contiguous stream that tree(), save() and every reopened file consist of -- with k_block_alive,
k_emit_zero and k_brick_offsets, at the length and alignment edges of its paths, byte for byte against the CPU oracle.

A workgroup of the kernel splices 16 consecutive 4096-leaf blocks (spine + string each) into the stream at 2-bit
granularity: blocks of at most 32 tokens by one lane over one, two or three words, longer ones through a list of
16-byte chunks; words two blocks share are merged in LDS, a workgroup's first and last word by atomicOr.  Which of
these cases a volume reaches depends on its token counts, so the contents here are designed and then *read*:
tests/streamlayout.py parses the oracle's stream into the blocks' (offset, spine, string) triples and sorts them into
the kernel's cases, tests/test_stream_layout_cpu.py asserts that every case occurs in the sets below, and a failing
comparison here names the first differing byte, the block that owns it and that block's cases.

Shapes are the smallest with the path: one block, four (a partial workgroup), 16 (exactly one workgroup), 64 (four)."""
import numpy as np
import pytest

import streamlayout as SL
from test_gpu_const_boxes import MIX_VALUES, _against_oracle, _from_leaves, _make, _mixed, _noise_box, _outputs, _refs, _same
from test_gpu_const_boxes import vr  # noqa: F401  (the module's fixture)
from test_gpu_index_batched import RUNS, _runs

pytestmark = pytest.mark.gpu

S12 = (16, 16, 16)          # (z, y, x): D = 12, one block
S14 = (16, 32, 32)          # D = 14, four blocks
S16 = (32, 32, 64)          # D = 16, 16 blocks: exactly one workgroup
S18 = (64, 64, 64)          # D = 18, 64 blocks: four workgroups
SHAPES = {"16x16x16": S12, "32x32x16": S14, "64x32x32": S16, "64x64x64": S18}
EPOCHS = 2


def _nblk(shape):
    return shape[0] * shape[1] * shape[2] // 4096


def _sparse(O, shape, seed, noise=(), kmax=3, vals=(128, 129, 131), amp=40):
    """Constant boxes of `vals` with up to `kmax` leaves moved by up to +-amp (box 0: at least one), boxes `noise` are
    noise: strings of a few tokens to a few hundred, the lengths at which the one-lane path and the chunk list meet."""
    rng = np.random.default_rng(seed)
    nb = _nblk(shape)
    leaves = np.repeat(rng.choice(vals, nb), 4096).reshape(nb, 4096).astype(np.int64)
    for b in range(nb):
        if b in noise:
            leaves[b] = _noise_box(rng)
            continue
        k = int(rng.integers(0, kmax + 1))
        k = max(k, 1) if b == 0 else k
        pos = rng.choice(4096, k, replace=False)
        leaves[b, pos] += rng.integers(1, amp + 1, k) * rng.choice([-1, 1], k)
    return _from_leaves(O, np.clip(leaves, 0, 255).reshape(-1).astype(np.uint8), shape)


def _noise(shape, seed):
    return np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8)


def _halves(O, shape, lo=100, hi=140):
    """the leaves' lower half `lo`, the upper half `hi`: a stream of a handful of tokens, all of them above the blocks
    where there is more than one block"""
    n = shape[0] * shape[1] * shape[2]
    return _from_leaves(O, np.repeat(np.array([lo, hi], np.uint8), n // 2), shape)


def _shape_set(O, shape):
    """The bricks of test_shapes: one busy box among dead ones (a long string, then single `3`s that share a word),
    uniform strings of 3 .. 255 tokens beside noise (`_mixed`), sparse boxes, plain noise (every block long), a
    constant brick between them, and a brick whose whole stream fits one word."""
    nb = _nblk(shape)
    vols = [_runs(O, shape, (0,), 1), _mixed(O, shape, 4, MIX_VALUES, busy=(nb // 2,)), np.full(shape, 8, np.uint8),
            _sparse(O, shape, 5, noise=(nb // 3,)), _sparse(O, shape, 6), _noise(shape, 9), _halves(O, shape)]
    if nb >= 4:
        vols.append(_runs(O, shape, (nb - 1,), 3))          # the only long block is the last one
    if nb == 64:
        # an empty workgroup behind a busy one, a workgroup whose only token is its first block's, dead runs
        vols += [_runs(O, shape, (16,), 2), _runs(O, shape, (15,), 3), _runs(O, shape, RUNS, 4),
                 _mixed(O, shape, 6, MIX_VALUES, busy=RUNS), _sparse(O, shape, 7, noise=(21, 40), kmax=8)]
    return vols


def _full_set(O):
    """Tolerance 0 at 64^3: nothing is pruned.  Noise (every workgroup takes a second trip through its chunk list),
    constant boxes behind 48 noise boxes (a workgroup whose 16 blocks are all 36863 tokens, the longest string there
    is) and constant boxes of several values behind 16."""
    return [_noise(S18, 9), _mixed(O, S18, 4, [90, 200], busy=tuple(range(48))),
            _mixed(O, S18, 4, MIX_VALUES, busy=tuple(range(16))), _noise(S18, 10)]


def _short_set(O):
    """64^3 bricks of short strings, for the same handle as _full_set"""
    return [_sparse(O, S18, 5, noise=(21,)), _mixed(O, S18, 4, MIX_VALUES, busy=(32,)), _runs(O, S18, (0,), 1),
            _sparse(O, S18, 6)]


def _batched_set(O):
    """seven bricks, constant ones first, in the middle and last"""
    return [np.full(S18, 8, np.uint8), _noise(S18, 9), _runs(O, S18, (0,), 1), np.full(S18, 0, np.uint8),
            _mixed(O, S18, 4, MIX_VALUES, busy=(32,)), _sparse(O, S18, 5, noise=(21,)), np.full(S18, 255, np.uint8)]


# name -> (volumes, tolerance, midrange)
CASES = {"full": (_full_set, 0, False), "short": (_short_set, 4, False), "batched": (_batched_set, 1, False)}
for _name, _shape in SHAPES.items():
    for _tol in (1, 4):
        CASES["%s tol %d" % (_name, _tol)] = (lambda O, s=_shape: _shape_set(O, s), _tol, False)
for _name in ("32x32x16", "64x32x32"):
    CASES["%s midrange" % _name] = (lambda O, s=SHAPES[_name]: _shape_set(O, s), 1, True)

_CACHE = {}
_LAYOUT = {}


def case(O, name):
    """(volumes, oracle trees, tolerance, midrange) of a content set: computed once, shared by the tests, never changed"""
    if name not in _CACHE:
        make, tol, midrange = CASES[name]
        vols = [np.ascontiguousarray(v) for v in make(O)]
        _CACHE[name] = (vols, _refs(O, vols, tol, EPOCHS, midrange), tol, midrange)
    return _CACHE[name]


def layouts(O, name):
    """the block layout of every brick of a set, from the oracle's (mid) stream"""
    if name not in _LAYOUT:
        _LAYOUT[name] = [SL.layout(r.tree, r.numActiveNodes, r.origTreeDepth) for r in case(O, name)[1]]
    return _LAYOUT[name]


def is_constant(vol, tol):
    """a brick the closed form serves: no kernel of the stream assembly touches it"""
    return tol >= 1 and int(vol.min()) == int(vol.max())


def _streams(bs, O, name, what):
    """every brick's stream bytes against the oracle's; a difference is named by byte, block and class"""
    vols, refs, tol, midrange = case(O, name)
    for b, ref in enumerate(refs):
        pairs = [("tree", bs.tree(b), ref.tree)]
        if midrange:
            pairs.append(("tree_range", bs.tree_range(b), ref.tree_range))
        for which, got, want in pairs:
            if not np.array_equal(got, want):
                pytest.fail("%s: %s of brick %d of '%s': %s" % (what, which, b, name, SL.describe(layouts(O, name)[b], got, want)))


def _check(bs, O, name, what):
    vols, refs, tol, midrange = case(O, name)
    _streams(bs, O, name, what)
    return _against_oracle(bs, vols, refs, midrange, what)


def _build(vr, O, name, compaction=None):
    vols, refs, tol, midrange = case(O, name)
    bs = _make(vr, len(vols), vols[0].shape, tol, EPOCHS, midrange)
    if compaction is not None:
        bs.set_compaction(compaction)
    return bs.build(np.stack(vols))


# ---------------------------------------------------------------- the cases ----
@pytest.mark.parametrize("shape", list(SHAPES))
def test_shapes(vr, oracle, shape):
    """One block, four, one workgroup, four workgroups, at tolerances 1 and 4."""
    for tol in (1, 4):
        name = "%s tol %d" % (shape, tol)
        _check(_build(vr, oracle, name), oracle, name, name)


def test_tolerance_zero(vr, oracle):
    """Nothing pruned: strings of up to 36863 tokens, 16 of them in one workgroup, a second trip through the chunks."""
    _check(_build(vr, oracle, "full"), oracle, "full", "tolerance 0")


def compact_bytes(ref):
    """what k_brick_offsets reserves for a stream: its words and a spare one, rounded up to 16 bytes"""
    return ((((ref.numActiveNodes + 15) >> 4) + 1) * 4 + 15) & ~15


def test_batched_bricks_and_constant_bricks(vr, oracle):
    """Seven bricks in one set, constant ones first, in the middle and last: the bricks' streams lie back to back at
    offsets that k_brick_offsets sums from their lengths, and a constant brick's is one closed-form word."""
    vols, refs, tol, _ = case(oracle, "batched")
    const = [is_constant(v, tol) for v in vols]
    assert const == [True, False, False, True, False, False, True]
    sizes = [compact_bytes(r) for r in refs]
    assert len({s for s, c in zip(sizes, const) if not c}) == 4 and all(s == 16 for s, c in zip(sizes, const) if c), sizes
    _check(_build(vr, oracle, "batched"), oracle, "batched", "seven bricks")


@pytest.mark.parametrize("name", ["64x64x64 tol 1", "full"])
def test_lazy_and_on_build_compaction(vr, oracle, name):
    """set_compaction(0): the build leaves the strings in their slots and the first tree() assembles the stream;
    set_compaction(1): the build ends with it.  Both equal the oracle and each other."""
    a = _check(_build(vr, oracle, name, compaction=0), oracle, name, "lazy compaction")
    b = _check(_build(vr, oracle, name, compaction=1), oracle, name, "compaction on build")
    _same(a, b, "lazy against on-build compaction")


def test_forced_64_bit_offsets(vr, oracle, monkeypatch):
    """VRHIP_FORCE_IDX64 (read when a set is created): the blocks' token offsets come from the 64-bit scan."""
    monkeypatch.setenv("VRHIP_FORCE_IDX64", "1")
    for name in ("64x64x64 tol 1", "64x64x64 tol 4"):
        _check(_build(vr, oracle, name), oracle, name, name + ", 64-bit offsets")


@pytest.mark.parametrize("shape", ["32x32x16", "64x32x32"])
def test_midrange_range_stream(vr, oracle, shape):
    """Variant 2: the second launch (k_concat12<true>) writes the range stream at the mid stream's offsets with its own
    strings and spine; both streams against the oracle's MidRangeTree."""
    name = "%s midrange" % shape
    _check(_build(vr, oracle, name), oracle, name, name)


def test_compact_buffer_grows_on_a_later_build(vr, oracle):
    """The compact buffer is sized at the first assembly (5/8 byte per voxel and a little) and regrown when a build's
    streams do not fit: short strings first, then tolerance-0 noise, which takes three times the first size (the
    kernels write nothing, the host regrows and repeats), then short strings again."""
    n = len(case(oracle, "full")[0])
    guess = n * (S18[0] * S18[1] * S18[2] // 8 * 5 + 64) + 4096
    assert sum(compact_bytes(r) for r in case(oracle, "short")[1]) < guess < sum(compact_bytes(r) for r in case(oracle, "full")[1])
    bs = _make(vr, n, S18, 0, EPOCHS)
    for step, name in enumerate(("short", "full", "short")):
        vols, _, tol, _ = case(oracle, name)
        bs.set_error_tolerance(tol)
        bs.build(np.stack(vols))
        _check(bs, oracle, name, "build %d ('%s') on one handle" % (step, name))


def shrinking_blocks(O):
    """(brick, block) pairs whose string in 'full' is longer than in 'short': long -> a short string that ends inside a
    word, and long -> a shorter long string that ends inside a word (the bits behind it in the slot are stale)"""
    to_short, to_long = [], []
    for b, (f, s) in enumerate(zip(layouts(O, "full"), layouts(O, "short"))):
        for k in range(f["cnt"].size):
            cf, cs = int(f["cnt"][k]), int(s["cnt"][k])
            if cf > 32 and 1 <= cs < 32 and cs % 16:
                to_short.append((b, k))
            if cf > cs > 32 and cs % 16:
                to_long.append((b, k))
    return to_short, to_long


@pytest.mark.parametrize("compaction", [1, 0], ids=["on_build", "lazy"])
def test_one_handle_long_short_long(vr, oracle, compaction):
    """One handle: tolerance-0 noise (every slot full), short strings (stale bits behind every one of them in the
    slots; the compact buffer is used to a fraction), noise again, short again.  Every build equals the oracle and a
    fresh handle."""
    to_short, to_long = shrinking_blocks(oracle)
    assert to_short and to_long, (len(to_short), len(to_long))
    n = len(case(oracle, "full")[0])
    assert len(case(oracle, "short")[0]) == n
    bs = _make(vr, n, S18, 0, EPOCHS)
    bs.set_compaction(compaction)
    for step, name in enumerate(("full", "short", "full", "short")):
        vols, _, tol, _ = case(oracle, name)
        bs.set_error_tolerance(tol)
        bs.build(np.stack(vols))
        what = "build %d ('%s') on one handle, compaction %d" % (step, name, compaction)
        out = _check(bs, oracle, name, what)
        fresh = _build(vr, oracle, name, compaction=compaction)
        _same(out, _outputs(fresh, n, S18, False), what + ", against a fresh handle")
