"""Constant 4096-leaf boxes in k_prune_emit12_const, against the CPU oracle and against the same build with
`no_uniform_blocks` on (k_prune_emit12 for every box).

A constant box of a leafless SkipBlocks build is uniform: one truth, one parent reconstruction, one code and one error
per level, one grown branch for all 4096 leaves.  k_prune_emit12_const writes what k_prune_emit12 writes for it --
codes, token count, statistics, the 64 index entries, the 256 fine-index words and the string -- from about fifteen
scalars.  Everything the host can see must stay what it was: stream bytes, distance map, info and decoded voxels are
compared bit for bit with the oracle, and with the other path also at the progressive cuts that read the index entries
(D-6), the depth-(D-3) scalars, the fine index (D) and the grown branches (full depth), and through decode_lod.

Which kinds of box a case holds is read off the oracle's own stream (`_box_tokens`: preorder; a leaf's branch ends at
its first 3 or after maxTreeDepth - D tokens) and the oracle's reconstruction (`_box_classes`), and asserted.

The clamp case -- a leaf of a constant box whose error exceeds min(v, 255 - v), which takes the exact stepping loop
instead of the table -- was searched for on the CPU oracle (`_clamp_leaves`): 32x32x16 bricks of three constant
boxes drawn from 0, 1, 2, 3, 252 .. 255 and one noise box (`_noise_box` of amplitude 12, 40 and 100, centred at 128,
pushed down onto 0 or up onto 255), 40 seeds each, tolerance 1 .. 3, one to three epochs; and the families of this
file.  1002 filled boxes, none with a clamped leaf: no case here asserts it.  The path is the stepping code
k_prune_emit12 itself uses (pe_leaf_step), which the busy boxes of tests/test_gpu_ref_parity.py and
test_gpu_fullsize.py take; `test_clamp_case_census` keeps the census of this file's families, so that a change of
the volumes that brings such a box in is noticed and gets an assertion of its own."""
import numpy as np
import pytest

from test_gpu_const_boxes import (S14, S15, MIX_VALUES, _leaf_order, _refs, _outputs, _same, _against_oracle, _make, _mixed,
                                  _mixed_set)
from test_gpu_const_boxes import vr  # noqa: F401  (the module's fixture)

pytestmark = pytest.mark.gpu

EDGE_VALUES = [0, 1, 2, 3, 5, 8, 247, 250, 252, 253, 254, 255]


# ---------------------------------------------------------------- the oracle's stream, per box ----
def _tokens(ref):
    n = int(ref.numActiveNodes)
    t = np.asarray(ref.tree)
    return ((t[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n].tolist()


def _box_tokens(ref):
    """tokens of every depth-(D-12) subtree in the oracle's stream (0: under a pruned ancestor)"""
    D, chain = ref.origTreeDepth, ref.maxTreeDepth - ref.origTreeDepth
    top = D - 12
    tok = _tokens(ref)
    counts = [0] * (1 << top)

    def subtree_end(i, d):
        stack = [d]
        while stack:
            d = stack.pop()
            c = tok[i]
            i += 1
            if c == 3:
                continue
            if d < D:
                stack.append(d + 1)
                stack.append(d + 1)
            else:
                for _ in range(chain):
                    c = tok[i]
                    i += 1
                    if c == 3:
                        break
        return i

    def upper(i, d, idx):
        if d == top:
            e = subtree_end(i, d)
            counts[idx] = e - i
            return e
        c = tok[i]
        i += 1
        if c == 3:
            return i
        return upper(upper(i, d + 1, 2 * idx), d + 1, 2 * idx + 1)

    assert upper(0, 0, 0) == len(tok)
    return counts


def _box_classes(O, vol, ref):
    """per box: 'brick' (constant brick), 'skipped', 'filled' or 'busy' -- test_gpu_const_boxes._census, box by box"""
    D = ref.origTreeDepth
    nb = 1 << (D - 12)
    if int(vol.min()) == int(vol.max()):
        return ["brick"] * nb
    leaves = vol.reshape(-1)[_leaf_order(O, vol.shape)].reshape(nb, 4096)
    const = (leaves == leaves[:, :1]).all(axis=1)
    n3 = 1 << (D - 3)
    par = np.asarray(ref.recon_all)[n3 - 1:2 * n3 - 1].reshape(nb, 512)
    exact = (par == leaves[:, :1]).all(axis=1)
    return ["busy" if not c else ("skipped" if e else "filled") for c, e in zip(const, exact)]


def _clamp_leaves(O, vol, ref, tol):
    """constant boxes of a busy brick whose leaves take the exact stepping: live, and their error above min(v, 255 - v)"""
    D = ref.origTreeDepth
    nb, n = 1 << (D - 12), 1 << D
    found = 0
    leaves = vol.reshape(-1)[_leaf_order(O, vol.shape)].reshape(nb, 4096).astype(np.int64)
    rec = np.asarray(ref.recon_all)[n - 1:2 * n - 1].reshape(nb, 4096).astype(np.int64)
    for b, k in enumerate(_box_classes(O, vol, ref)):
        if k == "filled":
            v, e = int(leaves[b, 0]), int(abs(rec[b, 0] - leaves[b, 0]))
            found += e >= tol and e > min(v, 255 - v)
    return found


def _seen(O, vols, refs):
    """{(class, tokens)} over the constant boxes of the busy bricks"""
    seen = set()
    for v, r in zip(vols, refs):
        for k, n in zip(_box_classes(O, v, r), _box_tokens(r)):
            if k in ("skipped", "filled"):
                seen.add((k, n))
    return seen


def _count(O, vols, refs, pred):
    return sum(pred(k, n) for v, r in zip(vols, refs) for k, n in zip(_box_classes(O, v, r), _box_tokens(r)))


# ---------------------------------------------------------------- comparison ----
def _cuts(bs):
    D = bs.info(0)["orig_tree_depth"]
    return (D - 6, D - 3, D, bs.info(0)["max_tree_depth"])


def _decodes(bs, n):
    out = {}
    for c in _cuts(bs):
        out["cut%d" % c] = bs.decode(cut_depth=c).cpu().numpy()
    cuts = [_cuts(bs)[b % 4] for b in range(n)]
    out["lod"] = bs.decode_lod(np.array(cuts, np.int32), out=bs.decode(cut_depth=0)).cpu().numpy()
    return out


def _check(vr, O, vols, tol, ep, refs=None, concurrency=None):
    """A fresh handle on the closed-form path against the oracle and against a handle with no_uniform_blocks on."""
    vols = [np.ascontiguousarray(v) for v in vols]
    n, shape, what = len(vols), vols[0].shape, (tol, ep, concurrency)
    refs = refs if refs is not None else _refs(O, vols, tol, ep)
    on = _make(vr, n, shape, tol, ep, concurrency=concurrency).build(np.stack(vols))
    out = _against_oracle(on, vols, refs, False, what)
    off = _make(vr, n, shape, tol, ep, switches=("no_uniform_blocks",), concurrency=concurrency).build(np.stack(vols))
    _same(out, _outputs(off, n, shape, False), what)
    _same(_decodes(on, n), _decodes(off, n), what)
    for r in refs:
        assert r.zeroRunRewrites == 0
    seen = _seen(O, vols, refs)
    print("constant boxes (class, tokens) %r  %r" % (sorted(seen), what))
    return refs, seen


def _filled(seen):
    return {n for k, n in seen if k == "filled"}


# ---------------------------------------------------------------- the cases ----
_MIXED = {}


def _mixed_case(O, tol, ep):
    """(volumes, oracle builds, {(class, tokens)}) of the mixed set under one tolerance and epoch count, made once"""
    if (tol, ep) not in _MIXED:
        vols = _mixed_set(O)
        refs = _refs(O, vols, tol, ep)
        _MIXED[(tol, ep)] = (vols, refs, _seen(O, vols, refs))
    return _MIXED[(tol, ep)]


@pytest.mark.parametrize("ep", [1, 2, 3])
@pytest.mark.parametrize("tol", [1, 2, 3])
def test_mixed_set(vr, oracle, tol, ep):
    """The mixed volume of test_gpu_const_boxes: the two leaf-level string shapes at tolerance 1, boxes under a pruned
    ancestor (no token of their own) at tolerance 3, and in every combination 12 or 13 skipped boxes that emit more
    than one token (exact leaves under non-zero upper codes)."""
    vols, refs, seen = _mixed_case(oracle, tol, ep)
    _check(vr, oracle, vols, tol, ep, refs=refs)
    filled = _filled(seen)
    if tol == 1:
        assert {36863, 12287} <= filled, sorted(filled)
    if tol == 3:
        assert 0 in filled, sorted(filled)
    multi = _count(oracle, vols, refs, lambda k, n: k == "skipped" and n > 1)
    assert 12 <= multi <= 13, multi


def test_mixed_set_prunes_at_every_upper_level(oracle):
    """tolerance 2 and 3 of the sweep above: uniform boxes pruned at in-block levels 0 .. 5 (1, 3, .. 63 tokens)"""
    allf = set()
    for tol in (2, 3):
        for ep in (1, 2, 3):
            allf |= _filled(_mixed_case(oracle, tol, ep)[2])
    assert {1, 3, 7, 15, 31, 63} <= allf, sorted(allf)


EDGE_S14 = [(45, 0), (46, 1), (47, 2), (48, 3)]
EDGE_S15 = [(41, 0), (42, 3), (43, 5), (44, 7)]
FAMILIES = {"32x32x16": (S14, EDGE_S14), "32x32x32": (S15, EDGE_S15)}
_EDGE = {}


def _edge(O, name, tol, ep):
    """(volumes, oracle builds, filled boxes' token counts) of one edge-value family, made once"""
    if (name, tol, ep) not in _EDGE:
        shape, family = FAMILIES[name]
        vols = [_mixed(O, shape, s, EDGE_VALUES, busy=(b,)) for s, b in family]
        refs = _refs(O, vols, tol, ep)
        _EDGE[(name, tol, ep)] = (vols, refs, _filled(_seen(O, vols, refs)))
    return _EDGE[(name, tol, ep)]


@pytest.mark.parametrize("ep", [1, 2, 3])
@pytest.mark.parametrize("tol", [1, 2, 3])
@pytest.mark.parametrize("name", ["32x32x16", "32x32x32"])
def test_edge_values(vr, oracle, name, tol, ep):
    """Constant boxes of 0 .. 8 and 247 .. 255 around one busy box, D = 14 and 15."""
    vols, refs, filled = _edge(oracle, name, tol, ep)
    _check(vr, oracle, vols, tol, ep, refs=refs)
    if name == "32x32x16" and tol == 1:
        assert 36863 in filled, sorted(filled)
        if ep >= 2:
            assert 32767 in filled, sorted(filled)
    if name == "32x32x32" and tol >= 2 and ep == 3:
        assert 4095 in filled, sorted(filled)
    if name == "32x32x32" and tol >= 2 and ep == 1:
        assert 127 in filled, sorted(filled)


def test_edge_values_cover_the_lengths(oracle):
    """across the cases above: one token, a prune at the top of the registers' levels, the two leaf-level shapes"""
    allf = set()
    for name in FAMILIES:
        for tol in (1, 2, 3):
            for ep in (1, 2, 3):
                allf |= _edge(oracle, name, tol, ep)[2]
    assert {1, 4095, 12287, 32767, 36863} <= allf, sorted(allf)


def test_pruned_just_above_the_leaf_pairs(vr, oracle):
    """Uniform boxes pruned at in-block levels 8, 9 and 10 (511, 1023 and 2047 tokens): every thread's 16-leaf
    subtree is 1, 3 or 7 tokens.  Found by a search over seeds on the CPU oracle; tolerance 2, one epoch."""
    vols = [_mixed(oracle, S14, s, EDGE_VALUES, busy=(b,)) for s, b in ((514, 2), (594, 2), (619, 3))]
    _, seen = _check(vr, oracle, vols, 2, 1)
    assert {511, 1023, 2047} <= {n for _, n in seen}, sorted(seen)


def test_rebuilds_on_one_handle(vr, oracle):
    """A, B, A, B on one handle (the sets of test_gpu_const_boxes.test_rebuilds_on_one_handle): a stale word behind a
    shorter string, a stale fine-index word or index entry of an earlier build would show."""
    A = _mixed_set(oracle)
    B = [np.full(S15, 8, np.uint8), _mixed(oracle, S15, 21, MIX_VALUES, busy=(5,)), np.full(S15, 131, np.uint8),
         np.random.default_rng(22).integers(0, 256, S15, dtype=np.uint8), _mixed(oracle, S15, 23, [90, 200], busy=(0, 1)),
         _mixed(oracle, S15, 24, [128, 129], busy=())]
    sets = {"A": (A, _refs(oracle, A, 1, 2)), "B": (B, _refs(oracle, B, 1, 2))}
    for name, (V, R) in sets.items():
        assert len(_filled(_seen(oracle, V, R))) >= 2, name       # strings of several lengths swap places
    bs = _make(vr, len(A), S15, 1, 2)
    for name in "ABAB":
        V, R = sets[name]
        bs.build(np.stack(V))
        out = _against_oracle(bs, V, R, False, "rebuild " + name)
        fresh = _make(vr, len(V), S15, 1, 2).build(np.stack(V))
        _same(out, _outputs(fresh, len(V), S15, False), "rebuild %s against a fresh handle" % name)
        _same(_decodes(bs, len(V)), _decodes(fresh, len(V)), "rebuild %s against a fresh handle" % name)


@pytest.fixture(scope="module")
def sixty_four(oracle):
    rng = np.random.default_rng(31)
    vols = []
    for b in range(64):
        if b % 4 == 0:
            vols.append(np.full(S14, int(rng.integers(0, 256)), np.uint8))
        else:
            vols.append(_mixed(oracle, S14, 100 + b, MIX_VALUES + EDGE_VALUES, busy=(b % 4,)))
    return vols, _refs(oracle, vols, 1, 2)


@pytest.mark.parametrize("streams", [1, 4])
def test_set_concurrency(vr, oracle, sixty_four, streams):
    """64 bricks of 32x32x16, constant bricks between mixed ones: the closed-form launch follows the join of the brick
    ranges' level loops and does not depend on how many there were."""
    vols, refs = sixty_four
    _, seen = _check(vr, oracle, vols, 1, 2, refs=refs, concurrency=streams)
    assert any(k == "skipped" for k, _ in seen) and len(_filled(seen)) >= 2, sorted(seen)


def test_clamp_case_census(oracle):
    """The families of this file hold no constant box whose leaves take the exact stepping (module docstring); a
    change of the volumes that brings one in should turn this into a case with its own assertion."""
    found = 0
    for tol in (1, 2, 3):
        for name in FAMILIES:
            vols, refs, _ = _edge(oracle, name, tol, 2)
            for v, r in zip(vols, refs):
                found += _clamp_leaves(oracle, v, r, tol)
    print("constant boxes with clamped leaves: %d" % found)
    assert found == 0
