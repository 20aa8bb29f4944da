"""GPU parity of k_fill16's batched skip flags and two-deep chunk loop (and of k_est_summ beside it, on the same
flags) against the CPU oracle: tree bytes, distance map, numActiveNodes, reverts and decoded voxels, bit for bit.

k_fill16 reads the flag bytes of all chunks of a workgroup in its prologue, walks only its live chunks with two chunks
of inputs in flight, and stores the per-chunk error sums and the level D-2 flag bits after the loop.  What can go
wrong is which chunk a bit belongs to, where the live chunks start, stop and run out, and what a skipped chunk's slots
hold afterwards -- so the volumes put skipped 4096-leaf boxes at chosen places of the leaf-level workgroups, and `_runs`
checks on the oracle's own reconstruction that they came out skipped there.

Shapes: the smallest that reach every (kernel, chunks per workgroup) pair the host launches -- 32x32x16 (D 14: one chunk
everywhere), 64^3 (D 18: the leaf fill at 4), 128^3 (D 21: the leaf fill at 8, the storing fill at 4), 256x128x128 (D 22:
the storing fill at 8).  The two small shapes take every (tolerance, epochs) pair of {0, 1, 4} x {1, 2, 3}: tolerance 0
has no flags at all, one epoch no central difference, two the fill-less leaf epoch, three reach reverts.  The two large
ones take each value once, (0, 1), (1, 2), (4, 3): their oracle trees cost a second each."""
import numpy as np
import pytest

from test_gpu_const_boxes import MIX_VALUES, _against_oracle, _census, _from_leaves, _leaf_order, _make, _mixed, _noise_box, _refs

pytestmark = pytest.mark.gpu

SHAPES = [(16, 32, 32), (64, 64, 64), (128, 128, 128), (128, 128, 256)]      # (z, y, x)
IDS = ["32x32x16", "64x64x64", "128x128x128", "256x128x128"]
ALL_PARAMS = [(tol, ep) for ep in (1, 2, 3) for tol in (0, 1, 4)]
FEW_PARAMS = [(0, 1), (1, 2), (4, 3)]
CASES = [pytest.param(s, p, id="%s-tol%d-ep%d" % (i, p[0], p[1]))
         for s, i in zip(SHAPES, IDS) for p in (ALL_PARAMS if s[0] * s[1] * s[2] <= (1 << 18) else FEW_PARAMS)]

# box kinds per 4096-leaf box in leaf order, tiled over the brick: S constant at the noise boxes' midrange (comes out
# skipped), N noise.  "filled" is the mixed pattern of test_gpu_const_boxes: constant boxes of several values around
# plain noise boxes, of which some come out exact (skipped) and the others not (filled), side by side.
CONTENT_NAMES = ["noise", "runs", "wg_skipped", "filled"]
TILES = {"runs": "SNSSNSSS" "NSSSSNNS",                    # skipped runs of 1, 2, 3, 4; first and last chunk skipped
         "wg_skipped": "NSSSSSSS" "SSSSSSSS" "SSSSSSSN" "NNSSSSNN"}
LO, HI = 100, 156


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _iters_leaf(shape):
    """chunks per k_fill16 workgroup at the leaf level (a chunk there is one 4096-leaf box)"""
    nb = shape[0] * shape[1] * shape[2] // 4096
    return 8 if nb >= 512 else (4 if nb >= 64 else 1)


def _tiled(O, shape, name, seed):
    rng = np.random.default_rng(seed)
    nb = shape[0] * shape[1] * shape[2] // 4096
    tile = TILES[name]
    # A few noise boxes, reused.  Each spans exactly LO .. HI: every node above the boxes then has the midrange 128 as
    # its truth and is reconstructed exactly, so an S box meets its value at its root whatever its neighbours are, and
    # the skipped boxes sit where the tile puts them.
    noise = []
    for _ in range(4):
        box = np.clip(_noise_box(rng), LO, HI)
        box[0], box[1] = LO, HI
        noise.append(box)
    leaves = np.empty((nb, 4096), np.int64)
    for b in range(nb):
        kind = tile[b % len(tile)]
        leaves[b] = noise[b % 4] if kind == "N" else 128
    return _from_leaves(O, leaves.reshape(-1).astype(np.uint8), shape)


_CONTENTS = {}


def _contents(O, shape):
    if shape not in _CONTENTS:
        vols = [np.random.default_rng(1).integers(0, 256, shape, dtype=np.uint8)]
        vols += [_tiled(O, shape, name, 10 + i) for i, name in enumerate(CONTENT_NAMES[1:3])]
        nb = shape[0] * shape[1] * shape[2] // 4096
        vols.append(_mixed(O, shape, 12, MIX_VALUES, busy=range(min(5, nb - 1), nb, 16)))
        _CONTENTS[shape] = vols
    return _CONTENTS[shape]


def _skipped_boxes(O, vol, ref):
    """per 4096-leaf box in leaf order: constant, and every depth-(D-2) truth equal to its parent's reconstruction"""
    D = ref.origTreeDepth
    nb = 1 << (D - 12)
    leaves = vol.reshape(-1)[_leaf_order(O, vol.shape)].reshape(nb, 4096)
    const = (leaves == leaves[:, :1]).all(axis=1)
    n3 = 1 << (D - 3)
    par = np.asarray(ref.recon_all)[n3 - 1:2 * n3 - 1].reshape(nb, 512)
    return const & (par == leaves[:, :1]).all(axis=1)


def _runs(sk, iters):
    """of the leaf-level workgroups (`iters` boxes each): lengths of the skipped runs inside partly skipped ones, how
    many of those have their first and last chunk skipped, and how many are skipped entirely"""
    lengths, ends, whole = set(), 0, 0
    for g in sk.reshape(-1, iters):
        if g.all():
            whole += 1
            continue
        ends += int(g[0] and g[-1])
        run = 0
        for s in list(g) + [False]:
            if s:
                run += 1
            elif run:
                lengths.add(run)
                run = 0
    return dict(lengths=sorted(lengths), first_and_last=ends, whole=whole)


_REFS = {}


def _shared_refs(O, shape, tol, ep):
    """the oracle trees of a shape's volumes and of a constant brick, computed once per (shape, tolerance, epochs)"""
    key = (shape, tol, ep)
    if key not in _REFS:
        vols = _contents(O, shape) + [np.full(shape, 128, np.uint8)]
        _REFS[key] = (vols, _refs(O, vols, tol, ep))
    return _REFS[key]


@pytest.mark.parametrize("shape,params", CASES)
def test_contents(vr, oracle, shape, params):
    """Noise, skipped runs, whole skipped workgroups and filled boxes as four bricks of one set; then runs, a constant
    brick and the filled boxes as a set of three."""
    tol, ep = params
    vols, refs = _shared_refs(oracle, shape, tol, ep)
    what = (shape, tol, ep)
    iters = _iters_leaf(shape)
    for name, v, r in zip(CONTENT_NAMES, vols, refs):
        runs = _runs(_skipped_boxes(oracle, v, r), iters)
        census = _census(oracle, v, r)
        print("%-10s boxes %r  leaf workgroups of %d: %r  reverts %d" % (name, census, iters, runs, r.numReverts))
        if tol == 0 or iters == 1:
            continue        # (tolerance 0: the flags are off; one chunk per workgroup: nothing to run through)
        if name == "noise":
            assert census["skipped"] == 0, (what, census)
        if name == "runs":
            assert set(runs["lengths"]) >= {1, 2, 3} | ({4} if iters == 8 else set()) and runs["first_and_last"] > 0, (what, runs)
        if name == "wg_skipped":
            assert runs["whole"] > 0 and runs["lengths"], (what, runs)
        if name == "filled":
            assert census["filled"] > 0 and census["skipped"] > 0, (what, census)
    four = _make(vr, 4, shape, tol, ep).build(np.stack(vols[:4]))
    _against_oracle(four, vols[:4], refs[:4], False, what)
    pick = [1, 4, 3]                # skipped runs, the constant brick, filled boxes
    three = _make(vr, 3, shape, tol, ep).build(np.stack([vols[i] for i in pick]))
    _against_oracle(three, [vols[i] for i in pick], [refs[i] for i in pick], False, what + ("three",))


@pytest.mark.parametrize("shape", SHAPES[1:3], ids=IDS[1:3])
def test_one_handle_rebuilt(vr, oracle, shape):
    """Busy, constant-heavy, busy again on one handle: a flag byte or a per-chunk slot left from the build before
    would show in the third build."""
    vols, refs = _shared_refs(oracle, shape, 1, 2)
    flipped = vols[0][::-1].copy()
    busy = ([vols[0], vols[1], flipped], [refs[0], refs[1]] + _refs(oracle, [flipped], 1, 2))
    heavy = ([vols[2], vols[4], vols[3]], [refs[2], refs[4], refs[3]])
    bs = _make(vr, 3, shape, 1, 2)
    for step, (V, R) in enumerate((busy, heavy, busy)):
        bs.build(np.stack(V))
        _against_oracle(bs, V, R, False, (shape, "rebuild", step))
