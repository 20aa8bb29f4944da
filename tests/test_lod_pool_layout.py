"""vr_lod_pool_layout (host only, no device): the layout of a level-of-detail pool against a NumPy restatement of the
rule written in include/vrhip.h, its error cases, and the premise it rests on (a progressive cut is constant on the
layout's boxes)."""
import numpy as np
import pytest

from volumerenderer_amd import _lib
from volumerenderer_amd.render import POOL_ENTRY, default_camera, default_params, lod_pool_layout, select_lod


def split_counts(dims, cut):
    """Splits per axis among depths 0 .. cut-1 of buildRecursive's split-axis rule (R.cpp:151-159): depth d splits
    axis d % 3, or the next one while the box has more than one voxel and extent 1 on that axis."""
    ext = [int(q) for q in dims]
    n = [0, 0, 0]
    for d in range(cut):
        sd, i = d % 3, 0
        while ext[0] * ext[1] * ext[2] > 1 and ext[sd] == 1:
            i += 1
            sd = (d + i) % 3
        ext[sd] //= 2
        n[sd] += 1
    return n


def rule(dims, ijk, grid, cuts, otd):
    """include/vrhip.h, vr_lod_pool_layout, restated: (table, pool_bytes)."""
    lg = [int(q).bit_length() - 1 for q in dims]
    table = np.zeros(int(np.prod(grid)), POOL_ENTRY)
    table["offset"] = -1
    run = 0
    for b, c in enumerate(cuts):
        if c < 0:
            continue
        sh = [0, 0, 0]
        if c < otd:
            n = split_counts(dims, c)
            sh = [lg[k] - n[k] for k in range(3)]
        off = (run + 255) // 256 * 256
        run = off + int(np.prod([int(dims[k]) >> sh[k] for k in range(3)]))
        i, j, k = ijk[b]
        cell = i + grid[0] * (j + grid[1] * k)
        table[cell]["offset"] = off
        table[cell]["shift"] = sh
    return table, run


def depth(dims):
    return sum(int(q).bit_length() - 1 for q in dims)


SHAPES = [(256, 256, 128), (32, 32, 32), (64, 16, 32), (16, 1, 8), (1, 1, 1)]


def test_bench_brick_shifts():
    """The 256 x 256 x 128 brick (D = 23) at the cuts the start camera uses."""
    dims = (256, 256, 128)
    ijk = np.zeros((1, 3), np.int64)
    for cut, want in [(20, (1, 1, 1)), (21, (1, 1, 0)), (22, (0, 1, 0)), (23, (0, 0, 0)), (30, (0, 0, 0))]:
        t, n = lod_pool_layout(dims, ijk, (1, 1, 1), [cut], 23, 30)
        assert tuple(t[0]["shift"]) == want, cut
        assert n == 256 * 256 * 128 >> sum(want)


@pytest.mark.parametrize("dims", SHAPES)
def test_layout_matches_numpy_rule(dims):
    rng = np.random.default_rng(sum(dims))
    D = depth(dims)
    M = D + 7
    grid = (3, 2, 4)
    cells = [(i, j, k) for k in range(grid[2]) for j in range(grid[1]) for i in range(grid[0])]
    for trial in range(6):
        B = int(rng.integers(1, len(cells) + 1))
        pick = rng.permutation(len(cells))[:B]                    # random order, sparse cells
        ijk = np.array([cells[p] for p in pick], np.int64)
        if trial == 0:
            cuts = np.array([(b % (M + 2)) - 1 for b in range(B)], np.int32)   # every value in -1 .. M
        else:
            cuts = rng.integers(-1, M + 1, B).astype(np.int32)
        got, n = lod_pool_layout(dims, ijk, grid, cuts, D, M)
        want, wn = rule(dims, ijk, grid, cuts, D)
        assert n == wn, (trial, n, wn)
        assert np.array_equal(got["offset"], want["offset"]), trial
        assert np.array_equal(got["shift"], want["shift"]), trial
        assert np.all(got["pad"] == 0)
    # every cut in one brick each
    for c in range(-1, M + 1):
        got, n = lod_pool_layout(dims, np.zeros((1, 3), np.int64), (1, 1, 1), [c], D, M)
        want, wn = rule(dims, np.zeros((1, 3), np.int64), (1, 1, 1), [c], D)
        assert n == wn and np.array_equal(got, want), c


def test_invalid_layouts():
    dims, D, M = (32, 32, 32), 15, 22
    ijk = np.array([(0, 0, 0), (1, 0, 0)], np.int64)
    ok = np.array([M, 3], np.int32)
    lod_pool_layout(dims, ijk, (2, 1, 1), ok, D, M)

    def bad(**kw):
        a = dict(brick_dims=dims, brick_ijk=ijk, grid=(2, 1, 1), cuts=ok, orig_tree_depth=D, max_tree_depth=M)
        a.update(kw)
        with pytest.raises(_lib.VrError) as e:
            lod_pool_layout(*a.values())
        assert e.value.status == -1, kw     # VR_ERR_INVALID

    bad(brick_ijk=np.array([(0, 0, 0), (0, 0, 0)], np.int64))           # two bricks on one cell
    bad(brick_ijk=np.array([(0, 0, 0), (2, 0, 0)], np.int64))           # outside the grid
    bad(brick_ijk=np.array([(0, 0, 0), (-1, 0, 0)], np.int64))
    bad(cuts=np.array([M + 1, 0], np.int32))                            # cut outside -1 .. M
    bad(cuts=np.array([-2, 0], np.int32))
    bad(brick_dims=(48, 32, 32), orig_tree_depth=15)                    # not a power of two
    bad(brick_dims=(96, 80, 40), orig_tree_depth=6 + 6 + 5)
    bad(orig_tree_depth=D + 1)                                          # not the depth of the dims
    bad(max_tree_depth=D - 1)
    bad(grid=(0, 1, 1))


@pytest.mark.parametrize("shape,seed", [((16, 16, 16), 1), ((8, 16, 32), 2), ((32, 4, 8), 3)])
def test_progressive_cut_is_constant_on_layout_boxes(oracle, shape, seed):
    """The premise: levelCutProgressive(c) of the oracle is constant on every 2^shift box of the layout (shape is
    (Z, Y, X)), for every cut."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    vol = np.clip(100 + 60 * np.sin(0.5 * x + 0.3 * y) + 40 * np.cos(0.4 * z) + rng.integers(0, 20, shape), 0, 255).astype(np.uint8)
    ref = oracle.OracleTree(vol.copy(), tolerance=1, max_epochs=2).build()
    dims = (shape[2], shape[1], shape[0])
    D = ref.origTreeDepth
    assert D == depth(dims)
    for c in range(0, D + 1):
        t, _ = lod_pool_layout(dims, np.zeros((1, 3), np.int64), (1, 1, 1), [c], D, ref.maxTreeDepth)
        sx, sy, sz = (int(v) for v in t[0]["shift"])
        a = np.asarray(ref.levelCutProgressive(c)).reshape(shape)
        mn = a.reshape(shape[0] >> sz, 1 << sz, shape[1] >> sy, 1 << sy, shape[2] >> sx, 1 << sx)
        assert np.all(mn == mn[:, :1, :, :1, :, :1]), c


def test_start_camera_pool_is_small():
    """The bench geometry (8 x 8 x 15 bricks of 256 x 256 x 128) at the start camera, 1920 x 1080, tolerance 1."""
    bd, grid, D, M = (256, 256, 128), (8, 8, 15), 23, 30
    B = grid[0] * grid[1] * grid[2]
    ijk = np.array([(b % 8, (b // 8) % 8, b // 64) for b in range(B)], np.int64)
    cuts = select_lod(default_camera(), default_params(1920, 1080, bd), bd, ijk, grid, D, M, 1.0)
    t, n = lod_pool_layout(bd, ijk, grid, cuts, D, M)
    want, wn = rule(bd, ijk, grid, cuts, D)
    assert n == wn and np.array_equal(t, want)
    V = bd[0] * bd[1] * bd[2]
    assert n <= 0.25 * 2 * B * V, n
    assert np.any((cuts >= 0) & (cuts < D))
