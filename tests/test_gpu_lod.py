"""View-dependent level-of-detail decode on the GPU: vr_brickset_decode_lod (a cut per brick, -1 = skipped) against the
uniform decode and the oracle, calls queued without host synchronisation, and the culling contract of vr_lod_select
(a frame drawn from a LOD decode equals the frame drawn from the full decode)."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FILL = 0xA5
GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def rm_like(shape, seed=3):
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    h = shape[0] / 2 + 3 * np.sin(x * 0.4) + 2 * np.cos(y * 0.23)
    v = 128 + 120 * np.tanh((z - h) / 3.0) + rng.integers(0, 3, shape)
    return np.clip(v, 0, 255).astype(np.uint8)


def cut_pool(D, M):
    """A cut of every kernel class: skipped, above the index level (k_cut_values first), the fine / tile kernels,
    the region / quad kernels (>= D-3), the grown-branch levels."""
    Ds = D - min(D, 6)
    pool = [-1, 0, 3, Ds - 1, Ds, D - 3, D - 1, D, M - 1, M]
    return sorted({c for c in pool if c == -1 or 0 <= c <= M})


def lod(vr, bs, cuts, stream=None):
    import torch
    out = torch.full((bs.num_bricks * bs.voxels_per_brick,), FILL, dtype=torch.uint8, device="cuda")
    bs.decode_lod(cuts, out=out, stream=stream)
    return out


def check_lod(vr, bs, refs=None, rounds=None, seed=0):
    """Round r gives brick b the cut pool[(r + b) % len(pool)] (every brick sees every cut over the rounds), then one
    random round.  Every decoded brick equals the uniform decode at its cut, skipped bricks keep the fill, and the
    bricks with an oracle tree (refs: {brick: OracleTree}) equal levelCutProgressive at their cut."""
    import torch
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    pool = cut_pool(D, M)
    B, V = bs.num_bricks, bs.voxels_per_brick
    uni = {}

    def uniform(c):
        if c not in uni:
            uni[c] = bs.decode(cut_depth=c).cpu().numpy().reshape(B, V).copy()
        return uni[c]

    rng = np.random.default_rng(seed)
    plans = [[pool[(r + b) % len(pool)] for b in range(B)] for r in range(rounds or len(pool))]
    plans.append(list(rng.choice(pool, B)))
    seen = set()
    for cuts in plans:
        got = lod(vr, bs, np.array(cuts, np.int32)).cpu().numpy().reshape(B, V)
        torch.cuda.synchronize()
        for b, c in enumerate(cuts):
            if c < 0:
                assert np.all(got[b] == FILL), ("skipped brick written", b)
                continue
            assert np.array_equal(got[b], uniform(c)[b]), (b, c)
            if refs and b in refs and (b, c) not in seen:
                seen.add((b, c))
                want = refs[b].levelCut() if c == M else refs[b].levelCutProgressive(c)
                assert np.array_equal(got[b], want.reshape(-1)), ("oracle", b, c)
    if refs:
        for b in refs:
            assert {c for (bb, c) in seen if bb == b} == set(pool) - {-1}
    return D, M


def test_lod_8_bricks_64cubed(vr, oracle):
    """64^3 bricks: the lane kernel."""
    rng = np.random.default_rng(21)
    vols = [rm_like((64, 64, 64), s) for s in range(4)] + [rng.integers(0, 256, (64, 64, 64), dtype=np.uint8)]
    vols += [np.full((64, 64, 64), 9, np.uint8), rm_like((64, 64, 64), 9)[::-1].copy(), rm_like((64, 64, 64), 11).transpose(2, 1, 0).copy()]
    bs = vr.BrickSet(8, (64, 64, 64), 1, 2)
    bs.build(np.stack(vols))
    refs = {b: oracle.OracleTree(vols[b].copy(), tolerance=1, max_epochs=2).build() for b in (0, 4)}
    check_lod(vr, bs, refs)


@pytest.fixture(scope="module")
def bench_set(vr, oracle):
    """Four bench-shaped bricks (256 x 256 x 128, the bench's field): the region kernel at full depth, the fine kernel
    at shallower cuts, k_cut_values above the index level."""
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    bd = (256, 256, 128)
    vox = bench.make_volume_gpu(torch, (256, 256, 512), bd, seed=12345, kind="rm_volume")
    host = vox.cpu().numpy()
    bs = vr.BrickSet(4, bd, 1, 2)
    bs.build(vox.reshape(-1))
    b = int(np.argmax([len(np.unique(host[i])) for i in range(4)]))      # a brick with the interface in it
    return bs, {b: oracle.OracleTree(host[b].copy(), tolerance=1, max_epochs=2).build()}


def test_lod_bench_bricks(vr, bench_set):
    bs, refs = bench_set
    check_lod(vr, bs, refs)


def test_lod_bench_bricks_quad_and_walk(vr, bench_set):
    """The same per-brick decode through the quad kernel (VRHIP_DECODE_QUAD) and the walking tile kernel."""
    bs, _ = bench_set
    for sw in ("decode_quad", "decode_walk"):
        bs.set_switch(sw, 1)
        try:
            check_lod(vr, bs, rounds=4, seed=5)
        finally:
            bs.set_switch(sw, 0)


def test_lod_all_full_depth_equals_decode(vr, bench_set):
    bs, _ = bench_set
    M = bs.info(0)["max_tree_depth"]
    got = lod(vr, bs, np.full(bs.num_bricks, M, np.int32)).cpu().numpy()
    assert np.array_equal(got, bs.decode().cpu().numpy())


def test_lod_general_extents(vr, oracle):
    shape = (40, 80, 96)
    vols = [rm_like(shape, 2), rm_like(shape, 7)[:, ::-1].copy()]
    bs = vr.BrickSet(2, (96, 80, 40), 1, 2)
    bs.build(np.stack(vols))
    check_lod(vr, bs, {1: oracle.OracleTree(vols[1].copy(), tolerance=1, max_epochs=2).build()})


def test_lod_midrange_mid_stream(vr, oracle):
    shape = (16, 32, 128)
    vols = [rm_like(shape, 4), rm_like(shape, 5)[::-1].copy(), np.full(shape, 200, np.uint8)]
    bs = vr.BrickSet(3, (128, 32, 16), 2, 2, vr.VARIANT_MIDRANGE)
    bs.build(np.stack(vols))
    ref = oracle.OracleTree(vols[0].copy(), tolerance=2, max_epochs=2, midrange=True, guarded=True).build()
    check_lod(vr, bs, {0: ref})


def test_lod_opened_golden_file(vr, oracle):
    """A set opened from the reference-written file: cuts above the index level come from the host parse."""
    p = os.path.join(GOLD, "ref_sphere_n3_16_tol1_ep2.tree.bin")
    bs = vr.BrickSet.open(p)
    check_lod(vr, bs, {0: oracle.OracleTree.open(p)})


def test_lod_rejects_bad_cuts(vr, bench_set):
    import torch
    bs, _ = bench_set
    M = bs.info(0)["max_tree_depth"]
    out = torch.full((bs.num_bricks * bs.voxels_per_brick,), FILL, dtype=torch.uint8, device="cuda")
    for bad in (-2, M + 1):
        cuts = np.full(bs.num_bricks, M, np.int32)
        cuts[1] = bad
        with pytest.raises(vr.VrError):
            bs.decode_lod(cuts, out=out)
    with pytest.raises(ValueError):
        bs.decode_lod(np.full(bs.num_bricks - 1, M, np.int32), out=out)
    torch.cuda.synchronize()
    assert bool((out == FILL).all())                    # nothing was launched


def _expected(bs, cuts, uni):
    V = bs.voxels_per_brick
    e = np.full((bs.num_bricks, V), FILL, np.uint8)
    for b, c in enumerate(cuts):
        if c >= 0:
            e[b] = uni[c][b]
    return e.reshape(-1)


def test_lod_back_to_back_one_stream_and_two_streams(vr, bench_set):
    """Calls queued with no host synchronisation between them each read their own lists, cut values and tables:
    different cuts of the same bricks in the fine class (per-cut tables) and above the index level (cut values)."""
    import torch
    bs, _ = bench_set
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    Ds = D - 6
    cutsA = np.array([Ds - 2, Ds + 1, D - 4, M], np.int32)
    cutsB = np.array([Ds - 1, Ds + 2, -1, D - 5], np.int32)
    cutsC = np.array([M, -1, Ds - 3, Ds + 3], np.int32)
    uni = {int(c): bs.decode(cut_depth=int(c)).cpu().numpy().reshape(bs.num_bricks, -1).copy()
           for c in set(cutsA) | set(cutsB) | set(cutsC) if c >= 0}
    n = bs.num_bricks * bs.voxels_per_brick
    bufs = [torch.full((n,), FILL, dtype=torch.uint8, device="cuda") for _ in range(6)]
    torch.cuda.synchronize()
    # one stream, back to back (more calls than the ring has slots: the fifth waits for the first on the host)
    s0 = torch.cuda.current_stream()
    plan = [cutsA, cutsB, cutsC, cutsB, cutsA, cutsC]
    for buf, cuts in zip(bufs, plan):
        bs.decode_lod(cuts, out=buf, stream=s0)
    torch.cuda.synchronize()
    for buf, cuts in zip(bufs, plan):
        assert np.array_equal(buf.cpu().numpy(), _expected(bs, cuts, uni))
    # two streams of one set
    for buf in bufs:
        buf.fill_(FILL)
    torch.cuda.synchronize()
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    for i, (buf, cuts) in enumerate(zip(bufs[:4], [cutsA, cutsB, cutsC, cutsA])):
        bs.decode_lod(cuts, out=buf, stream=s1 if i % 2 == 0 else s2)
    torch.cuda.synchronize()
    for buf, cuts in zip(bufs[:4], [cutsA, cutsB, cutsC, cutsA]):
        assert np.array_equal(buf.cpu().numpy(), _expected(bs, cuts, uni))


# ---- rendering: the culling contract of vr_lod_select

GRID, BD = (4, 4, 4), (32, 32, 32)


@pytest.fixture(scope="module")
def render_set(vr):
    """A 128^3 volume as 64 bricks of 32^3 in a 4 x 4 x 4 grid."""
    full = rm_like((128, 128, 128), 6)
    ijk = np.array([(i, j, k) for k in range(4) for j in range(4) for i in range(4)], np.int64)
    bricks = np.stack([full[k * 32:(k + 1) * 32, j * 32:(j + 1) * 32, i * 32:(i + 1) * 32] for i, j, k in ijk])
    bs = vr.BrickSet(64, BD, 1, 2)
    bs.build(bricks.copy())
    return bs, ijk


CAMERAS = [  # (pos, front, fov)
    ((0.25, 0.2, -0.6), (0.0, 0.0, 1.0), 20.0),
    ((-0.3, 0.0, -0.7), (0.5, 0.0, 1.0), 15.0),
    ((0.0, 0.0, 1.2), (0.15, -0.1, -1.0), 12.0),
    ((0.1, -0.15, -0.9), (0.2, 0.1, 1.0), 25.0),
    ((0.0, 0.0, 0.2), (0.0, 0.0, 1.0), 50.0),       # inside the cube: the bricks behind it are culled (and the frame is empty)
]


def _cam(vr, pos, front, fov):
    cam = vr.default_camera()
    f = np.array(front) / np.linalg.norm(front)
    cam.pos[:], cam.front[:], cam.fov_deg = pos, tuple(float(v) for v in f), fov
    return cam


def _frame(vr, bricks, ijk, cam, P, skip):
    vol = vr.assemble_bricks(bricks, BD, ijk, GRID)
    if skip:
        vr.use_skip_grid(P, vr.build_skip_grid(vol, (128, 128, 128), 8), 8)
    else:
        vr.use_skip_grid(P, None)
    return vr.raycast(vol, (128, 128, 128), cam, P).cpu().numpy()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("skip", [False, True])
def test_culled_bricks_are_never_read(vr, render_set, mode, skip):
    import torch
    bs, ijk = render_set
    info = bs.info(0)
    full = bs.decode()
    total, shown = 0, 0
    for pos, front, fov in CAMERAS:
        cam = _cam(vr, pos, front, fov)
        P = vr.default_params(160, 120, BD, mode)
        cuts = vr.select_lod(cam, P, BD, ijk, GRID, info["orig_tree_depth"], info["max_tree_depth"], 1e-6)
        assert np.all((cuts == -1) | (cuts == info["max_tree_depth"]))
        assert np.any(cuts >= 0), cuts
        total += int(np.sum(cuts == -1))
        buf = torch.full((bs.num_bricks * bs.voxels_per_brick,), 0xFF, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=buf)
        want = _frame(vr, full, ijk, cam, P, skip)
        got = _frame(vr, buf, ijk, cam, P, skip)
        assert np.array_equal(got, want), (pos, np.abs(got - want).max())
        shown += int(np.any(want != want[0, 0]))
    assert total >= 64 and shown >= 3, (total, shown)


# max |frame - full frame| over the pixels and channels for the two cameras below, as this test printed it on an
# MI355X: 0.182818 at pixel tolerance 1, 0.493927 at 4 (the decode is exact, so the figure is deterministic); the
# bound is that measurement rounded up
COARSE_BOUND = {1.0: 0.19, 4.0: 0.50}


@pytest.mark.parametrize("tol", [1.0, 4.0])
def test_coarse_render_error_is_bounded(vr, render_set, tol):
    import torch
    bs, ijk = render_set
    info = bs.info(0)
    full = bs.decode()
    worst, coarser = 0.0, 0
    for pos, front, fov in [((0.0, 0.0, -2.0), (0.0, 0.0, 1.0), 50.0), ((0.4, 0.3, -1.2), (-0.3, -0.2, 1.0), 40.0)]:
        cam = _cam(vr, pos, front, fov)
        P = vr.default_params(96, 72, BD, 0)
        cuts = vr.select_lod(cam, P, BD, ijk, GRID, info["orig_tree_depth"], info["max_tree_depth"], tol)
        coarser += int(np.sum((cuts >= 0) & (cuts < info["max_tree_depth"])))
        buf = torch.zeros(bs.num_bricks * bs.voxels_per_brick, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=buf)
        got = _frame(vr, buf, ijk, cam, P, False)
        want = _frame(vr, full, ijk, cam, P, False)
        worst = max(worst, float(np.abs(got - want).max()))
    print("coarse render: tolerance %.1f, max |diff| %.6f, coarser bricks %d" % (tol, worst, coarser))
    assert coarser > 0
    bound = COARSE_BOUND[tol]
    assert worst <= bound, worst


def test_draw_lod_keeps_its_volume(vr, render_set):
    """HeadlessViewer.draw_lod: select, decode, assemble, draw; the frame is the full decode's, and a brick culled in
    a frame keeps what an earlier frame decoded into it."""
    from volumerenderer_amd.viewer import HeadlessViewer
    bs, ijk = render_set
    V = bs.voxels_per_brick
    full = bs.decode().cpu().numpy().reshape(bs.num_bricks, V)
    v = HeadlessViewer(160, 120)
    frame, cuts = v.draw_lod(bs, ijk, GRID, pixel_tolerance=1e-6)
    M = bs.info(0)["max_tree_depth"]
    assert np.all((cuts == -1) | (cuts == M)) and np.any(cuts == M)
    want = vr.raycast(vr.assemble_bricks(bs.decode(), BD, ijk, GRID), (128, 128, 128), v.camera(),
                      vr.default_params(160, 120, BD, 0, float(v.currIsoVal) / 255.0)).cpu().numpy()
    assert np.array_equal(frame.cpu().numpy(), want)
    keep = v._lodBricks
    before = keep.cpu().numpy().reshape(bs.num_bricks, V).copy()
    v.cameraPos = np.array([0.0, 0.0, 0.2], np.float32)          # inside: the bricks behind are culled
    frame2, cuts2 = v.draw_lod(bs, ijk, GRID, pixel_tolerance=1e-6)
    assert np.any(cuts2 == -1) and v._lodBricks is keep
    after = v._lodBricks.cpu().numpy().reshape(bs.num_bricks, V)
    for b in range(bs.num_bricks):
        assert np.array_equal(after[b], before[b] if cuts2[b] < 0 else full[b]), b
    assert np.any(cuts == M) and np.any((cuts == M) & (cuts2 == -1))   # some kept brick holds the first frame's decode
