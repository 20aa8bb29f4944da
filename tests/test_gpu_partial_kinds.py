"""The algebra of the three kinds of partial image -- grey (c, tau, covered, 0), colour (C.r, C.g, C.b, T) and projection
(v, n, 0, 0), the last with max, min and mean -- pinned bit for bit on seeded synthetic partials, without any marching:

  (a) the slab call on n slabs == pairwise folds in the pixel's view order, then the kind's finish;
  (b) the slab call on a row tile with first_pixel == those rows of the whole-frame result;
  (c) the compositor at world = 1 == the slab call with one slab.

Frames are 16 pixels wide and 1, 4 and 17 rows high: 16 pixels (less than a wave), 64, and 272 (across the edge of a
256-thread block).  The three cameras have a slab order that is known without computing the view basis: with up =
(0, 1, 0), front = (0, 0, 1) gives s = (-1, 0, 0) and u = (0, 1, 0) exactly, so along axis 2 every pixel's d is 1
(ascending), with front = (0, 0, -1) it is -1 (descending), and along axis 0 it is -nx tanX: never zero for an even width,
ascending in the left half of the frame and descending in the right half."""
import functools

import pytest

pytestmark = pytest.mark.gpu

W = 16
HEIGHTS = (1, 4, 17)
SLABS = (1, 2, 5)
KINDS = ("grey", "colour", "max", "min", "mean")
# (front, axis, order): "asc", "desc" or "split" (columns px < W / 2 ascending, the rest descending)
CAMERAS = (((0.0, 0.0, 1.0), 2, "asc"), ((0.0, 0.0, -1.0), 2, "desc"), ((0.0, 0.0, 1.0), 0, "split"))
TILE = (5, 12)      # rows [lo, hi) of the 17-row frame


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@functools.lru_cache(maxsize=None)
def partials(kind, H):
    """max(SLABS) seeded partial images [slab][H * W][4] of `kind` on the GPU; never written to."""
    import torch
    n, npix = max(SLABS), H * W
    g = torch.Generator().manual_seed(1000 * KINDS.index(kind) + H)
    p = torch.zeros((n, npix, 4), dtype=torch.float32)
    if kind in ("grey", "colour"):
        channels = 1 if kind == "grey" else 3
        p[..., :channels] = torch.rand((n, npix, channels), generator=g)                # c or C in [0, 1)
        p[..., channels] = 1.0 - torch.rand((n, npix), generator=g)                     # tau or T in (0, 1]
        if kind == "grey":
            p[..., 2] = (torch.rand((n, npix), generator=g) < 0.6).float()
            p[:, ::5, 2] = 0.0                                                          # uncovered in every slab
            assert (p[..., 2].sum(0) == 0).any() and (p[..., 2].sum(0) > 0).any()
    else:
        p[..., 0] = torch.rand((n, npix), generator=g)
        p[:, 1::9, 0] = 1.0                                                             # v in [0, 1], both ends
        p[:, 2::9, 0] = 0.0
        p[..., 1] = torch.randint(0, 4, (n, npix), generator=g).float()                 # n: 0..3 samples
        p[:, ::7, 1] = 0.0                                                              # no sample in any slab
        p[..., 0] *= (p[..., 1] > 0).float()                                            # n = 0: the row is all zero
        assert (p[..., 1].sum(0) == 0).any() and (p[..., 1] == 0).any() and (p[..., 1] > 0).any()
    return p.cuda()


@functools.lru_cache(maxsize=None)
def finisher(vr, kind):
    """What finishes `kind`: None, a TransferFunction (its background) or a Projection (window and background)."""
    import torch
    if kind == "grey":
        return None
    if kind == "colour":
        return vr.TransferFunction(torch.zeros((256, 4)), background=(0.25, 0.5, 0.75))
    return vr.Projection(kind, window=(0.125, 0.875), background=(0.1, 0.2, 0.3))


def camera(vr, front):
    cam = vr.default_camera()
    cam.pos[:], cam.front[:], cam.up[:] = (0.0, 0.0, -0.75), front, (0.0, 1.0, 0.0)
    return cam


def slab_call(vr, kind, stack, first, axis, cam, P):
    from volumerenderer_amd import distributed as D
    stack = stack.contiguous()
    if kind == "grey":
        return D._gpu_combine(stack, first, axis, cam, P)
    if kind == "colour":
        return D._gpu_combine_tf(stack, first, axis, cam, P, finisher(vr, kind))
    return D._gpu_combine_proj(stack, finisher(vr, kind))


def fold_and_finish(vr, kind, stack, order):
    """Pairwise folds of the slabs `order` names, front first, then the finish."""
    acc = stack[order[0]].clone()
    for k in order[1:]:
        if kind == "grey":
            vr.composite_over(acc, stack[k])
        elif kind == "colour":
            vr.composite_over_tf(acc, stack[k])
        else:
            vr.composite_combine_proj(acc, stack[k], finisher(vr, kind))
    if kind == "grey":
        return vr.composite_finish(acc)
    if kind == "colour":
        return vr.composite_finish_tf(acc, finisher(vr, kind))
    return vr.composite_finish_proj(acc, finisher(vr, kind))


def expected(vr, kind, stack, order, H):
    """Law (a)'s right-hand side for a camera of the slab order `order`; a projection always folds ascending."""
    import torch
    n = stack.shape[0]
    asc = fold_and_finish(vr, kind, stack, list(range(n)))
    if order == "asc" or kind not in ("grey", "colour"):
        return asc
    desc = fold_and_finish(vr, kind, stack, list(range(n - 1, -1, -1)))
    if order == "desc":
        return desc
    left = (torch.arange(H * W, device=stack.device) % W < W // 2)[:, None]
    return torch.where(left, asc, desc)


@pytest.mark.parametrize("n", SLABS)
@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
def test_slab_call_equals_pairwise_folds_in_view_order(vr, kind, H, n):
    import torch
    stack = partials(kind, H)[:n]
    P = vr.default_params(W, H, (64, 64, 64))
    for front, axis, order in CAMERAS:
        got = slab_call(vr, kind, stack, 0, axis, camera(vr, front), P)
        want = expected(vr, kind, stack, order, H)
        assert not torch.isnan(got).any()
        assert torch.equal(got, want), (kind, H, n, front, axis)
    if n > 1 and kind in ("grey", "colour"):      # "over" does not commute: the pins above tell the two orders apart
        assert not torch.equal(expected(vr, kind, stack, "asc", H), fold_and_finish(vr, kind, stack, list(range(n - 1, -1, -1))))


@pytest.mark.parametrize("n", SLABS)
@pytest.mark.parametrize("kind", KINDS)
def test_slab_call_on_a_row_tile_equals_those_rows_of_the_frame(vr, kind, n):
    import torch
    H, (lo, hi) = 17, TILE
    stack = partials(kind, H)[:n]
    P = vr.default_params(W, H, (64, 64, 64))
    for front, axis, _ in CAMERAS:
        cam = camera(vr, front)
        whole = slab_call(vr, kind, stack, 0, axis, cam, P)
        tile = slab_call(vr, kind, stack[:, lo * W:hi * W], lo * W, axis, cam, P)
        assert tile.shape == ((hi - lo) * W, 4)
        assert torch.equal(tile, whole[lo * W:hi * W]), (kind, n, front, axis)


@pytest.mark.parametrize("H", HEIGHTS)
@pytest.mark.parametrize("kind", KINDS)
def test_compositor_of_one_rank_equals_the_slab_call_with_one_slab(vr, kind, H):
    import torch
    from volumerenderer_amd import distributed as D
    stack = partials(kind, H)[:1]
    image = stack[0].reshape(H, W, 4)
    P = vr.default_params(W, H, (64, 64, 64))
    for front, axis, _ in CAMERAS:
        cam = camera(vr, front)
        out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        if kind == "grey":
            got = D.composite_sort_last(image, cam, P, axis, out=out)
        elif kind == "colour":
            got = D.composite_sort_last_tf(image, cam, P, finisher(vr, kind), axis, out=out)
        else:
            got = D.composite_sort_last_proj(image, finisher(vr, kind), out=out)
        assert got is out and not torch.isnan(out).any()
        assert torch.equal(out.reshape(H * W, 4), slab_call(vr, kind, stack, 0, axis, cam, P)), (kind, H, front, axis)
