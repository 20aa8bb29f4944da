"""The ray-march kernels (csrc/raymarch.hip) against the float64 marcher at their edges.

Every frame here is compared pixel by pixel with refmarch.march_checked, which also reports how close each ray came to a
discrete decision (`slack`) and the propagated float32 rounding bound of each channel (`tol`); the derivation of both is
in tests/refmarch.py.  The rule for every case:
  * every pixel with slack > 1 (no decision can flip in float32) and tol <= CAP on every channel matches within its own
    `tol`;
  * the other pixels are masked and counted: those with slack <= 1 (a ray that grazes a face, an iso value within
    rounding of a sample) and those whose colour is so steep a function of the inputs that the bound exceeds CAP (the
    iso shading between about 1 and 7 degrees off the specular peak).  Together they are fewer than MASKED of the
    frame, and never the whole frame;
  * where the C restatement (oracle/raymarch_oracle.c) takes the same parameters, the frame also matches it within TOL.
The helper kernels (brick assembly, error metrics, compositing) are checked against NumPy; the wrappers' buffer checks
are exercised by rejection only -- no test hands a bad extent or a short buffer to a kernel.

Each case prints one "EDGE" line: the largest unmasked error, the largest unmasked error / tol, the largest tol a
checked pixel was held to, and the masked counts (by a decision, by the cap).
"""

import numpy as np
import pytest

from refmarch import march_checked, view_dir

pytestmark = pytest.mark.gpu
TOL = 2e-3            # the C restatement's tolerance (test_gpu_render.py)
MASKED = 0.05         # default bound on the masked fraction of a frame (CPU runs against the C restatement: <= 2.3 %)
CAP = TOL             # a pixel whose derived bound is looser than the C restatement's tolerance is not a check
# iso frames: besides the decisions, the pixels between about 1 and 7 degrees off the specular peak, where x^250 turns
# the normal's rounding (the float32 camera basis moves the hit by ~1e-5 of the cube) into more than CAP
MASKED_ISO = 0.15


@pytest.fixture(scope="module")
def vr():
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def f32(v):
    return tuple(float(np.float32(q)) for q in v)


def smooth(dims, seed=0):
    """A smooth [Z][Y][X] volume (largest voxel-to-voxel step a few grey levels for dims >= 16): the value bound of
    refmarch grows with G * dmax, so smooth data keeps it informative."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    a = rng.uniform(0.5, 1.5, 3)
    z, y, x = np.meshgrid(np.linspace(0, 1, Z), np.linspace(0, 1, Y), np.linspace(0, 1, X), indexing="ij")
    v = 125 + 65 * np.sin(3 * a[0] * x + 1) * np.cos(2 * a[1] * y) + 55 * np.sin(4 * a[2] * z + 2 * x)
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def _render(vr, vol, dims, cam, P, out=None):
    import torch
    v = vol if isinstance(vol, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(vol).reshape(-1)).cuda()
    return vr.raycast(v, dims, cam, P, out=out).cpu().numpy().astype(np.float64)


def check_case(vr, oracle, name, vol, W, H, mode=0, pos=(0.0, 0.0, -1.6), front=(0.0, 0.0, 1.0), up=(0.0, 1.0, 0.0),
               fov=50.0, step_dims=None, iso=0.4, ns=300, nee=0, near=0.1, far=100.0, box=None, sub=None,
               masked=None, covered=True, hits=False, got=None):
    """Render (unless `got` is given), compare with march_checked and (where it applies) the C restatement, print the
    case's EDGE line.  `sub` = (local volume, vol_origin) for partial mode: `vol` is then the global volume."""
    Z, Y, X = vol.shape
    sd = step_dims or (X, Y, Z)
    masked = masked if masked is not None else (MASKED_ISO if mode == 1 else MASKED)
    cam = vr.default_camera()
    cam.pos[:] = pos; cam.front[:] = front; cam.up[:] = up; cam.fov_deg = fov; cam.z_near = near; cam.z_far = far
    P = vr.default_params(W, H, sd, mode, iso)
    P.max_samples = ns; P.no_early_exit = nee
    if box is not None:
        P.box_min[:] = box[0]; P.box_max[:] = box[1]
    local, org = (vol, (0, 0, 0)) if sub is None else sub
    if sub is not None:
        P.global_dims[:] = (X, Y, Z); P.vol_origin[:] = org
    lz, ly, lx = local.shape
    if got is None:
        got = _render(vr, local, (lx, ly, lz), cam, P)
    ref, slack, tol = march_checked(vol, f32(pos), f32(front), f32(up), float(np.float32(fov)), W, H, f32(P.step_size),
                                    mode, float(np.float32(iso)), ns, not nee, f32(P.box_min), f32(P.box_max),
                                    float(np.float32(near)), float(np.float32(far)))
    d = np.abs(got - ref)
    decided = slack > 1
    ok = decided & (tol.max(-1) <= CAP)
    nmask = int((~ok).sum())
    worst = float(d[ok].max()) if ok.any() else 0.0
    ratio = float((d[ok] / np.maximum(tol[ok], 1e-30)).max()) if ok.any() else 0.0
    print("EDGE %-34s %5dx%-5d mode %d  max unmasked err %.3e  err/tol %.3f  max tol %.2e  masked %d+%d/%d"
          % (name, W, H, mode, worst, ratio, float(tol[ok].max()) if ok.any() else 0.0, int((~decided).sum()),
             int((decided & ~ok).sum()), W * H))
    assert np.isfinite(got).all(), name
    bad = (d > tol) & ok[..., None]
    if bad.any():
        i = np.argwhere(bad)[0]
        raise AssertionError("%s: pixel %s channel %d: kernel %.9g, float64 %.9g, tol %.3g (slack %.3g); %d such"
                             % (name, tuple(i[:2]), i[2], got[tuple(i)], ref[tuple(i)], tol[tuple(i)],
                                slack[tuple(i[:2])], int(bad.any(-1).sum())))
    assert nmask < W * H, "%s: every pixel masked" % name
    assert nmask <= masked * W * H, "%s: %d of %d pixels masked" % (name, nmask, W * H)
    if covered and mode != 1 or hits:   # some unmasked pixel where the ray took samples (0), hit (1), the cube is (2)
        seen = ref[..., 3] < 1 if mode == 0 else (ref[..., 0] < 1 if mode == 1 else ref[..., 2] == 1)
        assert (ok & seen).any(), name
    if oracle is not None:
        oc = oracle.default_camera()
        oc.pos[:] = cam.pos[:]; oc.front[:] = cam.front[:]; oc.up[:] = cam.up[:]
        oc.fov_deg, oc.z_near, oc.z_far = cam.fov_deg, cam.z_near, cam.z_far
        Po = oracle.default_params(W, H, sd, mode, iso)
        Po.max_samples = ns; Po.no_early_exit = nee
        Po.box_min[:] = P.box_min[:]; Po.box_max[:] = P.box_max[:]
        Po.global_dims[:] = P.global_dims[:]; Po.vol_origin[:] = P.vol_origin[:]
        want = oracle.render(local, oc, Po)
        assert np.abs(got - want).max() <= TOL, (name, float(np.abs(got - want).max()))
    return got, ref, ok


# ---- image sizes -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (1, 9), (9, 1), (7, 5), (65, 63)])
@pytest.mark.parametrize("mode", [0, 1, 2])
def test_image_sizes(vr, oracle, W, H, mode):
    """Frames that are not whole 8x8 wave tiles, down to one pixel: a 1x1 frame's ray is the exact centre ray
    (dir = front), the odd sizes have exact-zero direction components on their centre row / column."""
    vol = smooth((24, 20, 28), 1)
    check_case(vr, oracle, "size", vol, W, H, mode, pos=(0.05, -0.03, -1.4), front=(-0.02, 0.01, 1.0), iso=0.55,
               hits=W * H > 100)


def test_full_hd_frame_every_row(vr, oracle):
    """One 1920x1080 frame, every pixel, into a NaN-prefilled `out` (every pixel is written: misses too)."""
    import torch
    vol = smooth((20, 20, 20), 2)
    W, H = 1920, 1080
    cam = vr.default_camera()
    cam.pos[:] = (0.3, 0.2, -2.2); cam.front[:] = (-0.12, -0.08, 1.0)
    for mode in (0, 1):
        P = vr.default_params(W, H, (16, 16, 16), mode, 0.5)
        out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
        got = _render(vr, vol, (20, 20, 20), cam, P, out=out)
        assert not np.isnan(got).any()
        check_case(vr, None, "1080p", vol, W, H, mode, pos=(0.3, 0.2, -2.2), front=(-0.12, -0.08, 1.0),
                   step_dims=(16, 16, 16), iso=0.5, got=got)


@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (65, 63)])
def test_nan_prefilled_out_is_written_everywhere(vr, W, H):
    import torch
    vol = smooth((12, 10, 9), 3)
    for mode in (0, 1, 2):
        for pos, front in (((0.0, 0.0, -1.5), (0.0, 0.0, 1.0)), ((3.0, 3.0, 3.0), (1.0, 1.0, 1.0))):   # hit; all miss
            cam = vr.default_camera()
            cam.pos[:] = pos; cam.front[:] = front
            P = vr.default_params(W, H, (9, 10, 12), mode, 0.5)
            out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
            got = _render(vr, vol, (9, 10, 12), cam, P, out=out)
            assert not np.isnan(got).any(), (mode, pos)


# ---- volume dims and data --------------------------------------------------------------------------------------------
def _vol_cases():
    rng = np.random.default_rng(7)
    sat = smooth((23, 19, 17), 4)
    sat[:, :, :6] = 0
    sat[:, :, 11:] = 255                                                    # saturated at both ends
    return [("x=1", smooth((1, 9, 7), 11), None),
            ("y=2", smooth((6, 2, 5), 12), None),
            ("noise 7x5x6, 2 samples", rng.integers(0, 256, (6, 5, 7), dtype=np.uint8), None),
            ("all=1", np.full((1, 1, 1), 173, np.uint8), None),
            ("z=2,x=1", np.array([[[40]], [[220]]], np.uint8), None),
            ("primes 31x17x11", smooth((31, 17, 11), 5), None),
            ("64x3x5", smooth((64, 3, 5), 6), None),
            ("3x5x61", smooth((3, 5, 61), 7), None),
            ("saturated 0/255", sat, None),
            ("brick step 256x256x128", smooth((29, 23, 19), 8), (256, 256, 128)),
            ("brick step 8x8x8", smooth((29, 23, 19), 9), (8, 8, 8))]


@pytest.mark.parametrize("case", range(11))
def test_volume_dims(vr, oracle, case):
    name, vol, sd = _vol_cases()[case]
    # (white noise is steep everywhere: the composite bound stays informative over two samples, not three hundred)
    ns = 2 if name.startswith("noise") else 300
    # (iso shading of white noise is steep everywhere: most hit pixels exceed CAP, so noise runs modes 0 and 2 only)
    for mode in ((0, 2) if name.startswith("noise") else (0, 1, 2)):
        check_case(vr, oracle, name, vol, 33, 27, mode, pos=(0.4, 0.3, -1.3), front=(-0.35, -0.25, 1.0),
                   step_dims=sd, iso=0.5, ns=ns)


# ---- cameras ---------------------------------------------------------------------------------------------------------
SIDES = [((1.6, 0, 0), (-1, 0, 0)), ((-1.6, 0, 0), (1, 0, 0)), ((0, 1.6, 0), (0, -1, 0)), ((0, -1.6, 0), (0, 1, 0)),
         ((0, 0, 1.6), (0, 0, -1)), ((0, 0, -1.6), (0, 0, 1))]


@pytest.mark.parametrize("side", range(6))
def test_cameras_on_each_side(vr, oracle, side):
    """Outside on each of the six sides, the front along an axis, odd W and H (exact-zero directions on the centre row
    and column); up is chosen off the front's axis."""
    vol = smooth((21, 18, 15), 10 + side)
    pos, front = SIDES[side]
    up = (0.0, 0.0, 1.0) if side in (2, 3) else (0.0, 1.0, 0.0)
    for mode in (0, 1, 2):
        check_case(vr, oracle, "side %d" % side, vol, 31, 23, mode, pos=pos, front=front, up=up, iso=0.5)


# (name, camera, masked fraction (None: the mode's default), some ray takes samples).  Four frames take no sample at all,
# by the GL semantics k_raycast keeps (the nearest cube point in front of the near plane, no culling): a camera on a face
# plane looking in or inside the cube sees the exit face (t0 < z_near, so th = t1) and its rays leave the cube at once;
# so does every ray when z_near cuts the whole front of the cube; z_far before the cube covers nothing.  Those four pin
# the coverage decision and the constant colours only.  "z_near cuts a corner" mixes both kinds of ray in one frame.
CAMS = [("on face plane x=0.5, looking in", dict(pos=(0.5, 0.1, 0.2), front=(-1.0, 0.05, 0.02)), 0.25, False),
        ("in plane y=0.5, outside", dict(pos=(0.1, 0.5, -1.5), front=(0.0, 0.0, 1.0)), 0.25, True),
        ("on edge x=y=-0.5", dict(pos=(-0.5, -0.5, -1.5), front=(0.2, 0.2, 1.0)), 0.25, True),
        ("inside the cube", dict(pos=(0.1, 0.05, -0.2), front=(0.2, 0.1, 1.0)), None, False),
        ("z_near cuts the cube", dict(pos=(0.05, 0.0, -0.75), front=(0.0, 0.0, 1.0), near=0.5), None, False),
        ("z_near cuts a corner", dict(pos=(-1.0, 0.05, -1.0), front=(1.0, 0.0, 1.0), near=0.9), None, True),
        ("z_far before the cube", dict(pos=(0.05, 0.0, -1.5), front=(0.0, 0.0, 1.0), far=0.8), None, False),
        ("z_far through the cube", dict(pos=(0.05, 0.0, -1.5), front=(0.0, 0.0, 1.0), far=1.2), None, True),
        ("tilted up", dict(pos=(0.6, 0.5, -1.2), front=(-0.5, -0.4, 1.0), up=(0.4, 1.0, 0.3)), None, True),
        ("fov 10", dict(pos=(0.1, 0.05, -1.4), front=(-0.05, -0.03, 1.0), fov=10.0), None, True),
        ("fov 120", dict(pos=(0.3, 0.2, -0.9), front=(-0.2, -0.1, 1.0), fov=120.0), None, True)]


@pytest.mark.parametrize("case", range(len(CAMS)))
def test_camera_edges(vr, oracle, case):
    name, kw, masked, cov = CAMS[case]
    vol = smooth((19, 17, 23), 20 + case - (case > 5))        # (the seeds the cases had before the corner case)
    for mode in (0, 1, 2):
        _, ref, ok = check_case(vr, oracle, name, vol, 29, 21, mode, iso=0.45, masked=masked, covered=cov, **kw)
        if name == "z_near cuts a corner" and mode == 0:
            # checked rays behind the cut (covered, the back face: no sample, A = 0) and in front of it (A > 0)
            assert (ok & (ref[..., 3] == 0)).any() and (ok & (ref[..., 3] > 0) & (ref[..., 3] < 1)).any()


# ---- march settings and iso values -----------------------------------------------------------------------------------
@pytest.mark.parametrize("ns", [0, 1, 2, 300, 2000])
@pytest.mark.parametrize("nee", [0, 1])
def test_max_samples(vr, oracle, ns, nee):
    vol = smooth((20, 18, 22), 30)
    vol[8:14] = 255                                     # an opaque slab: alpha > 0.99 within a few samples
    sd = (256, 256, 256) if ns == 2000 else None        # 2000 steps of 1/256 reach through the cube
    for mode in (0, 2):
        check_case(vr, oracle, "ns %d nee %d" % (ns, nee), vol, 25, 19, mode, pos=(0.2, 0.1, -1.4),
                   front=(-0.1, -0.05, 1.0), step_dims=sd, ns=ns, nee=nee, covered=ns > 0)
    # (2000 steps of 1/256: eight times the iso decisions of a 1/32 step, so more rays come within rounding of one)
    check_case(vr, oracle, "ns %d iso" % ns, vol, 25, 19, 1, pos=(0.2, 0.1, -1.4), front=(-0.1, -0.05, 1.0),
               step_dims=sd, ns=ns, iso=0.6, hits=ns > 2)


@pytest.mark.parametrize("iso", [0.0, 1 / 255.0, 77 / 255.0, 200 / 255.0, 1.0])
def test_iso_values(vr, oracle, iso):
    """iso exactly on a grey level: the samples at voxel centres sit on it, so those rays are masked, the rest pinned.
    iso 0: no sample is below it, no hit; iso 1: only a crossing into a 255 region hits."""
    vol = smooth((21, 19, 17), 40)
    vol[5:12, 8:11, 6:14] = 255
    vol[:, :6, :] = 0
    check_case(vr, oracle, "iso %.4f" % iso, vol, 33, 25, 1, pos=(0.3, -0.2, -1.3), front=(-0.25, 0.15, 1.0),
               iso=iso, masked=0.15, hits=0.1 < iso < 0.9)


# ---- partial mode: slabs with halo and vol_origin --------------------------------------------------------------------
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_partial_slabs(vr, oracle, axis):
    """Rank r of 3 along `axis`: box [lo/n, hi/n) (the last rank's box_max 2.0), one halo voxel each side, vol_origin;
    the float64 reference marches the GLOBAL volume with the same box."""
    dims = (22, 19, 25)
    vol = smooth(dims, 50 + axis)
    n = dims[axis]
    for r in range(3):
        lo, hi = r * n // 3, (r + 1) * n // 3
        a0, a1 = max(0, lo - 1), min(n, hi + 1)
        bmin, bmax, org = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 0, 0]
        bmin[axis] = float(np.float32(lo / n)); bmax[axis] = float(np.float32(hi / n)) if r < 2 else 2.0
        org[axis] = a0
        sl = [slice(None)] * 3
        sl[2 - axis] = slice(a0, a1)
        local = np.ascontiguousarray(vol[tuple(sl)])
        check_case(vr, oracle, "partial axis %d rank %d" % (axis, r), vol, 31, 25, 2, pos=(0.45, 0.35, -1.3),
                   front=(-0.35, -0.25, 1.0), box=(bmin, bmax), sub=(local, org))


# ---- skip grid -------------------------------------------------------------------------------------------------------
def _grid_def(vol, S):
    Z, Y, X = vol.shape
    n = [(q + S - 1) // S for q in (X, Y, Z)]
    want = np.empty((n[2], n[1], n[0], 2), np.uint8)
    for cz in range(n[2]):
        for cy in range(n[1]):
            for cx in range(n[0]):
                blk = vol[cz * S:cz * S + S + 1, cy * S:cy * S + S + 1, cx * S:cx * S + S + 1]
                want[cz, cy, cx] = (blk.min(), blk.max())
    return want.reshape(-1)


def _sparse_volume(dims, seed):
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    vol = np.zeros((Z, Y, X), np.uint8)
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    r = np.sqrt((xx - X * 0.4) ** 2 + (yy - Y * 0.5) ** 2 + (zz - Z * 0.45) ** 2)
    vol[r < min(dims) * 0.3] = 180
    vol[Z // 2:Z // 2 + 3, 1:Y // 3, X // 2:] = rng.integers(0, 256, (3, Y // 3 - 1, X - X // 2))
    vol[1, :, :] = 2
    return vol


def _grid_and_frames(vr, vol, dims, cell):
    """The grid against the definition; frames with / without it bit-identical in composite and iso mode."""
    import torch
    dvol = torch.from_numpy(vol).cuda().reshape(-1)
    grid = vr.build_skip_grid(dvol, dims, cell)
    assert np.array_equal(grid.cpu().numpy(), _grid_def(vol, cell)), (dims, cell)
    cam = vr.default_camera()
    cam.pos[:] = (0.5, 0.4, -1.2); cam.front[:] = (-0.4, -0.3, 1.0)
    for mode, iso in ((0, 0.0), (1, 1 / 255.0), (1, 100 / 255.0), (1, 181 / 255.0)):
        P = vr.default_params(48, 40, (64, 64, 64), mode, iso)
        plain = _render(vr, dvol, dims, cam, P)
        vr.use_skip_grid(P, grid, cell)
        assert np.array_equal(plain, _render(vr, dvol, dims, cam, P)), (dims, cell, mode, iso)


@pytest.mark.parametrize("cell", [1, 2, 3, 5, 7, 8, 16, 24, 31, 64])
def test_skip_grid_cells(vr, cell):
    """Every cell size, on dims the cell does not divide, through the one-wave-per-cell kernel k_skip_grid (the only
    one for x not a multiple of 128): x = 40 has 8-byte aligned rows, so cells of 8, 16, 24 and 64 take its 8-byte
    path; x = 37 never does."""
    for dims in ((40, 29, 23), (37, 29, 23)):
        _grid_and_frames(vr, _sparse_volume(dims, cell), dims, cell)


@pytest.mark.parametrize("v1", [0, 1])
def test_skip_grid_strip_kernel_vs_v1(vr, v1):
    """x a multiple of 128 with 8-voxel cells: k_skip_grid8 (v1 = 0) and the one-wave-per-cell kernel forced by
    vr_debug_set("skip_grid_v1") (v1 = 1), each against the definition and with bit-identical frames."""
    from volumerenderer_amd import _lib
    assert _lib.lib().vr_debug_set(b"skip_grid_v1", v1) == 0
    try:
        for dims in ((256, 19, 13), (128, 17, 9)):
            _grid_and_frames(vr, _sparse_volume(dims, 3), dims, 8)
    finally:
        _lib.lib().vr_debug_set(b"skip_grid_v1", 0)


# ---- offset views ----------------------------------------------------------------------------------------------------
def test_offset_views(vr):
    """A volume and a grid at byte offsets 1..15 into larger allocations: the grid build, the frames (with and without
    the grid) and brick (dis)assembly equal the aligned results, and nothing outside the views is written."""
    import torch
    dims = (40, 21, 17)
    vol = _sparse_volume(dims, 11)
    nvox = vol.size
    dvol = torch.from_numpy(vol).cuda().reshape(-1)
    cam = vr.default_camera()
    cam.pos[:] = (0.4, 0.3, -1.2); cam.front[:] = (-0.3, -0.2, 1.0)
    for cell in (8, 16, 5):
        grid = vr.build_skip_grid(dvol, dims, cell)
        want = {}
        for mode, iso in ((0, 0.0), (1, 100 / 255.0)):
            P = vr.default_params(24, 20, (64, 64, 64), mode, iso)
            want[mode] = _render(vr, dvol, dims, cam, P)
        for off in range(1, 16):
            big = torch.full((nvox + 64,), 0xA5, dtype=torch.uint8, device="cuda")
            v = big[off:off + nvox]
            v.copy_(dvol)
            gbig = torch.full((grid.numel() + 64,), 0x5A, dtype=torch.uint8, device="cuda")
            g = gbig[off:off + grid.numel()]
            vr.build_skip_grid(v, dims, cell, out=g)
            assert torch.equal(g, grid), (cell, off)
            assert (gbig[:off] == 0x5A).all() and (gbig[off + grid.numel():] == 0x5A).all()
            for mode, iso in ((0, 0.0), (1, 100 / 255.0)):
                P = vr.default_params(24, 20, (64, 64, 64), mode, iso)
                assert np.array_equal(_render(vr, v, dims, cam, P), want[mode]), (cell, off, mode)
                vr.use_skip_grid(P, g, cell)
                assert np.array_equal(_render(vr, v, dims, cam, P), want[mode]), (cell, off, mode)
    # brick (dis)assembly from / into offset views
    bd, grid3 = (32, 5, 3), (2, 3, 2)
    ijk = np.array([[1, 2, 1], [0, 0, 0], [1, 0, 1]], np.int64)
    rng = np.random.default_rng(12)
    bricks = rng.integers(0, 256, 3 * 32 * 5 * 3, dtype=np.uint8)
    ref_vol = vr.assemble_bricks(torch.from_numpy(bricks).cuda(), bd, ijk, grid3)
    nb = bricks.size
    for off in range(1, 16):
        src = torch.zeros(nb + 32, dtype=torch.uint8, device="cuda")
        src[off:off + nb].copy_(torch.from_numpy(bricks))
        dst = torch.zeros(ref_vol.numel() + 32, dtype=torch.uint8, device="cuda")
        vr.assemble_bricks(src[off:off + nb], bd, ijk, grid3, out=dst[off:off + ref_vol.numel()])
        assert torch.equal(dst[off:off + ref_vol.numel()], ref_vol), off
        assert (dst[:off] == 0).all() and (dst[off + ref_vol.numel():] == 0).all()
        back = torch.full((nb + 32,), 7, dtype=torch.uint8, device="cuda")
        vr.disassemble_bricks(dst[off:off + ref_vol.numel()], bd, ijk, grid3, out=back[off:off + nb])
        assert np.array_equal(back[off:off + nb].cpu().numpy(), bricks), off
        assert (back[:off] == 7).all() and (back[off + nb:] == 7).all()


# ---- helpers against NumPy -------------------------------------------------------------------------------------------
def _place(bricks, bd, ijk, grid3, vol):
    X, Y, Z = bd
    GX, GY = X * grid3[0], Y * grid3[1]
    v = vol.reshape(Z * grid3[2], GY, GX)
    for b, (i, j, k) in enumerate(ijk):
        v[k * Z:(k + 1) * Z, j * Y:(j + 1) * Y, i * X:(i + 1) * X] = bricks[b].reshape(Z, Y, X)
    return vol


@pytest.mark.parametrize("X", [16, 32])
def test_assemble_maps(vr, X):
    """Sparse, permuted and single-brick maps; a poisoned `out` whose brick-less cells must survive (vrhip.h)."""
    import torch
    rng = np.random.default_rng(X)
    bd, grid3 = (X, 3, 5), (3, 2, 2)
    maps = {"sparse": [[2, 1, 0], [0, 0, 1]],
            "permuted": [[(b * 5) % 3, (b * 5 // 3) % 2, (b * 5 // 6) % 2] for b in range(12)],
            "single": [[1, 1, 1]]}
    assert len({tuple(t) for t in maps["permuted"]}) == 12
    nvol = X * 3 * 5 * 12
    for name, m in maps.items():
        ijk = np.array(m, np.int64)
        bricks = rng.integers(0, 256, (len(m), X * 15), dtype=np.uint8)
        out = torch.full((nvol,), 0xCD, dtype=torch.uint8, device="cuda")
        vr.assemble_bricks(torch.from_numpy(bricks.reshape(-1)).cuda(), bd, ijk, grid3, out=out)
        want = _place(bricks, bd, ijk, grid3, np.full(nvol, 0xCD, np.uint8))
        assert np.array_equal(out.cpu().numpy(), want), name
        back = vr.disassemble_bricks(out, bd, ijk, grid3).cpu().numpy()
        assert np.array_equal(back, bricks.reshape(-1)), name


@pytest.mark.parametrize("n", [1, 255, 257, (1 << 20) + 3])
def test_error_metrics_tails(vr, n):
    import torch
    rng = np.random.default_rng(n)
    a = rng.integers(0, 256, n, dtype=np.uint8)
    b = rng.integers(0, 256, n, dtype=np.uint8)
    e = np.abs(a.astype(np.int64) - b.astype(np.int64))
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    mx, mean = vr.measure_error(da, db)
    assert mx == e.max() and abs(mean - e.sum() / n) <= 1e-12 * max(1.0, e.sum() / n)
    assert np.array_equal(vr.query_error(da, db).cpu().numpy(), e.astype(np.uint8))


def test_measure_error_past_2_31_voxels(vr):
    """n = 2^31 + 2^20 + 5: the 64-bit index and sum.  b repeats 0..200 (built on the device), a = 0, so the sum has a
    closed form; the one error of 250 sits past 2^31."""
    import torch
    n = (1 << 31) + (1 << 20) + 5
    block = (torch.arange(201, dtype=torch.int32, device="cuda")).to(torch.uint8)
    b = block.repeat(n // 201 + 1)[:n].contiguous()
    b[n - 2] = 250
    a = torch.zeros(n, dtype=torch.uint8, device="cuda")
    full, rem = divmod(n, 201)
    total = full * (200 * 201 // 2) + rem * (rem - 1) // 2 - ((n - 2) % 201) + 250
    mx, mean = vr.measure_error(a, b)
    assert mx == 250
    assert abs(mean * n - total) <= 1e-9 * total, (mean * n, total)
    del a, b
    torch.cuda.empty_cache()


@pytest.mark.parametrize("npix", [1, 255, 257])
def test_composite_helpers(vr, npix):
    """composite_over / composite_finish / composite_slabs at lengths that are not multiples of 256, against float64.
    Each output is a product or sum of two float32 roundings of [0, 1] values: |err| <= 4 EPS per operation."""
    import ctypes as C
    import torch
    from volumerenderer_amd import _lib
    rng = np.random.default_rng(npix)
    def part():
        p = np.zeros((npix, 4), np.float32)
        p[:, 0] = rng.uniform(0, 1, npix); p[:, 1] = rng.uniform(0, 1, npix); p[:, 2] = rng.integers(0, 2, npix)
        return p
    f, b = part(), part()
    df, db = torch.from_numpy(f).cuda(), torch.from_numpy(b).cuda()
    got = vr.composite_over(df.clone(), db).cpu().numpy().astype(np.float64)
    F, B = f.astype(np.float64), b.astype(np.float64)
    assert np.abs(got[:, 0] - (F[:, 0] + F[:, 1] * B[:, 0])).max() <= 4 * 2.0 ** -24
    assert np.abs(got[:, 1] - F[:, 1] * B[:, 1]).max() <= 2 * 2.0 ** -24
    assert np.array_equal(got[:, 2], np.maximum(F[:, 2], B[:, 2]))
    fin = vr.composite_finish(df).cpu().numpy().astype(np.float64)
    cov = F[:, 2] > 0
    want = np.ones((npix, 4))
    want[cov, 0] = 1 - F[cov, 0]; want[cov, 1] = 1 - F[cov, 0]; want[cov, 3] = 1 - F[cov, 1]
    assert np.abs(fin - want).max() <= 2.0 ** -24
    # slabs: three partials of a W x H frame's pixels [first, first + npix), every pixel in its view order
    W, H = 37, 29
    first = (W * H - npix) // 2
    parts = np.stack([part() for _ in range(3)])
    cam, P = vr.default_camera(), vr.default_params(W, H)
    cam.pos[:] = (0.1, 0.2, -0.3); cam.front[:] = (0.0, 0.2, 1.0)    # dir.y changes sign inside the frame
    dparts = torch.from_numpy(parts).cuda()
    for axis in (0, 1, 2):
        dout = torch.full((npix, 4), float("nan"), dtype=torch.float32, device="cuda")
        assert _lib.lib().vr_composite_slabs(C.c_void_p(dparts.data_ptr()), 3, npix, first, axis, C.byref(cam), C.byref(P),
                                             C.c_void_p(dout.data_ptr()), None) == 0
        out = dout.cpu().numpy().astype(np.float64)
        asc = view_dir((None, cam.pos[:], cam.front[:], cam.up[:], cam.fov_deg), W, H, axis).reshape(-1)[first:first + npix] >= 0
        Pp = parts.astype(np.float64)
        c = np.zeros(npix); tau = np.ones(npix); cv = np.zeros(npix)
        for k in range(3):
            p = np.where(asc[:, None], Pp[k], Pp[2 - k])
            c = c + tau * p[:, 0]; tau = tau * p[:, 1]; cv = np.maximum(cv, p[:, 2])
        w = np.ones((npix, 4))
        w[cv > 0, 0] = 1 - c[cv > 0]; w[cv > 0, 1] = 1 - c[cv > 0]; w[cv > 0, 3] = 1 - tau[cv > 0]
        assert np.abs(out - w).max() <= 16 * 2.0 ** -24, axis


# ---- the wrappers refuse bad buffers before any launch ---------------------------------------------------------------
def test_wrappers_refuse_bad_buffers(vr, monkeypatch):
    """Every rejection is raised by the Python wrapper: the C entry points are replaced by a tripwire first."""
    import torch
    from volumerenderer_amd import _lib
    dims = (12, 10, 8)
    vol = torch.zeros(12 * 10 * 8, dtype=torch.uint8, device="cuda")
    cam, P = vr.default_camera(), vr.default_params(16, 8, dims)
    grid = vr.build_skip_grid(vol, dims, 4)
    other = vr.build_skip_grid(torch.zeros(13 * 10 * 8, dtype=torch.uint8, device="cuda"), (13, 10, 8), 4)
    real = _lib.lib()

    class Tripwire:
        def __getattr__(self, name):
            if name.startswith("vr_raycast") or name.startswith("vr_composite") or name.startswith("vr_skip_grid"):
                raise AssertionError("%s reached with a bad buffer" % name)
            return getattr(real, name)
    monkeypatch.setattr(_lib, "lib", lambda: Tripwire())
    img = lambda *s, **k: torch.empty(*s, dtype=k.get("dtype", torch.float32), device=k.get("device", "cuda"))
    for bad in (img(8, 16, 3), img(8, 15, 4), img(8 * 16 * 4 - 4), img(8, 16, 4, dtype=torch.float64),
                img(8, 16, 4, device="cpu"), img(16, 8, 4).transpose(0, 1)):
        with pytest.raises(ValueError):
            vr.raycast(vol, dims, cam, P, out=bad)
    for d in ((12, 10, 7), (0, 10, 8), (-12, -10, 8)):
        with pytest.raises(ValueError):
            vr.raycast(vol, d, cam, P)
    for g, cell in ((grid[:-2], 4), (grid, 8), (other, 4)):           # short; another cell; another volume's dims
        Pg = vr.default_params(16, 8, dims)
        vr.use_skip_grid(Pg, g, cell)
        with pytest.raises(ValueError):
            vr.raycast(vol, dims, cam, Pg)
    Pg = vr.default_params(16, 8, dims)
    Pg.skip_cell, Pg.skip_grid_dev = 4, grid.data_ptr()                 # not attached by use_skip_grid
    with pytest.raises(ValueError):
        vr.raycast(vol, dims, cam, Pg)
    u8 = lambda n, **k: torch.empty(n, dtype=k.get("dtype", torch.uint8), device=k.get("device", "cuda"))
    for bad in (u8(grid.numel() - 1), u8(grid.numel(), dtype=torch.int16), u8(grid.numel(), device="cpu"),
                u8(2 * grid.numel())[::2]):
        with pytest.raises(ValueError):
            vr.build_skip_grid(vol, dims, 4, out=bad)
    for cell in (0, 65):
        with pytest.raises(ValueError):
            vr.build_skip_grid(vol, dims, cell)
    front = img(8, 16, 4)
    for bad in (img(8, 15, 4), img(8, 16, 4, dtype=torch.float16), img(8, 16, 4, device="cpu"),
                img(16, 8, 4).transpose(0, 1)):
        with pytest.raises(ValueError):
            vr.composite_over(front, bad)
        with pytest.raises(ValueError):
            vr.composite_over(bad, front) if bad.numel() == front.numel() else vr.composite_over(front, bad)
        with pytest.raises(ValueError):
            vr.composite_finish(front, out=bad)
        if bad.numel() == front.numel():
            with pytest.raises(ValueError):
                vr.composite_finish(bad)
    with pytest.raises(ValueError):
        vr.composite_over(img(8, 16, 4, dtype=torch.float64), img(8, 16, 4, dtype=torch.float64))
    with pytest.raises(ValueError):
        vr.composite_over(img(5, 3), img(5, 3))                          # not whole pixels
