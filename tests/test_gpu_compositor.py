"""Sort-last compositing across ranks (vr_compositor_composite's world > 1 path) on ONE GPU.

Two RCCL ranks cannot share a device, so the ranks' compositors are created with vr_compositor_create_with_transport
and a loopback transport (tests/loopback_transport.cpp, built here with g++): NCCL's grouped point-to-point semantics,
copies on the callers' streams, no synchronisation of its own, a log of every call.  Every rank is a host thread with
its own stream; it ray-marches its slab in VR_RENDER_PARTIAL mode and calls the compositor at once.  Checked per case:

  1. the exchange pattern in the transport's log (tile rows from distributed.tile_rows);
  2. the exchange is lossless: rank 0's frame equals ONE vr_composite_slabs call over the stacked partials bit for bit;
  3. each partial equals the float64 march_partial of the GLOBAL volume (tests/refmarch.py: halo and vol_origin);
  4. the frame equals the float64 order-free reference (march_composite without early exit) and the single pass;
  5. the scene can tell: partials combined in the wrong view order differ from the reference visibly.
"""
import ctypes as C
import math
import os
import subprocess
import threading
import time

import numpy as np
import pytest

from refmarch import march_composite, march_partial, rays, view_dir

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
DIMS = (29, 23, 31)                 # x, y, z: no extent divides by any world size below
STEPS = tuple(2 * d for d in DIMS)  # step_size = half a voxel on every axis
W, H = 83, 61                       # H odd, divisible by no world size below
WORLDS = (2, 3, 5, 8)
TOL = 2e-3
PARTIAL_FRAC = 0.005                # partial pixels allowed above TOL: samples within rounding of a slab plane
SENSE = 0.02                        # a wrong view order must move >= 1 % of the pixels by more than this
INSIDE_POS, INSIDE_DIST, INSIDE_TILT, INSIDE_FOV = 0.25, 1.0, 0.4459, 90.0
GROUP_START, GROUP_END, SEND, RECV = 0, 1, 2, 3
VR_ERR_INVALID, VR_ERR_NO_DEVICE = -1, -2


def build_loopback(out_dir):
    """Compiles tests/loopback_transport.cpp with g++ into out_dir; returns the .so's path."""
    so = os.path.join(str(out_dir), "libloopback.so")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-fPIC", "-shared", "-pthread",
                           "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(ROCM, "include"),
                           os.path.join(ROOT, "tests", "loopback_transport.cpp"), "-L" + os.path.join(ROCM, "lib"),
                           "-lamdhip64", "-Wl,-rpath," + os.path.join(ROCM, "lib"), "-o", so])
    return so


# ---- the scene (host only) -------------------------------------------------------------------------------------------
def scene_volume(dims=DIMS, seed=3):
    """A smooth off-centre blob, seeded bright 2-voxel lumps (denser inside the blob) and faint noise: mid-density
    (median exit transmittance 0.2-0.8 per camera) and lumpy along every ray, so that the order in which the slabs
    are combined moves the colour."""
    X, Y, Z = dims
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid((np.arange(Z) + 0.5) / Z, (np.arange(Y) + 0.5) / Y, (np.arange(X) + 0.5) / X, indexing="ij")
    blob = np.exp(-((x - 0.42) ** 2 + (y - 0.55) ** 2 + (z - 0.47) ** 2) / 0.06)
    n = [(q + 1) // 2 for q in (Z, Y, X)]
    lumps = (rng.random(n) < 0.08) * rng.uniform(120, 230, n)
    lumps = lumps.repeat(2, 0).repeat(2, 1).repeat(2, 2)[:Z, :Y, :X]
    v = 25 * blob + lumps * (0.4 + 0.6 * blob) + rng.uniform(0, 3, (Z, Y, X))
    return np.clip(np.rint(v), 0, 255).astype(np.uint8)


def orbit(deg):
    th = math.radians(deg)
    return ("orbit%g" % deg, (0.75 * math.sin(th), 0.0, -0.75 * math.cos(th)), (-math.sin(th), 0.0, math.cos(th)),
            (0.0, 1.0, 0.0), 50.0)


def cameras(axis):
    """(name, pos, front, up): outside the cube on the - side of `axis`; on the + side; "inside": pos[axis] inside the
    slab range but pos outside the cube, tilted so that dir[axis] changes sign between rows 43 and 44 of 61 (up =
    the axis, so rows run along it: a tile other than rank 0's for every world size); and for axis 1 "orbit", the bench
    orbit camera at 30 degrees (dir.y = 0 exactly on the middle row, row 30)."""
    e = np.eye(3)
    a = axis
    b, c = [k for k in range(3) if k != a]
    up = e[2] if a == 1 else e[1]
    side = 0 if a == 2 else 2
    cams = [("minus", -1.8 * e[a] + 0.12 * e[b] - 0.07 * e[c], e[a] - 0.08 * e[b] + 0.05 * e[c], up),
            ("plus", 1.8 * e[a] - 0.1 * e[b] + 0.06 * e[c], -e[a] + 0.05 * e[b] - 0.07 * e[c], up),
            ("inside", INSIDE_POS * e[a] - INSIDE_DIST * e[side], e[side] + INSIDE_TILT * e[a], e[a])]
    out = [(n, tuple(float(q) for q in p), tuple(float(q) for q in f), tuple(float(q) for q in u),
            INSIDE_FOV if n == "inside" else 50.0) for n, p, f, u in cams]
    return out + [orbit(30.0)] if a == 1 else out


def shard(n, r, world):
    q, m = divmod(n, world)
    lo = r * q + min(r, m)
    return lo, lo + q + (1 if r < m else 0)


def f32(v):
    return float(np.float32(v))


def slab_setup(axis, world, r, dims=DIMS):
    """Rank r's slab along `axis`: (box_min, box_max, vol_origin, local dims, numpy slice of the [Z][Y][X] volume).
    One halo voxel each side; the last rank's box_max is 2.0 (bench.py)."""
    n = dims[axis]
    lo, hi = shard(n, r, world)
    a0, a1 = max(0, lo - 1), min(n, hi + 1)
    bmin, bmax, org = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0], [0, 0, 0]
    bmin[axis] = f32(lo / n)
    bmax[axis] = f32(hi / n) if r < world - 1 else 2.0
    org[axis] = a0
    sub = list(dims)
    sub[axis] = a1 - a0
    sl = [slice(None)] * 3
    sl[2 - axis] = slice(a0, a1)
    return bmin, bmax, org, sub, tuple(sl)


def combine64(parts, ascending):
    """Float64 over-combine of [world][h][w][4] partials, slab order ascending where `ascending`, then the colour
    transfer of k_composite_slabs."""
    n = parts.shape[0]
    c = np.zeros(parts.shape[1:3]); tau = np.ones(parts.shape[1:3]); cov = np.zeros(parts.shape[1:3])
    for k in range(n):
        p = np.where(ascending[..., None], parts[k], parts[n - 1 - k])
        c = c + tau * p[..., 0]
        tau = tau * p[..., 1]
        cov = np.maximum(cov, p[..., 2])
    out = np.ones(parts.shape[1:])
    out[..., 0] = np.where(cov > 0, 1 - c, 1.0)
    out[..., 1] = out[..., 0]
    out[..., 3] = np.where(cov > 0, 1 - tau, 1.0)
    return out


def reference(vol, cam, axis, world, w, h, rows=None, dims=DIMS, steps=STEPS):
    """Float64 partials of every rank and the order-free frame, on `rows` (default all)."""
    cov, vuv, g = rays(cam[1], cam[2], cam[3], cam[4], w, h, rows=rows)
    step = tuple(1.0 / s for s in steps)
    parts = np.stack([march_partial(vol, cov, vuv, g, step, *slab_setup(axis, world, r, dims)[:2]) for r in range(world)])
    frame = march_composite(vol, cov, vuv, g, step, early_exit=False)
    return parts, frame


def sensitivity(parts, frame, cam, axis, world, w, h, tile_shift):
    """Fractions of pixels that move by more than SENSE when the partials are combined with every pixel's order
    reversed, and (tile_shift) with each tile's order computed as if its first pixel were pixel 0."""
    d = view_dir(cam, w, h, axis) >= 0
    out = {"reversed": float((np.abs(combine64(parts, ~d) - frame).max(-1) > SENSE).mean())}
    if tile_shift:
        wrong = np.empty_like(d)
        for lo, hi in [shard(h, r, world) for r in range(world)]:
            wrong[lo:hi] = d[:hi - lo]
        out["first_pixel_0"] = float((np.abs(combine64(parts, wrong) - frame).max(-1) > SENSE).mean())
    return out


# ---- GPU side --------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def vr():
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def L(vr):
    from volumerenderer_amd import _lib
    return _lib.lib()


@pytest.fixture(scope="module")
def LB(L, tmp_path_factory):
    """The loopback transport, compiled (in a subprocess) and loaded after libvrhip.so, so both bind torch's HIP."""
    lb = C.CDLL(build_loopback(tmp_path_factory.mktemp("loopback")))
    lb.lb_create.restype = C.c_void_p; lb.lb_create.argtypes = [C.c_int32, C.c_double]
    lb.lb_destroy.argtypes = [C.c_void_p]
    lb.lb_rank_ctx.restype = C.c_void_p; lb.lb_rank_ctx.argtypes = [C.c_void_p, C.c_int32]
    lb.lb_transport.restype = C.c_void_p
    lb.lb_fail_at.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32]
    lb.lb_count_delta.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64]
    lb.lb_log_size.argtypes = [C.c_void_p]
    lb.lb_log_entry.argtypes = [C.c_void_p, C.c_int32, C.POINTER(C.c_int64)]
    lb.lb_log_clear.argtypes = [C.c_void_p]
    lb.lb_errors.argtypes = [C.c_void_p, C.c_char_p, C.c_int32]
    return lb


@pytest.fixture(scope="module")
def volume():
    return scene_volume()


class Ranks:
    """`world` compositors over one loopback fake, one stream each."""

    def __init__(self, vr, L, LB, world, w, h, timeout=30.0):
        self.vr, self.L, self.LB, self.world, self.w, self.h = vr, L, LB, world, w, h
        self.fake = LB.lb_create(world, timeout)
        assert self.fake
        self.streams, self.comps = [], []
        for r in range(world):
            s = C.c_void_p()
            assert L.vr_stream_create(C.byref(s)) == 0
            self.streams.append(s)
            c = C.c_void_p()
            assert L.vr_compositor_create_with_transport(C.byref(c), C.c_void_p(LB.lb_transport()),
                                                         C.c_void_p(LB.lb_rank_ctx(self.fake, r)), r, world, w, h) == 0
            self.comps.append(c)

    def close(self):
        for s in self.streams:
            self.L.vr_stream_synchronize(s)
        for c in self.comps:
            assert self.L.vr_compositor_destroy(c) == 0
        for s in self.streams:
            self.L.vr_stream_destroy(s)
        self.LB.lb_destroy(self.fake)

    def log(self):
        e = (C.c_int64 * 5)()
        out = []
        for i in range(self.LB.lb_log_size(self.fake)):
            assert self.LB.lb_log_entry(self.fake, i, e) == 0
            out.append(tuple(int(q) for q in e))
        return out

    def errors(self):
        buf = C.create_string_buffer(4096)
        self.LB.lb_errors(self.fake, buf, 4096)
        return buf.value.decode()

    def run(self, jobs, timeout=120.0):
        """jobs[r]() on a thread per rank; returns their results once every thread is back (no stream is
        synchronised here)."""
        res = [None] * self.world
        def body(r):
            try:
                res[r] = jobs[r]()
            except BaseException as ex:      # noqa: BLE001 -- handed to the test below
                res[r] = ex
        th = [threading.Thread(target=body, args=(r,), daemon=True) for r in range(self.world)]
        for t in th:
            t.start()
        for t in th:
            t.join(timeout)
        assert not any(t.is_alive() for t in th), "a rank did not return"
        for x in res:
            if isinstance(x, BaseException):
                raise x
        return res

    def sync(self):
        for s in self.streams:
            assert self.L.vr_stream_synchronize(s) == 0


def _cam(vr, cam):
    c = vr.default_camera()
    c.pos[:] = cam[1]; c.front[:] = cam[2]; c.up[:] = cam[3]; c.fov_deg = cam[4]
    return c


def render_frames(vr, L, ranks, vol, axis, cams, dims=DIMS, steps=STEPS):
    """Every rank: for each camera, vr_raycast of its slab into ITS partial buffer (reused across frames) on its
    stream, then vr_compositor_composite at once; rank 0's frames are NaN beforehand.  Returns (frames, partials of
    the last frame), after the streams are synchronised."""
    import torch
    world, w, h = ranks.world, ranks.w, ranks.h
    slabs, params, subs = [], [], []
    for r in range(world):
        bmin, bmax, org, sub, sl = slab_setup(axis, world, r, dims)
        P = vr.default_params(w, h, steps, 2)
        P.box_min[:] = bmin; P.box_max[:] = bmax; P.global_dims[:] = dims; P.vol_origin[:] = org
        slabs.append(torch.from_numpy(np.ascontiguousarray(vol[sl])).cuda().reshape(-1))
        params.append(P)
        subs.append((C.c_int64 * 3)(*sub))
    parts = [torch.empty((h, w, 4), dtype=torch.float32, device="cuda") for _ in range(world)]
    frames = [torch.full((h, w, 4), float("nan"), dtype=torch.float32, device="cuda") for _ in cams]
    torch.cuda.synchronize()            # uploads and NaN fills are on torch's stream, the ranks use their own

    def job(r):
        def go():
            rcs = []
            for k, cam in enumerate(cams):
                c = _cam(vr, cam)
                rcs.append(L.vr_raycast(C.c_void_p(slabs[r].data_ptr()), subs[r], C.byref(c), C.byref(params[r]),
                                        C.c_void_p(parts[r].data_ptr()), ranks.streams[r]))
                rcs.append(L.vr_compositor_composite(ranks.comps[r], C.c_void_p(parts[r].data_ptr()), axis, C.byref(c),
                                                     C.byref(params[r]),
                                                     C.c_void_p(frames[k].data_ptr()) if r == 0 else None,
                                                     ranks.streams[r]))
            return rcs
        return go

    rcs = ranks.run([job(r) for r in range(world)])
    ranks.sync()
    assert all(rc == 0 for x in rcs for rc in x), (rcs, ranks.errors())
    return [f.cpu().numpy().astype(np.float64) for f in frames], torch.stack([p.reshape(-1, 4) for p in parts], 0)


def check_log(log, world, w, h, frames=1):
    """Check 1: per rank and group, exactly the traffic the direct-send exchange needs, every group closed."""
    rows = [hi - lo for lo, hi in (shard(h, r, world) for r in range(world))]
    for r in range(world):
        mine = [e for e in log if e[1] == r]
        for f in range(frames):
            for grp in (2 * f, 2 * f + 1):
                ev = [e for e in mine if e[0] == grp]
                assert ev and ev[0][3] == GROUP_START and ev[-1][3] == GROUP_END, (r, grp, ev)
                assert sum(e[3] == GROUP_START for e in ev) == 1 and sum(e[3] == GROUP_END for e in ev) == 1
                got = sorted((e[3], e[2], e[4]) for e in ev[1:-1])
                if grp % 2 == 0:
                    want = sorted([(SEND, p, rows[p] * w * 4) for p in range(world) if p != r] +
                                  [(RECV, p, rows[r] * w * 4) for p in range(world) if p != r])
                else:
                    want = [(SEND, 0, rows[r] * w * 4)] if r else sorted((RECV, p, rows[p] * w * 4) for p in range(1, world))
                assert got == want, (r, grp, got, want)
        assert len(mine) == sum(2 + (2 * (world - 1)) for _ in range(frames)) + sum(
            2 + (1 if r else world - 1) for _ in range(frames)), (r, len(mine))


def check_frame(vr, frame, stack, cam, axis, w, h, vol, ref_parts, ref_frame, parts_np, world, steps=STEPS):
    """Checks 2 to 4 on one frame."""
    import torch
    from volumerenderer_amd import distributed as D
    assert not np.isnan(frame).any()
    # 2. lossless exchange: one vr_composite_slabs over the stacked full-frame partials, first_pixel = 0
    c = _cam(vr, cam)
    P = vr.default_params(w, h, steps, 0)
    one = D._gpu_combine(stack.contiguous(), 0, axis, c, P)
    torch.cuda.synchronize()
    assert np.array_equal(one.cpu().numpy().reshape(h, w, 4), frame.astype(np.float32)), "exchange or tile offset bug"
    # 3. every partial against the float64 partial of the global volume
    if parts_np is not None:
        for r in range(world):
            d = np.abs(parts_np[r] - ref_parts[r])
            assert (d > TOL).mean() <= PARTIAL_FRAC and np.median(d) < 1e-5, (r, float((d > TOL).mean()), float(np.median(d)))
    # 4. the frame against the order-free float64 reference and the single pass
    d = np.abs(frame - ref_frame)
    assert d.max() <= TOL and np.median(d) < 1e-5, (float(d.max()), float(np.median(d)))
    vdims = (vol.shape[2], vol.shape[1], vol.shape[0])
    dvol = torch.from_numpy(np.ascontiguousarray(vol)).cuda().reshape(-1)
    P.mode = 0
    P.no_early_exit = 1
    single = vr.raycast(dvol, vdims, c, P).cpu().numpy()
    assert np.abs(frame - single).max() <= TOL
    P.no_early_exit = 0
    single = vr.raycast(dvol, vdims, c, P).cpu().numpy()
    assert np.abs(frame - single).max() <= 0.017


CASES = [(wd, ax, cam[0]) for wd in WORLDS for ax in (0, 1, 2) for cam in cameras(ax)]


@pytest.mark.parametrize("world,axis,cam_name", CASES, ids=["w%d-ax%d-%s" % c for c in CASES])
def test_compositor_exchange(vr, L, LB, volume, world, axis, cam_name):
    cam = [c for c in cameras(axis) if c[0] == cam_name][0]
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        (frame,), stack = render_frames(vr, L, ranks, volume, axis, [cam])
        check_log(ranks.log(), world, W, H)
        assert ranks.errors() == ""
    finally:
        ranks.close()
    parts_np = stack.cpu().numpy().reshape(world, H, W, 4).astype(np.float64)
    ref_parts, ref_frame = reference(volume, cam, axis, world, W, H)
    check_frame(vr, frame, stack, cam, axis, W, H, volume, ref_parts, ref_frame, parts_np, world)
    # 5. the scene can tell a wrong view order from the right one.  (The orbit camera's sign change lies on row 30,
    # in rank 0's tile at world 2 -- rows 0-30 -- and its rays below row 30 never leave slab 0 there: the tilted
    # "inside" camera covers a misplaced tile order at world 2.)
    tile_shift = cam_name == "inside" or (cam_name == "orbit30" and world > 2)
    sens = sensitivity(ref_parts, ref_frame, cam, axis, world, W, H, tile_shift)
    assert all(v >= 0.01 for v in sens.values()), sens


@pytest.mark.parametrize("world", WORLDS)
def test_one_row_per_tile(vr, L, LB, volume, world):
    """H == world: every tile is one row (axis 1; the orbit camera raised to y = 0.15, so that the rays below the
    middle cross slabs too; W = 4 H + 1 keeps the cube in view)."""
    o = orbit(30.0)
    cam = ("orbit30-raised", (o[1][0], 0.15, o[1][2]), o[2], o[3], o[4])
    w, h = 4 * world + 1, world
    ranks = Ranks(vr, L, LB, world, w, h)
    try:
        (frame,), stack = render_frames(vr, L, ranks, volume, 1, [cam])
        check_log(ranks.log(), world, w, h)
    finally:
        ranks.close()
    parts_np = stack.cpu().numpy().reshape(world, h, w, 4).astype(np.float64)
    ref_parts, ref_frame = reference(volume, cam, 1, world, w, h)
    check_frame(vr, frame, stack, cam, 1, w, h, volume, ref_parts, ref_frame, parts_np, world)
    sens = sensitivity(ref_parts, ref_frame, cam, 1, world, w, h, tile_shift=True)
    assert all(v >= 0.01 for v in sens.values()), sens


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_single_rank_through_the_new_constructor(vr, L, LB, volume, axis):
    """world = 1 with a caller's transport: no transport call, the frame is the colour transfer of the partial."""
    cam = cameras(axis)[0]
    ranks = Ranks(vr, L, LB, 1, W, H)
    try:
        (frame,), stack = render_frames(vr, L, ranks, volume, axis, [cam])
        assert ranks.log() == []
    finally:
        ranks.close()
    ref_parts, ref_frame = reference(volume, cam, axis, 1, W, H)
    check_frame(vr, frame, stack, cam, axis, W, H, volume, ref_parts, ref_frame,
                stack.cpu().numpy().reshape(1, H, W, 4).astype(np.float64), 1)


def test_compositors_reused_back_to_back(vr, L, LB, volume):
    """The same compositors and partial buffers composite three frames with different cameras, queued without a host
    synchronisation between them."""
    world, axis = 5, 2
    cams = cameras(axis)
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        frames, stack = render_frames(vr, L, ranks, volume, axis, cams)
        check_log(ranks.log(), world, W, H, frames=3)
    finally:
        ranks.close()
    for k, cam in enumerate(cams):
        ref_parts, ref_frame = reference(volume, cam, axis, world, W, H)
        last = k == len(cams) - 1
        if last:
            check_frame(vr, frames[k], stack, cam, axis, W, H, volume, ref_parts, ref_frame,
                        stack.cpu().numpy().reshape(world, H, W, 4).astype(np.float64), world)
        else:
            d = np.abs(frames[k] - ref_frame)
            assert not np.isnan(frames[k]).any() and d.max() <= TOL and np.median(d) < 1e-5, (k, float(d.max()))


def test_bench_shaped_frame(vr, L, LB):
    """1920 x 1080, eight ranks, y-slabs of a 64^3 volume, the orbit camera at two angles (bench.py's strong leg):
    check 2 and the single pass on the full frame, the float64 reference on the middle rows and every tile's first and
    last row."""
    import torch
    from volumerenderer_amd import distributed as D
    w, h, world, axis = 1920, 1080, 8, 1
    dims = (64, 64, 64)
    steps = (128, 128, 128)
    vol = scene_volume(dims, seed=9)
    tiles = [shard(h, r, world) for r in range(world)]
    rows = sorted({0, 539, 540, 1079} | {lo for lo, _ in tiles} | {hi - 1 for _, hi in tiles})
    cams = [orbit(30.0), orbit(200.0)]
    for cam in cams:
        ranks = Ranks(vr, L, LB, world, w, h)
        try:
            (frame,), stack = render_frames(vr, L, ranks, vol, axis, [cam], dims=dims, steps=steps)
            check_log(ranks.log(), world, w, h)
        finally:
            ranks.close()
        c = _cam(vr, cam)
        P = vr.default_params(w, h, steps, 0)
        got = D._gpu_combine(stack.contiguous(), 0, axis, c, P)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy().reshape(h, w, 4), frame.astype(np.float32))
        dvol = torch.from_numpy(vol).cuda().reshape(-1)
        P.no_early_exit = 1
        single = vr.raycast(dvol, dims, c, P).cpu().numpy()
        assert np.abs(frame - single).max() <= TOL
        P.no_early_exit = 0
        assert np.abs(frame - vr.raycast(dvol, dims, c, P).cpu().numpy()).max() <= 0.017
        cov, vuv, g = rays(cam[1], cam[2], cam[3], cam[4], w, h, rows=rows)
        ref = march_composite(vol, cov, vuv, g, tuple(1.0 / s for s in steps), early_exit=False)
        # float32 against float64 over 30 720 pixels: a sample within rounding of a cube face is taken by one and
        # not the other (measured: 1 and 2 pixels, up to 0.013, for the two angles); the small frames see none
        d = np.abs(frame[rows] - ref)
        assert (d > TOL).any(-1).mean() <= 2e-4 and np.median(d) < 1e-5, (cam[0], int((d > TOL).any(-1).sum()))


# ---- errors ----------------------------------------------------------------------------------------------------------
def test_wrong_frame_size_is_refused_before_any_transport_call(vr, L, LB):
    import torch
    world = 3
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        part = torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda")
        out = torch.zeros((H, W + 1, 4), dtype=torch.float32, device="cuda")
        c = vr.default_camera()
        for bad in ((W + 1, H), (W, H + 1), (W - 1, H - 1)):
            P = vr.default_params(bad[0], bad[1], STEPS, 2)
            for r in range(world):
                assert L.vr_compositor_composite(ranks.comps[r], C.c_void_p(part.data_ptr()), 1, C.byref(c), C.byref(P),
                                                 C.c_void_p(out.data_ptr()) if r == 0 else None, ranks.streams[r]) == VR_ERR_INVALID
        P = vr.default_params(W, H, STEPS, 2)
        assert L.vr_compositor_composite(ranks.comps[0], C.c_void_p(part.data_ptr()), 1, C.byref(c), C.byref(P), None,
                                         ranks.streams[0]) == VR_ERR_INVALID     # rank 0 needs a frame
        assert L.vr_compositor_composite(ranks.comps[1], C.c_void_p(part.data_ptr()), 3, C.byref(c), C.byref(P), None,
                                         ranks.streams[1]) == VR_ERR_INVALID     # axis out of range
        assert ranks.log() == []
    finally:
        ranks.close()


def _exchange(vr, L, ranks, parts, frame, axis=2):
    c = vr.default_camera()
    P = vr.default_params(ranks.w, ranks.h, STEPS, 2)

    def job(r):
        return lambda: L.vr_compositor_composite(ranks.comps[r], C.c_void_p(parts[r].data_ptr()), axis, C.byref(c),
                                                 C.byref(P), C.c_void_p(frame.data_ptr()) if r == 0 else None,
                                                 ranks.streams[r])
    return ranks.run([job(r) for r in range(ranks.world)])


def test_send_failure_closes_the_group_and_peers_time_out(vr, L, LB):
    """An injected failure of rank 1's first send: rank 1 returns VR_ERR_NO_DEVICE with its group closed, the peers
    return an error from the transport's bounded wait (0.5 s here) instead of hanging."""
    import torch
    world = 3
    ranks = Ranks(vr, L, LB, world, W, H, timeout=0.5)
    try:
        parts = [torch.rand((H, W, 4), device="cuda") for _ in range(world)]
        frame = torch.full((H, W, 4), float("nan"), device="cuda")
        torch.cuda.synchronize()
        LB.lb_fail_at(ranks.fake, 0, 1, 0)
        t0 = time.perf_counter()
        rcs = _exchange(vr, L, ranks, parts, frame)
        assert time.perf_counter() - t0 < 20.0
        ranks.sync()
        assert rcs == [VR_ERR_NO_DEVICE] * world, rcs
        log = ranks.log()
        mine = [e for e in log if e[1] == 1]
        assert [e[3] for e in mine] == [GROUP_START, SEND, GROUP_END], mine       # stopped at the failure, group closed
        for r in (0, 2):
            ev = [e[3] for e in log if e[1] == r]
            assert ev[0] == GROUP_START and ev[-1] == GROUP_END and ev.count(GROUP_START) == 1, ev   # no second group
        err = ranks.errors()
        assert "injected failure" in err and "timed out" in err, err
        assert torch.isnan(frame).all()
    finally:
        ranks.close()


def test_count_mismatch_is_reported_not_copied(vr, L, LB):
    """Rank 2's gather send recorded 4 floats longer than rank 0's recv: every rank fails the group, the error names
    the ranks and counts, and nothing is copied (rank 0's frame keeps NaN outside its own tile)."""
    import torch
    world = 3
    ranks = Ranks(vr, L, LB, world, W, H)
    try:
        parts = [torch.rand((H, W, 4), device="cuda") for _ in range(world)]
        frame = torch.full((H, W, 4), float("nan"), device="cuda")
        torch.cuda.synchronize()
        LB.lb_count_delta(ranks.fake, 1, 2, 0, 4)
        rcs = _exchange(vr, L, ranks, parts, frame)
        ranks.sync()
        assert rcs == [VR_ERR_NO_DEVICE] * world, rcs
        tiles = [shard(H, r, world) for r in range(world)]
        n2 = (tiles[2][1] - tiles[2][0]) * W * 4
        err = ranks.errors()
        assert ("rank 2 sends %d floats to rank 0, which receives %d" % (n2 + 4, n2)) in err, err
        f = frame.cpu().numpy()
        assert not np.isnan(f[:tiles[0][1]]).any() and np.isnan(f[tiles[0][1]:]).all()
    finally:
        ranks.close()


def test_loopback_refuses_calls_outside_a_group(vr, L, LB):
    """The fake itself: send and group_end outside a group are errors (vr_transport member 2 is send)."""
    import torch
    fake = LB.lb_create(2, 1.0)
    try:
        table = C.cast(C.c_void_p(LB.lb_transport()), C.POINTER(C.c_void_p))
        group_end = C.CFUNCTYPE(C.c_int32, C.c_void_p)(table[1])
        send = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)(table[2])
        buf = torch.zeros(16, device="cuda")
        ctx = LB.lb_rank_ctx(fake, 0)
        assert send(ctx, buf.data_ptr(), 16, 1, None) != 0
        assert group_end(ctx) != 0
        err = C.create_string_buffer(512)
        LB.lb_errors(fake, err, 512)
        assert "outside a group" in err.value.decode() and "group_end outside" in err.value.decode()
    finally:
        LB.lb_destroy(fake)


def test_composite_sort_last_refuses_bad_partials(vr):
    """distributed.composite_sort_last hands raw pointers to C: dtype, contiguity and shape are checked first."""
    import torch
    from volumerenderer_amd import distributed as D
    cam, P = vr.default_camera(), vr.default_params(W, H, STEPS, 2)
    good = torch.zeros((H, W, 4), dtype=torch.float32, device="cuda")
    for bad in (good.double(), torch.zeros((W, H, 4), device="cuda").transpose(0, 1),
                torch.zeros((H, W, 3), device="cuda"), torch.zeros((H * W, 4), device="cuda")):
        with pytest.raises(ValueError):
            D.composite_sort_last(bad, cam, P, axis=2)
    with pytest.raises(ValueError):
        D.composite_sort_last(good, cam, P, axis=2, out=torch.zeros((H, W + 1, 4), device="cuda"))
    frame = D.composite_sort_last(good, cam, P, axis=2)      # and a good one still goes through
    torch.cuda.synchronize()
    assert frame.shape == (H, W, 4)
