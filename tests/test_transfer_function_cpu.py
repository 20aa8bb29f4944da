"""CPU checks of the transfer-function path (vr_raycast_tf / vr_raycast_pool_tf): the C struct, argument checks before
the device, the table from control points (Python and the header-only C++ helper agree bit for bit), and the float64
reference compositor of tests/reftf.py against closed forms."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays  # noqa: E402
from reftf import lookup, march_tf, ray_samples  # noqa: E402

# the control points of examples/transfer_function.cpp
EXAMPLE_POINTS = [(0, 0.0, 0.0, 0.0, 0.0), (40, 0.1, 0.3, 0.9, 0.0), (90, 0.9, 0.6, 0.1, 0.35), (255, 1.0, 1.0, 1.0, 0.8)]


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def test_struct_layout_matches_header():
    from volumerenderer_amd import _lib
    T = _lib.TransferFunctionDesc
    assert C.sizeof(T) == 24
    assert (T.lut_dev.offset, T.opacity_unit.offset, T.background.offset) == (0, 8, 12)


def test_symbols_exported(L):
    from volumerenderer_amd import _lib
    for name in ("vr_raycast_tf", "vr_raycast_pool_tf"):
        assert hasattr(L, name) and name in _lib.SIGNATURES


class _Bufs:
    """Buffers for the argument checks: host memory on a box without a device (nothing may be launched there), device
    memory of the right sizes where there is one, so that no call can touch memory it does not own."""

    def __init__(self, L, ndev):
        self.L, self.ndev, self.dev, self.keep = L, ndev, [], []
        self.vol, self.img, self.lut, self.table = [self._alloc(n) for n in (64, 8 * 8 * 16, 4096 + 64, 16)]

    def _alloc(self, nbytes):
        if self.ndev > 0:
            p = C.c_void_p()
            assert self.L.vr_malloc(C.byref(p), nbytes) == 0
            self.dev.append(p)
            return p.value
        b = (C.c_uint8 * (nbytes + 16))()
        self.keep.append(b)
        a = C.addressof(b)
        return a + (-a % 16)

    def free(self):
        for p in self.dev:
            self.L.vr_free(p)


def test_bad_arguments_rejected_before_the_device(L):
    from volumerenderer_amd import _lib
    from volumerenderer_amd import render as R
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)
    try:
        cam = R.default_camera()
        dims = (C.c_int64 * 3)(4, 4, 4)
        bd, grid = (C.c_int64 * 3)(4, 4, 4), (C.c_int64 * 3)(1, 1, 1)

        def tf(lut=B.lut, unit=0.0, bg=(1.0, 1.0, 1.0)):
            t = _lib.TransferFunctionDesc()
            t.lut_dev, t.opacity_unit = lut, unit
            t.background[:] = bg
            return t

        def call(t, P=None):
            P = P or R.default_params(8, 8, (4, 4, 4))
            tp = C.byref(t) if t is not None else None
            a = L.vr_raycast_tf(B.vol, dims, C.byref(cam), C.byref(P), tp, B.img, None)
            b = L.vr_raycast_pool_tf(B.vol, B.table, bd, grid, C.byref(cam), C.byref(P), tp, B.img, None)
            return a, b

        bad = [None, tf(lut=None), tf(lut=B.lut + 4), tf(lut=B.lut + 8), tf(unit=-1e-6), tf(unit=math.inf),
               tf(unit=math.nan), tf(bg=(1.0, math.nan, 1.0)), tf(bg=(math.inf, 0.0, 0.0)), tf(bg=(0.0, 0.0, -math.inf))]
        for k, t in enumerate(bad):
            assert call(t) == (-1, -1), k
        for mode in (1, 2, 3, -1):
            P = R.default_params(8, 8, (4, 4, 4), mode)
            assert call(tf(), P) == (-1, -1), mode
        # vr_raycast's own checks still apply
        P = R.default_params(8, 8, (4, 4, 4))
        P.width = 0
        assert call(tf(), P) == (-1, -1)
        P = R.default_params(8, 8, (4, 4, 4))
        P.vol_origin[:] = (1, 0, 0)          # the pool takes vr_raycast_pool's restrictions
        assert L.vr_raycast_pool_tf(B.vol, B.table, bd, grid, C.byref(cam), C.byref(P), C.byref(tf()), B.img, None) == -1
        nbd = (C.c_int64 * 3)(4, 6, 4)       # not a power of two
        assert L.vr_raycast_pool_tf(B.vol, B.table, nbd, grid, C.byref(cam), C.byref(R.default_params(8, 8, (4, 4, 4))),
                                    C.byref(tf()), B.img, None) == -1
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback
            assert call(tf()) == (-2, -2)
            assert call(tf(unit=0.5, bg=(0.0, 0.0, 0.0))) == (-2, -2)
    finally:
        B.free()


def test_table_from_points_by_hand():
    from volumerenderer_amd.render import transfer_function_table
    pts = [(10, 0.0, 0.5, 1.0, 0.0), (20, 1.0, 0.5, 0.0, 1.0), (200, 0.2, 0.4, 0.6, 0.5)]
    t = transfer_function_table(pts)
    assert t.dtype == np.float32 and t.shape == (256, 4)
    f = np.float32
    for k in range(0, 11):                                    # clamped below the first point
        assert np.array_equal(t[k], np.array([0.0, 0.5, 1.0, 0.0], f)), k
    assert np.array_equal(t[15], np.array([0.5, 0.5, 0.5, 0.5], f))
    assert np.array_equal(t[20], np.array([1.0, 0.5, 0.0, 1.0], f))
    assert np.array_equal(t[110], np.array([1.0 + 0.5 * (0.2 - 1.0), 0.5 + 0.5 * (0.4 - 0.5), 0.6 * 0.5, 1.0 - 0.25], f))
    assert np.array_equal(t[21], np.array([1.0 + (1 / 180) * -0.8, 0.5 + (1 / 180) * -0.1, (1 / 180) * 0.6,
                                           1.0 + (1 / 180) * -0.5], f))
    for k in range(200, 256):                                 # clamped past the last point
        assert np.array_equal(t[k], np.array([0.2, 0.4, 0.6, 0.5], f)), k
    # one point: constant; a repeated value: a step (the later point from that value on)
    assert np.array_equal(transfer_function_table([(77, 0.1, 0.2, 0.3, 0.4)]), np.tile(np.array([0.1, 0.2, 0.3, 0.4], f), (256, 1)))
    s = transfer_function_table([(0, 0, 0, 0, 0), (100, 0, 0, 0, 0), (100, 1, 1, 1, 1), (255, 1, 1, 1, 1)])
    assert (s[:100] == 0).all() and (s[100:] == 1).all()


@pytest.mark.parametrize("pts", [[], [(10, 0.0, 0.0, 0.0)], [(256, 0, 0, 0, 0)], [(-1, 0, 0, 0, 0)],
                                 [(10, 0, 0, 0, 1.5)], [(10, 0, -0.1, 0, 0)], [(20, 0, 0, 0, 0), (10, 0, 0, 0, 0)],
                                 [(math.nan, 0, 0, 0, 0)]])
def test_table_from_points_rejects(pts):
    from volumerenderer_amd.render import transfer_function_table
    with pytest.raises(ValueError):
        transfer_function_table(pts)


def test_transfer_function_rejects_bad_values():
    pytest.importorskip("torch")
    from volumerenderer_amd.render import TransferFunction
    ok = np.zeros((256, 4), np.float32)
    for lut in (np.full((256, 4), 1.01, np.float32), np.full((256, 4), -0.01, np.float32), np.zeros((255, 4)),
                np.full((256, 4), np.nan)):
        with pytest.raises(ValueError):
            TransferFunction(lut, device="cpu")
    for unit in (-0.5, math.inf, math.nan):
        with pytest.raises(ValueError):
            TransferFunction(ok, opacity_unit=unit, device="cpu")
    with pytest.raises(ValueError):
        TransferFunction(ok, background=(1.0, math.inf, 0.0), device="cpu")
    with pytest.raises(ValueError):
        TransferFunction.from_points([(0, 0, 0, 0, 2.0)], device="cpu")
    t = TransferFunction.from_points(EXAMPLE_POINTS, 0.25, (0.0, 0.5, 1.0), device="cpu")
    d = t.desc()
    assert d.opacity_unit == 0.25 and tuple(d.background) == (0.0, 0.5, 1.0)


def _compile_example(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "transfer_function")
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "transfer_function.cpp"), "-L" + lib, "-lvrhip",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


def test_cpp_table_equals_python(tmp_path):
    from volumerenderer_amd.render import transfer_function_table
    exe = _compile_example(tmp_path)
    out = subprocess.run([exe, "table"], capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([[float.fromhex(v) for v in line.split()[1:]] for line in out if line], np.float32)
    assert got.shape == (256, 4)
    assert np.array_equal(got, transfer_function_table(EXAMPLE_POINTS))


def test_cpp_example_fails_loudly_without_gpu(tmp_path):
    exe = _compile_example(tmp_path)
    from volumerenderer_amd import _lib
    n = C.c_int32(-1)
    assert _lib.lib().vr_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("GPU present: covered by tests/test_gpu_transfer_function.py")
    r = subprocess.run([exe, "render", str(tmp_path / "f.bin")], capture_output=True, text=True)
    assert r.returncode != 0 and "no usable HIP device" in (r.stdout + r.stderr)


# ---- the float64 reference against closed forms --------------------------------------------------------------------
CAM = ((0.02, -0.03, -3.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 6.0)      # far and narrow: every ray crosses z = 0 .. 1
STEP = (1 / 60.5,) * 3


def _inside_samples(covered, vuv, g, step, max_samples):
    """n per ray: how many of pos_k = vUV + k st (k = 1 .. max_samples) lie strictly inside the cube before the first
    that does not (the rays of CAM are far from every face but z = 0 and z = 1 at the steps taken)."""
    st = g * np.asarray(step)
    n = np.zeros(covered.shape, np.int64)
    alive = covered.copy()
    for k in range(1, max_samples + 1):
        p = vuv + k * st
        alive &= ((p > 0) & (p < 1)).all(-1)
        n += alive
    return n


@pytest.mark.parametrize("value", [0, 77, 255])
def test_reference_constant_volume_constant_table(value):
    """C = rgb (1 - (1 - a)^n), T = (1 - a)^n over the n inside samples, without early exit; with it, the march stops at
    the first sample with T < 0.01."""
    vol = np.full((12, 10, 14), value, np.uint8)
    rgba = np.array([0.3, 0.6, 0.9, 0.07])
    lut = np.tile(rgba, (256, 1))
    W, H = 24, 16
    pos, front, up, fov = CAM
    cov, vuv, g = rays(pos, front, up, fov, W, H)
    assert cov.all()
    n = _inside_samples(cov, vuv, g, STEP, 300)
    assert (n >= 58).all() and (n <= 62).all()
    bg = np.array([0.1, 0.2, 0.4])
    img, _ = march_tf(vol, cov, vuv, g, STEP, lut, background=bg, early_exit=False)
    T = (1 - rgba[3]) ** n
    want = np.concatenate([rgba[:3] * (1 - T)[..., None] + T[..., None] * bg, (1 - T)[..., None]], -1)
    assert np.abs(img - want).max() < 1e-12
    # early exit: (1 - 0.07)^k < 0.01 first at k = 64 > n: never; with a = 0.2, first at k = 21
    lut[:, 3] = 0.2
    img, _ = march_tf(vol, cov, vuv, g, STEP, lut, background=bg)
    T = 0.8 ** np.minimum(n, 21)
    assert np.abs(img[..., 3] - (1 - T)).max() < 1e-12


def test_reference_opacity_correction_halves_the_unit_doubles_the_sample():
    """opacity_unit = L / 2 composites each sample as two samples of the uncorrected alpha."""
    rng = np.random.default_rng(3)
    vol = rng.integers(0, 256, (10, 12, 9), dtype=np.uint8)
    lut = np.clip(np.stack([np.linspace(0, 1, 256), np.linspace(1, 0, 256), np.full(256, 0.5),
                            0.3 * np.abs(np.sin(np.linspace(0, 4, 256)))], -1), 0, 1)
    W, H = 20, 14
    cov, vuv, g = rays((0.3, 0.2, -1.5), (-0.2, -0.1, 1.0), (0, 1, 0), 30.0, W, H)
    step = (1 / 32,) * 3                     # isotropic: L = 1/32 on every ray
    got, _ = march_tf(vol, cov, vuv, g, step, lut, opacity_unit=1 / 64, early_exit=False)
    C3, T = np.zeros(cov.shape + (3,)), np.ones(cov.shape)
    for take, s in ray_samples(vol, cov, vuv, g, step):
        e = lookup(lut, s)
        a = np.where(take, e[..., 3], 0.0)
        for _ in range(2):
            C3 += (T * a)[..., None] * e[..., :3]
            T = T * (1 - a)
    want = np.concatenate([C3 + T[..., None], (1 - T)[..., None]], -1)
    assert np.abs(got - want).max() < 1e-12
    assert (got[..., 3][cov] > 0.2).mean() > 0.5


def test_reference_exact_alpha_ends():
    """e.a = 0 composites nothing and e.a = 1 stops the light at once, with and without the correction."""
    vol = np.full((8, 8, 8), 128, np.uint8)
    W, H = 8, 8
    pos, front, up, fov = CAM
    cov, vuv, g = rays(pos, front, up, fov, W, H)
    for unit in (0.0, 0.01, 0.5):
        img, _ = march_tf(vol, cov, vuv, g, STEP, np.zeros((256, 4)), unit, (0.25, 0.5, 0.75))
        assert np.array_equal(img, np.broadcast_to([0.25, 0.5, 0.75, 0.0], img.shape))
        lut = np.tile([0.9, 0.8, 0.7, 1.0], (256, 1))
        img, _ = march_tf(vol, cov, vuv, g, STEP, lut, unit, (0.25, 0.5, 0.75))
        assert np.array_equal(img, np.broadcast_to([0.9, 0.8, 0.7, 1.0], img.shape))
