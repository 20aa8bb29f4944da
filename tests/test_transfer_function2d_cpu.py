"""CPU checks of the two-dimensional transfer-function path (vr_raycast_tf2d & co.): the C struct and symbols, argument
checks before the device, TransferFunction2D's own checks, the separable table (Python and the header-only C++ helper
agree bit for bit), the facade under plain g++, and the float64 reference of tests/reftf2d.py against closed forms."""
import ctypes as C
import math
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refhist import hist2d  # noqa: E402
from refmarch import rays  # noqa: E402
from refshade import lattice_gradient, march_shaded  # noqa: E402
from reftf import march_tf  # noqa: E402
from reftf2d import lookup2d, march_tf2d, row_coordinate  # noqa: E402
from test_transfer_function_cpu import _Bufs  # noqa: E402

ENTRIES = ("vr_tf2d_columns_build", "vr_raycast_tf2d", "vr_raycast_pool_tf2d", "vr_raycast_tf2d_partial",
           "vr_raycast_pool_tf2d_partial")


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def test_struct_layout_matches_header():
    from volumerenderer_amd import _lib
    T = _lib.TransferFunction2DDesc
    assert C.sizeof(T) == 40
    assert (T.lut_dev.offset, T.columns_dev.offset, T.rows.offset, T.grad_scale.offset, T.opacity_unit.offset,
            T.background.offset) == (0, 8, 16, 20, 24, 28)
    assert _lib.TF2D_MAX_ROWS == 256 and _lib.HIST_GRAD_BINS == 111


def test_symbols_in_header_binding_and_library(L):
    from volumerenderer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    declared = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", hdr))
    for name in ENTRIES:
        assert name in declared and name in _lib.SIGNATURES and hasattr(L, name), name
    assert "typedef struct vr_transfer_function2d" in hdr and "#define VR_TF2D_MAX_ROWS 256" in hdr


def test_bad_arguments_rejected_before_the_device(L):
    from volumerenderer_amd import _lib
    from volumerenderer_amd import render as R
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)
    try:
        big = B._alloc(3 * 4096 + 64)           # a 3-row table
        cols = B._alloc(512 + 64)
        grid = B._alloc(64)
        cam = R.default_camera()
        dims = (C.c_int64 * 3)(4, 4, 4)
        bd, g = (C.c_int64 * 3)(4, 4, 4), (C.c_int64 * 3)(1, 1, 1)

        def tf(lut=big, columns=cols, rows=3, scale=127.5, unit=0.0, bg=(1.0, 1.0, 1.0)):
            t = _lib.TransferFunction2DDesc()
            t.lut_dev, t.columns_dev, t.rows, t.grad_scale, t.opacity_unit = lut, columns, rows, scale, unit
            t.background[:] = bg
            return t

        def shading(**kw):
            s = R.Shading().desc()
            for k, v in kw.items():
                setattr(s, k, v)
            return s

        def params(mode=_lib.RENDER_SHADED):
            return R.default_params(8, 8, (4, 4, 4), mode)

        def call(t, P=None, sh=None):
            P = P or params()
            tp = C.byref(t) if t is not None else None
            sp = C.byref(sh) if sh is not None else None
            return (L.vr_raycast_tf2d(B.vol, dims, C.byref(cam), C.byref(P), tp, sp, B.img, None),
                    L.vr_raycast_pool_tf2d(B.vol, B.table, bd, g, C.byref(cam), C.byref(P), tp, sp, B.img, None),
                    L.vr_raycast_tf2d_partial(B.vol, dims, C.byref(cam), C.byref(P), tp, sp, B.img, None),
                    L.vr_raycast_pool_tf2d_partial(B.vol, B.table, bd, g, C.byref(cam), C.byref(P), tp, sp, B.img, None))

        INV = (-1,) * 4
        bad = [None, tf(lut=None), tf(lut=big + 4), tf(lut=big + 8), tf(columns=cols + 2), tf(columns=cols + 8),
               tf(rows=1), tf(rows=0), tf(rows=-3), tf(rows=257), tf(scale=0.0), tf(scale=-1.0), tf(scale=math.inf),
               tf(scale=math.nan), tf(unit=-1e-6), tf(unit=math.inf), tf(unit=math.nan), tf(bg=(1.0, math.nan, 1.0)),
               tf(bg=(math.inf, 0.0, 0.0))]
        for k, t in enumerate(bad):
            assert call(t) == INV, k
            assert call(t, sh=shading()) == INV, k
        for mode in (0, 1, 2, 4, -1):            # VR_RENDER_SHADED only, lit or not
            assert call(tf(), params(mode)) == INV, mode
            assert call(tf(), params(mode), shading()) == INV, mode
        for sh in (shading(ambient=-0.1), shading(shininess=math.nan), shading(grad_min=math.inf)):
            assert call(tf(), sh=sh) == INV
        # a skip grid attached without the column summary
        P = params()
        P.skip_cell, P.skip_grid_dev = 4, grid
        assert call(tf(columns=None), P) == INV
        # vr_raycast's own checks still apply; the pool takes vr_raycast_pool's restrictions
        P = params()
        P.width = 0
        assert call(tf(), P) == INV
        P = params()
        P.max_samples = -1
        assert call(tf(), P) == INV
        P = params()
        P.vol_origin[:] = (1, 0, 0)
        assert call(tf(), P)[1::2] == (-1, -1)
        for d in ((0, 4, 4), (4, -1, 4), (1 << 31, 1, 1)):
            assert L.vr_raycast_tf2d(B.vol, (C.c_int64 * 3)(*d), C.byref(cam), C.byref(params()), C.byref(tf()), None, B.img,
                                     None) == -1
        for a in ((None, 3, cols), (big + 4, 3, cols), (big, 1, cols), (big, 257, cols), (big, 3, None), (big, 3, cols + 2)):
            assert L.vr_tf2d_columns_build(a[0], a[1], a[2], None) == -1, a
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback
            NODEV = (-2,) * 4
            assert call(tf()) == NODEV
            assert call(tf(), sh=shading()) == NODEV
            assert call(tf(columns=None)) == NODEV            # no grid attached: the summary may be missing
            assert call(tf(rows=2, scale=1e-3, unit=0.5, bg=(0.0, 0.0, 0.0))) == NODEV
            assert L.vr_tf2d_columns_build(big, 3, cols, None) == -2
    finally:
        B.free()


def test_transfer_function2d_rejects_bad_values():
    pytest.importorskip("torch")
    from volumerenderer_amd.render import TransferFunction2D, tf2d_separable_table
    ok = np.zeros((3, 256, 4), np.float32)
    for lut in (np.full((3, 256, 4), 1.01, np.float32), np.full((3, 256, 4), -0.01, np.float32), np.zeros((256, 4)),
                np.zeros((1, 256, 4)), np.zeros((257, 256, 4)), np.zeros((3, 255, 4)), np.full((3, 256, 4), np.nan)):
        with pytest.raises(ValueError):
            TransferFunction2D(lut, device="cpu")
    for scale in (0.0, -2.0, math.inf, math.nan, 1e-60):
        with pytest.raises(ValueError):
            TransferFunction2D(ok, grad_scale=scale, device="cpu")
    for unit in (-0.5, math.inf, math.nan):
        with pytest.raises(ValueError):
            TransferFunction2D(ok, opacity_unit=unit, device="cpu")
    with pytest.raises(ValueError):
        TransferFunction2D(ok, background=(1.0, math.inf, 0.0), device="cpu")
    lut1 = np.zeros((256, 4), np.float32)
    for w in ([0.5], [0.1, 1.5], [0.1, -0.2], [0.1, math.nan], np.zeros(257), np.zeros((2, 2))):
        with pytest.raises(ValueError):
            tf2d_separable_table(lut1, w)
    with pytest.raises(ValueError):
        tf2d_separable_table(np.zeros((255, 4)), [0.0, 1.0])


def test_host_table_has_its_summary_and_background_and_never_reaches_a_kernel():
    """A valid table built with device="cpu" (what the CPU path of composite_sort_last_tf takes: it reads only the
    background): the column summary is computed on the host, no C call is made with host pointers, and the single-rank
    CPU path finishes a partial through an injected combine."""
    torch = pytest.importorskip("torch")
    from volumerenderer_amd import distributed as D
    from volumerenderer_amd import render as R
    rng = np.random.default_rng(2)
    lut = rng.uniform(0, 1, (5, 256, 4)).astype(np.float32)
    lut[:, :40, 3] = 0.0
    lut[:, 100:130, 3] = 0.0
    lut[3, 110, 3] = 0.25                    # one row alone keeps a column
    lut[:, 250:, 3] = 0.0
    calls = []
    real = R._lib.lib

    def spy():
        calls.append(1)
        return real()

    R._lib.lib = spy
    try:
        tf = R.TransferFunction2D(lut, opacity_unit=0.125, background=(0.25, 0.5, 0.75), device="cpu")
    finally:
        R._lib.lib = real
    assert not calls, "a host table must not reach the library"
    assert not tf.lut.is_cuda and not tf.columns.is_cuda and tf.columns.dtype == torch.int16
    opaque = (lut[:, :, 3] != 0).any(0)
    want, nxt = np.empty(256, np.int64), 256
    for k in range(255, -1, -1):
        nxt = k if opaque[k] else nxt
        want[k] = nxt
    assert np.array_equal(tf.columns.numpy().astype(np.int64), want)
    assert want[0] == 40 and want[100] == 110 and want[111] == 130 and want[250] == 256
    assert tf.rows == 5 and tf.grad_scale == 127.5 * 4 / 110
    d = R.background_desc(tf)
    assert d.lut_dev is None and d.opacity_unit == 0.125 and tuple(d.background) == (0.25, 0.5, 0.75)
    d1 = R.background_desc(R.TransferFunction(lut[0], 0.5, (0.0, 1.0, 0.0), device="cpu"))
    assert d1.lut_dev and tuple(d1.background) == (0.0, 1.0, 0.0)
    with pytest.raises(ValueError):
        R.background_desc("not a table")
    # an all-clear table: nothing opaque anywhere
    clear = R.TransferFunction2D(np.zeros((2, 256, 4), np.float32), device="cpu")
    assert (clear.columns.numpy() == 256).all()
    # one rank, host tensors, an injected combine: the table is asked for nothing
    part = torch.zeros((4, 6, 4))
    part[..., 3] = 1.0
    seen = []

    def combine(parts, first_pixel, axis, cam, params):
        seen.append((tuple(parts.shape), first_pixel, axis))
        return parts[0]

    out = D.composite_sort_last_tf(part, R.default_camera(), R.default_params(6, 4, (4, 4, 4)), tf, axis=1, combine=combine)
    assert seen == [((1, 24, 4), 0, 1)] and torch.equal(out, part)
    with pytest.raises(ValueError):
        D.composite_sort_last_tf(part, R.default_camera(), R.default_params(6, 4, (4, 4, 4)), None, combine=combine)


def test_viewer_style_with_a_two_dimensional_table():
    pytest.importorskip("torch")
    from volumerenderer_amd import _lib
    from volumerenderer_amd import render as R
    from volumerenderer_amd.viewer import _style
    tf = R.TransferFunction2D(np.zeros((2, 256, 4), np.float32), device="cpu")
    sh = R.Shading()
    for mode in (_lib.RENDER_COMPOSITE, _lib.RENDER_SHADED):
        assert _style(mode, tf, None, None) == (_lib.RENDER_SHADED, 4, (tf, None))
        assert _style(mode, tf, sh, None) == (_lib.RENDER_SHADED, 4, (tf, sh))
    for mode in (_lib.RENDER_ISOSURFACE, _lib.RENDER_PARTIAL, _lib.RENDER_PROJECTION, 7):
        with pytest.raises(ValueError):
            _style(mode, tf, None, None)
    with pytest.raises(ValueError):
        _style(_lib.RENDER_COMPOSITE, tf, None, object())       # a projection takes no table


def test_separable_table_by_hand():
    from volumerenderer_amd.render import tf2d_separable_table
    rng = np.random.default_rng(5)
    lut1 = rng.uniform(0, 1, (256, 4)).astype(np.float32)
    w = np.array([0.0, 1.0, 0.3, 1 / 3])
    t = tf2d_separable_table(lut1, w)
    assert t.dtype == np.float32 and t.shape == (4, 256, 4)
    assert all(np.array_equal(t[j, :, :3], lut1[:, :3]) for j in range(4))
    assert (t[0, :, 3] == 0).all() and np.array_equal(t[1, :, 3], lut1[:, 3])
    assert np.array_equal(t[3, :, 3], (lut1[:, 3].astype(np.float64) * (1 / 3)).astype(np.float32))


def _compile_example(tmp_path):
    import __graft_entry__ as g
    g.build()
    exe = str(tmp_path / "transfer_function2d")
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "transfer_function2d.cpp"), "-L" + lib, "-lvrhip",
                           "-Wl,-rpath," + lib, "-o", exe])
    return exe


# examples/transfer_function2d.cpp's table: its control points and row weights
EXAMPLE_POINTS = [(0, 0.0, 0.0, 0.0, 0.0), (30, 0.2, 0.3, 0.6, 0.0), (90, 0.3, 0.5, 0.9, 0.5), (200, 1.0, 0.9, 0.7, 0.9),
                  (255, 1.0, 1.0, 1.0, 0.9)]
EXAMPLE_WEIGHTS = [min(j / 8.0, 1.0) for j in range(111)]


def test_cpp_facade_compiles_and_its_separable_table_equals_python(tmp_path):
    """The facade (TransferFunction.hpp's helper and SortLastTf constructors, Viewer.hpp's overloads) under plain g++ with
    -Wall -Werror, and transfer_function2d_separable against tf2d_separable_table bit for bit."""
    from volumerenderer_amd.render import tf2d_separable_table, transfer_function_table
    exe = _compile_example(tmp_path)
    out = subprocess.run([exe, "table"], capture_output=True, text=True, check=True).stdout.split("\n")
    got = np.array([[float.fromhex(v) for v in line.split()[1:]] for line in out if line], np.float32)
    want = tf2d_separable_table(transfer_function_table(EXAMPLE_POINTS), EXAMPLE_WEIGHTS)
    assert got.shape == (111 * 256, 4)
    assert np.array_equal(got.reshape(111, 256, 4), want)
    # SortLastTf with a two-dimensional table: two halo layers lit or not, the background carried over
    src = tmp_path / "sl.cpp"
    src.write_text('#include "vrhip/Viewer.hpp"\n#include <cstdio>\nint main() {\n'
                   '  vr_camera c = vrhip::HeadlessViewer(8, 8).camera();\n'
                   '  vr_transfer_function2d t = vr_transfer_function2d(); t.background[1] = 0.5f; t.rows = 3;\n'
                   '  vr_transfer_function u = vr_transfer_function();\n'
                   '  vrhip::SortLastTf a(c, t), b(c, t, vrhip::default_shading()), d(c, u), e(c, u, vrhip::default_shading());\n'
                   '  std::printf("%d %d %d %d %g %d %g\\n", a.halo(), b.halo(), d.halo(), e.halo(), a.tf.background[1],\n'
                   '              a.tf.lut_dev == nullptr, vrhip::default_grad_scale(111));\n  return 0; }\n')
    exe2 = str(tmp_path / "sl")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"), str(src),
                           "-L" + os.path.join(ROOT, "volumerenderer_amd"), "-lvrhip",
                           "-Wl,-rpath," + os.path.join(ROOT, "volumerenderer_amd"), "-o", exe2])
    assert subprocess.run([exe2], capture_output=True, text=True, check=True).stdout.split() == ["2", "2", "1", "2", "0.5", "1",
                                                                                                  "127.5"]


def test_cpp_example_fails_loudly_without_gpu(L, tmp_path):
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    if n.value > 0:
        pytest.skip("GPU present: covered by tests/test_gpu_transfer_function2d.py")
    exe = _compile_example(tmp_path)
    r = subprocess.run([exe, "render", str(tmp_path / "f.ppm")], capture_output=True, text=True)
    assert r.returncode != 0 and "no usable HIP device" in (r.stdout + r.stderr)


# ---- the float64 reference against closed forms --------------------------------------------------------------------
CAM = ((0.02, -0.03, -3.0), (0.0, 0.0, 1.0), (0.0, 1.0, 0.0), 6.0)      # far and narrow: every ray crosses z = 0 .. 1
STEP = (1 / 60.5,) * 3


def _row_table(rng, rows):
    """Random colours, alpha a function of the row alone."""
    lut = rng.uniform(0, 1, (rows, 256, 4))
    lut[:, :, 3] = np.linspace(0.0, 0.5, rows)[:, None]
    return lut


def test_reference_constant_volume_reads_row_zero():
    """No gradient anywhere: every sample reads row 0, so the frame is reftf's through row 0 whatever the other rows."""
    rng = np.random.default_rng(1)
    vol = np.full((12, 10, 14), 93, np.uint8)
    lut = rng.uniform(0, 1, (7, 256, 4))
    lut[0, :, 3] *= 0.1
    pos, front, up, fov = CAM
    cov, vuv, g = rays(pos, front, up, fov, 24, 16)
    seen = []
    img = march_tf2d(vol, cov, vuv, g, STEP, lut, 127.5, background=(0.1, 0.2, 0.4), rows_seen=seen)[0]
    assert all((y == 0).all() for y in seen) and sum(len(y) for y in seen) > 24 * 16 * 50
    want, _ = march_tf(vol, cov, vuv, g, STEP, lut[0], background=(0.1, 0.2, 0.4))
    assert np.abs(img - want).max() < 1e-14
    assert (img[..., 3] > 0.5).all()


@pytest.mark.parametrize("slope", [1, 3, 4])
def test_reference_ramp_reads_half_its_slope(slope):
    """A ramp of `slope` grey levels per voxel along z: central differences 2 * slope, |g| = slope / 255, so
    y = slope / 2 at grad_scale 127.5 wherever the taps stay clear of the clamped ends."""
    Z = 255 // slope
    vol = np.broadcast_to((slope * np.arange(Z)).astype(np.uint8)[:, None, None], (Z, 6, 6)).copy()
    rng = np.random.default_rng(slope)
    p = rng.uniform(0.0, 1.0, (500, 3))
    p[:, 2] = rng.uniform(2.0 / Z, 1.0 - 2.0 / Z, 500)
    m = np.linalg.norm(lattice_gradient(vol, p), axis=-1)
    y, j, h = row_coordinate(m, 127.5, 111)
    assert np.abs(y - slope / 2).max() < 1e-12
    lut = _row_table(rng, 111)
    e = lookup2d(lut, np.full(500, 0.5), m, 127.5)
    a = np.linspace(0.0, 0.5, 111)
    assert np.abs(e[:, 3] - (a[slope // 2] + (slope / 2 - slope // 2) * (a[slope // 2 + 1] - a[slope // 2]))).max() < 1e-12
    # the clamp: a scale that puts y far beyond the table reads the top row
    y, j, h = row_coordinate(m, 1e6, 111)
    assert (y == 110).all() and (j == 109).all() and (h == 1).all()
    assert np.abs(lookup2d(lut, np.full(500, 0.5), m, 1e6)[:, 3] - 0.5).max() < 1e-15


@pytest.mark.parametrize("rows,scale", [(2, 127.5), (3, 40.0), (111, 127.5), (111, 3000.0)])
def test_reference_equal_rows_equal_the_one_dimensional_references(rows, scale):
    rng = np.random.default_rng(rows)
    vol = rng.integers(0, 256, (10, 12, 9), dtype=np.uint8)
    lut1 = rng.uniform(0, 1, (256, 4))
    lut1[:, 3] *= 0.3
    lut = np.broadcast_to(lut1, (rows, 256, 4))
    cov, vuv, g = rays((0.3, 0.2, -1.5), (-0.2, -0.1, 1.0), (0, 1, 0), 30.0, 20, 14)
    step = (1 / 32, 1 / 40, 1 / 28)
    for unit, early in ((0.0, True), (1 / 50, False)):
        got = march_tf2d(vol, cov, vuv, g, step, lut, scale, None, unit, (0.2, 0.3, 0.4), early_exit=early)[0]
        want = march_tf(vol, cov, vuv, g, step, lut1, unit, (0.2, 0.3, 0.4), early_exit=early)[0]
        assert np.abs(got - want).max() < 1e-13
        sh = (0.3, 0.6, 0.2, 8.0, (0.5, 0.7, -0.4), 1 / 255)
        got = march_tf2d(vol, cov, vuv, g, step, lut, scale, sh, unit, (0.2, 0.3, 0.4), early_exit=early)
        want = march_shaded(vol, cov, vuv, g, step, lut1, sh, unit, (0.2, 0.3, 0.4), early_exit=early)
        assert np.abs(got[0] - want[0]).max() < 1e-13
        for a, b in zip(got[1:], want[1:]):
            assert np.array_equal(a, b)
    assert (got[0][..., 3][cov] > 0.2).mean() > 0.5


def test_reference_row_at_voxel_centres_is_the_histogram_row():
    """At a voxel centre the lattice gradient is that voxel's central differences, y = |d| / 4 at grad_scale 127.5, and
    floor(y) is the row vr_histogram2d counts the voxel in: the two share one design space."""
    rng = np.random.default_rng(9)
    X, Y, Z = 11, 9, 7
    vol = rng.integers(0, 256, (Z, Y, X), dtype=np.uint8)
    vol[:3] //= 16                                                      # small gradients too
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    p = np.stack([(xx + 0.5) / X, (yy + 0.5) / Y, (zz + 0.5) / Z], -1)
    g = lattice_gradient(vol, p)
    d2 = np.rint((g * 510.0) ** 2).sum(-1).astype(np.int64)             # the integer squared length of d
    y = np.sqrt(d2.astype(np.float64)) / 4.0                            # exact input: no rounding of the gradient
    # rows from the reference's own y agree wherever y is not within rounding of an integer
    yr, _, _ = row_coordinate(np.linalg.norm(g, axis=-1), 127.5, 111)
    assert np.abs(yr - y).max() < 1e-9
    clear = np.abs(y - np.rint(y)) > 1e-6
    assert np.array_equal(np.floor(yr)[clear], np.floor(y)[clear])
    rows = np.minimum(np.floor(np.where(clear, y, np.rint(y))).astype(np.int64), 110)
    want = hist2d(vol)
    got = np.bincount((rows * 256 + vol).reshape(-1), minlength=111 * 256).reshape(111, 256)
    assert np.array_equal(got, want.astype(np.int64))
    assert rows.max() > 60 and rows.min() == 0
