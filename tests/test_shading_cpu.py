"""CPU checks of the gradient-shaded path (vr_raycast_tf_shaded / vr_raycast_pool_tf_shaded): the C struct, argument
checks before the device, the Python Shading checks, the float64 reference of tests/refshade.py against closed forms,
and vr_lod_select's two-voxel grow in VR_RENDER_SHADED mode."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from refmarch import rays  # noqa: E402
from refshade import lattice_gradient, march_shaded, shade  # noqa: E402
from reftf import march_tf  # noqa: E402
from test_lod_select import _cam, _grid_ijk, rule  # noqa: E402
from test_transfer_function_cpu import _Bufs  # noqa: E402


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def test_struct_layout_matches_header():
    from volumerenderer_amd import _lib
    S = _lib.ShadingDesc
    assert C.sizeof(S) == 32
    assert (S.ambient.offset, S.diffuse.offset, S.specular.offset, S.shininess.offset, S.light_dir.offset,
            S.grad_min.offset) == (0, 4, 8, 12, 16, 28)
    assert _lib.RENDER_SHADED == 3


def test_symbols_exported(L):
    from volumerenderer_amd import _lib
    for name in ("vr_raycast_tf_shaded", "vr_raycast_pool_tf_shaded"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    import volumerenderer_amd as vr
    for name in ("Shading", "raycast_tf_shaded", "raycast_pool_tf_shaded"):
        assert getattr(vr, name) is not None


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
        tf = _lib.TransferFunctionDesc()
        tf.lut_dev, tf.opacity_unit = B.lut, 0.0
        tf.background[:] = (1.0, 1.0, 1.0)

        def sh(**kw):
            s = R.Shading().desc()
            for k, v in kw.items():
                if k == "light_dir":
                    s.light_dir[:] = v
                else:
                    setattr(s, k, v)
            return s

        def call(s, P=None, t=tf):
            P = P or R.default_params(8, 8, (4, 4, 4), _lib.RENDER_SHADED)
            sp = C.byref(s) if s is not None else None
            a = L.vr_raycast_tf_shaded(B.vol, dims, C.byref(cam), C.byref(P), C.byref(t), sp, B.img, None)
            b = L.vr_raycast_pool_tf_shaded(B.vol, B.table, bd, grid, C.byref(cam), C.byref(P), C.byref(t), sp, B.img, None)
            return a, b

        bad = [None]
        for f in ("ambient", "diffuse", "specular", "shininess", "grad_min"):
            bad += [sh(**{f: -1e-6}), sh(**{f: math.nan}), sh(**{f: math.inf})]
        bad += [sh(light_dir=(0.0, math.nan, 1.0)), sh(light_dir=(math.inf, 0.0, 0.0))]
        for k, s in enumerate(bad):
            assert call(s) == (-1, -1), k
        for mode in (0, 1, 2, -1, 4):
            assert call(sh(), R.default_params(8, 8, (4, 4, 4), mode)) == (-1, -1), mode
        badtf = _lib.TransferFunctionDesc()
        badtf.lut_dev, badtf.opacity_unit = B.lut + 4, 0.0
        assert call(sh(), t=badtf) == (-1, -1)
        # vr_raycast_tf still rejects the new mode
        P = R.default_params(8, 8, (4, 4, 4), _lib.RENDER_SHADED)
        assert L.vr_raycast_tf(B.vol, dims, C.byref(cam), C.byref(P), C.byref(tf), B.img, None) == -1
        assert L.vr_raycast_pool_tf(B.vol, B.table, bd, grid, C.byref(cam), C.byref(P), C.byref(tf), B.img, None) == -1
        assert L.vr_raycast(B.vol, dims, C.byref(cam), C.byref(P), B.img, None) == -1
        P = R.default_params(8, 8, (4, 4, 4), _lib.RENDER_SHADED)
        P.vol_origin[:] = (1, 0, 0)          # the pool takes vr_raycast_pool's restrictions
        assert L.vr_raycast_pool_tf_shaded(B.vol, B.table, bd, grid, C.byref(cam), C.byref(P), C.byref(tf), C.byref(sh()),
                                           B.img, None) == -1
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback; a negative light direction is a direction
            assert call(sh()) == (-2, -2)
            assert call(sh(light_dir=(-1.0, -2.0, 0.5), ambient=0.0, shininess=0.0, grad_min=0.0)) == (-2, -2)
    finally:
        B.free()


@pytest.mark.parametrize("kw", [{"ambient": -0.1}, {"diffuse": math.nan}, {"specular": math.inf}, {"shininess": -1},
                                {"grad_min": -1e-9}, {"light_dir": (0, 0)}, {"light_dir": (0, math.nan, 0)}])
def test_python_shading_rejects(kw):
    from volumerenderer_amd.render import Shading
    with pytest.raises(ValueError):
        Shading(**kw)


def test_python_shading_defaults():
    from volumerenderer_amd.render import Shading
    d = Shading().desc()
    f = np.float32
    assert (d.ambient, d.diffuse, d.specular, d.shininess) == (f(0.3), f(0.7), f(0.2), f(32.0))
    assert tuple(d.light_dir) == (0.0, 0.0, 0.0) and d.grad_min == f(1 / 255)


# ---- the reference in closed forms ---------------------------------------------------------------------------------
def test_linear_ramp_gives_a_constant_gradient_and_normal():
    X, Y, Z = 20, 12, 10
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    vol = (3 * xx + 5 * yy + 7 * zz).astype(np.uint8)
    rng = np.random.default_rng(3)
    # positions whose taps and neighbours stay inside the volume
    p = np.stack([rng.uniform(2.5 / X, (X - 3.5) / X, 200), rng.uniform(2.5 / Y, (Y - 3.5) / Y, 200),
                  rng.uniform(2.5 / Z, (Z - 3.5) / Z, 200)], -1)
    g = lattice_gradient(vol, p)
    assert np.allclose(g, np.array([3, 5, 7]) / 255.0, atol=1e-12)
    gd = np.tile(np.array([0.0, 0.0, 1.0]), (200, 1))
    c, m = shade(np.full((200, 3), 0.5), g, (X, Y, Z), gd, 0.1, 0.9, 0.0, 1.0, (0, 0, 0), 0.0)
    n = np.array([3 * X, 5 * Y, 7 * Z], float)
    n /= np.linalg.norm(n)
    assert np.allclose(c, 0.5 * (0.1 + 0.9 * abs(n[2])), atol=1e-12)


def test_edge_clamp_halves_the_difference():
    X = 16
    vol = np.broadcast_to((10 * np.arange(X)).astype(np.uint8), (6, 6, X)).copy()
    # a sample exactly on voxel 0's centre and on the last voxel's: one-sided difference over two voxels
    for xc, want in ((0, 10 / 510), (X - 1, 10 / 510), (5, 20 / 510)):
        p = np.array([[(xc + 0.5) / X, 0.5, 0.5]])
        assert np.allclose(lattice_gradient(vol, p)[0], [want, 0, 0], atol=1e-12), xc
    # half a voxel outside the first centre: the clamped corner x0 - 1 = -1 reads v(0) - v(0)
    p = np.array([[0.1 / X, 0.5, 0.5]])
    fx = 0.1 - 0.5 + 1.0
    assert np.allclose(lattice_gradient(vol, p)[0, 0], fx * 10 / 510, atol=1e-12)


def test_ambient_only_is_the_transfer_function_compositor():
    rng = np.random.default_rng(5)
    vol = rng.integers(0, 256, (14, 12, 16), dtype=np.uint8)
    lut = rng.uniform(0, 1, (256, 4)).astype(np.float32)
    lut[:, 3] *= 0.3
    pos, front = (0.6, 0.4, -0.9), (-0.5, -0.3, 1.0)
    cov, vuv, g = rays(pos, front, (0, 1, 0), 50.0, 40, 30)
    step = (1 / 32, 1 / 24, 1 / 28)
    for light in ((0, 0, 0), (1, -2, 0.5)):
        got = march_shaded(vol, cov, vuv, g, step, lut, (1.0, 0.0, 0.0, 8.0, light, 0.0), 1 / 20, (0.2, 0.3, 0.4))[0]
        want = march_tf(vol, cov, vuv, g, step, lut, 1 / 20, (0.2, 0.3, 0.4))[0]
        assert np.allclose(got, want, atol=1e-12)


def test_head_light_along_the_gradient_is_ka_plus_kd_plus_ks():
    e = np.array([[0.2, 0.5, 0.9]])
    g = np.array([[0.0, 0.0, -0.1]])
    gd = np.array([[0.0, 0.0, 1.0]])
    c, m = shade(e, g, (8, 8, 8), gd, 0.2, 0.5, 0.3, 16.0, (0, 0, 0), 1 / 255)
    assert np.allclose(c, np.minimum(1.0, e * 0.7 + 0.3)) and np.isclose(m[0], 0.1)
    # below grad_min: unlit
    c, _ = shade(e, g * 0.01, (8, 8, 8), gd, 0.2, 0.5, 0.3, 16.0, (0, 0, 0), 1 / 255)
    assert np.array_equal(c, e)
    # the light exactly opposite the view: no specular term
    c, _ = shade(e, g, (8, 8, 8), gd, 0.0, 0.0, 1.0, 0.0, (0, 0, 1), 0.0)
    assert np.array_equal(c, np.zeros_like(e))


# ---- vr_lod_select in shaded mode ------------------------------------------------------------------------------------
def _rule_grow(cam, P, brick_dims, ijk, grid, otd, mtd, tol, voxels):
    """include/vrhip.h, vr_lod_select, with the box grown by `voxels` voxels (composite and shaded modes)."""
    F = np.float32
    from test_lod_select import _cross, _norm
    bd, g = np.array(brick_dims, np.float64), np.array(grid, np.float64)
    G = np.array([P.global_dims[k] if P.global_dims[k] > 0 else g[k] * bd[k] for k in range(3)], np.float64)
    vs = 1.0 / G
    step = max(abs(float(F(P.step_size[k]))) for k in range(3))
    grow = voxels * vs
    f = _norm(np.array(cam.front[:], F))
    s = _norm(_cross(f, np.array(cam.up[:], F)))
    u = _cross(s, f)
    tanYf = F(math.tan(float(F(0.5) * F(F(cam.fov_deg) * F(0.01745329251994329576923690768489)))))
    tanY, tanX = float(tanYf), float(F(tanYf * F(P.width) / F(P.height)))
    f, s, u = f.astype(np.float64), s.astype(np.float64), u.astype(np.float64)
    pos = np.array(cam.pos[:], F).astype(np.float64)
    zn, zf = float(F(cam.z_near)), float(F(cam.z_far)) + (max(P.max_samples, 0) + 1.0) * step
    out = []
    for ijk_b in np.asarray(ijk, np.int64).reshape(-1, 3):
        lo = ijk_b * bd * vs - grow - 0.5
        hi = (ijk_b + 1) * bd * vs + grow - 0.5
        bmin, bmax = np.array(P.box_min[:], F).astype(np.float64), np.array(P.box_max[:], F).astype(np.float64)
        culled = bool(np.any(hi + 0.5 < bmin) or np.any(lo + 0.5 >= bmax))
        corners = np.array([[hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]] for c in range(8)])
        d = corners - pos
        z, x, y = d @ f, d @ s, d @ u
        t = 1e-6 * (1.0 + np.abs(z))
        culled = culled or bool(np.all(z < zn - t) or np.all(z > zf + t))
        if np.any(s != 0):
            culled = culled or bool(np.all(x > tanX * z + t) or np.all(-x > tanX * z + t)
                                    or np.all(y > tanY * z + t) or np.all(-y > tanY * z + t))
        if culled:
            out.append(-1)
            continue
        e = np.maximum(np.maximum(lo - pos, 0.0), pos - hi)
        sz = (P.height / 2.0 / tanY) * vs.max() / max(math.sqrt(float(e @ e)), zn)
        k = 0 if sz >= tol else int(min(otd, math.floor(3.0 * math.log2(tol / sz))))
        out.append(mtd if k == 0 else otd - k)
    return np.array(out, np.int32)


@pytest.mark.parametrize("grid,bd", [((3, 2, 5), (64, 32, 16)), ((8, 8, 15), (256, 256, 128)), ((1, 4, 2), (96, 80, 40)),
                                     ((6, 5, 4), (8, 8, 8))])
def test_select_shaded_grows_by_two_voxels(grid, bd):
    from volumerenderer_amd import _lib
    from volumerenderer_amd.render import default_params, select_lod
    rng = np.random.default_rng(99 + sum(grid))
    ijk = _grid_ijk(grid)
    otd = int(round(math.log2(bd[0] * bd[1] * bd[2])))
    mtd = otd + 7
    differs = 0
    for trial in range(40):
        where = trial % 3
        pos = rng.uniform(-0.45, 0.45, 3) if where == 0 else rng.uniform(-2.0, 2.0, 3)
        if where == 2:
            pos = np.array([0.0, 0.0, 1.5]) + rng.uniform(-0.3, 0.3, 3)
        front = rng.normal(size=3)
        if where == 2:
            front[2] = abs(front[2]) + 0.5
        W, H = int(rng.integers(64, 1921)), int(rng.integers(64, 1081))
        cam = _cam(tuple(pos), tuple(front / np.linalg.norm(front)), fov=float(rng.uniform(10, 90)),
                   near=float(rng.uniform(0.01, 0.3)), far=float(rng.uniform(0.5, 100)))
        tol = float(rng.choice([0.25, 1.0, 4.0, 16.0]))
        P = default_params(W, H, bd, _lib.RENDER_SHADED)
        if trial % 4 == 3:      # a clip box: bricks just outside it are kept for their gradient taps
            P.box_min[:] = tuple(rng.uniform(0.0, 0.5, 3))
            P.box_max[:] = tuple(rng.uniform(0.5, 1.0, 3))
        got = select_lod(cam, P, bd, ijk, grid, otd, mtd, tol)
        assert np.array_equal(got, _rule_grow(cam, P, bd, ijk, grid, otd, mtd, tol, 2.0)), trial
        Pc = default_params(W, H, bd, _lib.RENDER_COMPOSITE)
        Pc.box_min[:], Pc.box_max[:] = tuple(P.box_min), tuple(P.box_max)
        comp = select_lod(cam, Pc, bd, ijk, grid, otd, mtd, tol)
        assert np.array_equal(comp, rule(cam, Pc, bd, ijk, grid, otd, mtd, tol))
        assert not np.any((comp >= 0) & (got < 0)), trial          # never culls what composite keeps
        differs += int(np.any(comp != got))
    assert differs > 0          # the wider grow changed some decision
