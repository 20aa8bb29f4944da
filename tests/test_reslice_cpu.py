"""Slice views (vr_reslice, vr_reslice_partial; the rule is in include/vrhip.h) without a GPU: the C struct and symbols,
the argument checks of the entry points (VR_ERR_INVALID before VR_ERR_NO_DEVICE), the Python wrappers' ValueErrors, the
float32 reference of tests/refslice.py against a float64 evaluation of the same positions, distributed.slab_plane, and
examples/slice.cpp."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refslice as RS  # noqa: E402

VR_ERR_INVALID, VR_ERR_NO_DEVICE = -1, -2
NEW_SYMBOLS = ("vr_reslice", "vr_reslice_partial")
TOL = 2e-3                          # the project's frame tolerance


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


# ---- the scene test_gpu_reslice.py shares ----------------------------------------------------------------------------
SCENE_DIMS = (28, 20, 24)           # x, y, z


def scene_volume():
    """The 28 x 20 x 24 random volume of the transfer-function tests (camera 0's), [Z][Y][X]."""
    vol = np.random.default_rng(17).integers(0, 256, (24, 20, 28), dtype=np.uint8)
    vol[8:16] //= 8
    return vol


# (centre, right, down, extent across the frame's width in texture space, layer pitch); the third sticks out of the cube
OBLIQUE = [((0.5, 0.5, 0.5), (1.0, 0.2, 0.1), (0.1, 1.0, -0.3), 0.62, 0.013),
           ((0.45, 0.55, 0.5), (0.3, 0.1, 1.0), (1.0, -0.6, 0.2), 0.55, 0.021),
           ((0.8, 0.7, 0.3), (1.0, 1.0, 0.2), (-0.3, 0.5, 1.0), 0.9, 0.017)]


def oblique_plane(which, width, height, layers, filter):
    from volumerenderer_amd.render import SlicePlane
    center, right, down, extent, lp = OBLIQUE[which]
    return SlicePlane.from_frame(center, right, down, width, height, extent / width, layers, lp, filter)


# ---- the ABI -----------------------------------------------------------------------------------------------------------
def test_struct_layout_and_constants():
    from volumerenderer_amd import _lib
    T = _lib.SlicePlaneDesc
    assert C.sizeof(T) == 136
    assert (T.width.offset, T.height.offset, T.layers.offset, T.filter.offset, T.origin.offset, T.du.offset, T.dv.offset,
            T.dw.offset, T.box_min.offset, T.box_max.offset, T.global_dims.offset, T.vol_origin.offset) == \
        (0, 4, 8, 12, 16, 28, 40, 52, 64, 76, 88, 112)
    assert (_lib.SLICE_NEAREST, _lib.SLICE_LINEAR) == (0, 1)
    header = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    assert "VR_SLICE_NEAREST = 0, VR_SLICE_LINEAR = 1" in header and "} vr_slice_plane;" in header


def test_symbols_exported_and_declared(L):
    from volumerenderer_amd import _lib
    header = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name) and name in _lib.SIGNATURES and ("vr_status %s(" % name) in header, name


def _plane(**kw):
    from volumerenderer_amd import _lib
    p = _lib.SlicePlaneDesc()
    p.width, p.height, p.layers, p.filter = 8, 8, 1, 1
    p.origin[:] = (0.0625, 0.0625, 0.5)
    p.du[:], p.dv[:], p.dw[:] = (0.125, 0.0, 0.0), (0.0, 0.125, 0.0), (0.0, 0.0, 0.125)
    p.box_min[:], p.box_max[:] = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    for k, v in kw.items():
        if isinstance(v, tuple):
            getattr(p, k)[:] = v
        else:
            setattr(p, k, v)
    return p


def _bad_planes():
    """Every way a vr_slice_plane can be wrong for every call, one at a time."""
    inf, nan = math.inf, math.nan
    bad = [_plane(width=0), _plane(width=-3), _plane(height=0), _plane(layers=0), _plane(layers=-1),
           _plane(layers=(1 << 24) + 1), _plane(filter=-1), _plane(filter=2)]
    for field in ("origin", "du", "dv", "dw", "box_min", "box_max"):
        for k in range(3):
            for v in (nan, inf, -inf):
                t = list(getattr(_plane(), field))
                t[k] = v
                bad.append(_plane(**{field: tuple(t)}))
    return bad


@pytest.mark.parametrize("partial", [False, True])
def test_reslice_rejects_bad_arguments_before_the_device(L, partial):
    from test_projection_cpu import _bad_projections, _proj
    from test_transfer_function_cpu import _Bufs
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)          # B.vol: 4 x 4 x 4 voxels, B.img: 8 x 8 pixels
    I64 = C.c_int64 * 3
    fd = L.vr_reslice_partial if partial else L.vr_reslice
    try:
        def ref(x):
            return None if x is None else C.byref(x)

        def dense(**kw):
            a = dict(vol=B.vol, dims=I64(4, 4, 4), pl=_plane(), pj=_proj(), img=B.img)
            a.update(kw)
            return fd(a["vol"], a["dims"], ref(a["pl"]), ref(a["pj"]), a["img"], None)

        for k in ("vol", "dims", "pl", "pj", "img"):
            assert dense(**{k: None}) == VR_ERR_INVALID, k
        shared = [{"pl": p} for p in _bad_planes()] + [{"pj": p} for p in _bad_projections(B)]
        for k, kw in enumerate(shared):
            assert dense(**kw) == VR_ERR_INVALID, (k, sorted(kw))
        for d in ((0, 4, 4), (4, -1, 4), (4, 4, 1 << 31)):
            assert dense(dims=I64(*d)) == VR_ERR_INVALID, d
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback
            for op in (0, 1, 2):
                for flt in (0, 1):
                    assert dense(pj=_proj(op=op), pl=_plane(filter=flt)) == VR_ERR_NO_DEVICE
            assert dense(pj=_proj(lut=B.lut, lo=0.1, hi=0.9, bg=(0.2, 0.4, 0.6))) == VR_ERR_NO_DEVICE
            assert dense(pl=_plane(layers=1 << 24)) == VR_ERR_NO_DEVICE
            assert dense(pl=_plane(global_dims=(4, 4, 9), vol_origin=(0, 0, 3), box_min=(0.0, 0.0, 0.4), box_max=(1.0, 1.0, 2.0))) \
                == VR_ERR_NO_DEVICE
    finally:
        B.free()


# ---- Python wrappers ---------------------------------------------------------------------------------------------------
def test_slice_plane_builders_and_bad_values():
    pytest.importorskip("torch")
    import volumerenderer_amd as vr
    from volumerenderer_amd import _lib
    S = vr.SlicePlane
    ok = dict(width=4, height=3, origin=(0.1, 0.2, 0.3), du=(0.1, 0.0, 0.0), dv=(0.0, 0.1, 0.0))
    for kw in ({"width": 0}, {"height": -1}, {"width": 2.5}, {"layers": 0}, {"layers": (1 << 24) + 1}, {"filter": "cubic"},
               {"filter": 2}, {"filter": None}, {"origin": (0.0, math.nan, 0.0)}, {"du": (math.inf, 0.0, 0.0)},
               {"dv": (0.0, 0.0)}, {"dw": 1.0}, {"box_min": (0.0, 0.0, -math.inf)}, {"box_max": (1e39, 1.0, 1.0)},
               {"global_dims": (4, 4)}, {"vol_origin": (0, -1, 0)}):
        with pytest.raises(ValueError):
            S(**dict(ok, **kw))
    d = S(layers=3, filter="nearest", dw=(0.0, 0.0, 0.25), **ok).desc()
    assert (d.width, d.height, d.layers, d.filter) == (4, 3, 3, _lib.SLICE_NEAREST)
    assert tuple(d.box_min) == (0.0, 0.0, 0.0) and tuple(d.box_max) == (1.0, 1.0, 1.0)
    assert tuple(d.global_dims) == (0, 0, 0) and tuple(d.vol_origin) == (0, 0, 0)
    assert [S(filter=f, **ok).filter for f in ("nearest", "linear", 0, 1)] == [0, 1, 0, 1]
    # axis_aligned: pixel centres on voxel centres, the image axes per orientation
    dims = (8, 4, 16)
    for axis, (cu, cv) in ((0, (1, 2)), (1, (0, 2)), (2, (0, 1))):
        p = S.axis_aligned(dims, axis, 3, layers=2, filter="nearest")
        assert (p.width, p.height, p.layers) == (dims[cu], dims[cv], 2)
        pos = RS.positions(p, 1)
        want = {cu: (np.arange(dims[cu])[None, :] + 0.5) / dims[cu], cv: (np.arange(dims[cv])[:, None] + 0.5) / dims[cv],
                axis: np.full((1, 1), 4.5 / dims[axis])}
        for k in range(3):
            assert np.array_equal(pos[k], np.broadcast_to(want[k], pos[k].shape).astype(np.float32)), (axis, k)
    p = S.axis_aligned(dims, 2, 0, pixels_per_voxel=0.5)
    assert (p.width, p.height) == (4, 2) and p.du[0] == 0.25 and p.origin[0] == 0.125
    for a in ((dims, 3, 0), (dims, 2, 16), (dims, 2, -1), ((8, 0, 16), 2, 0)):
        with pytest.raises(ValueError):
            S.axis_aligned(*a)
    with pytest.raises(ValueError):
        S.axis_aligned(dims, 2, 0, pixels_per_voxel=0)
    # from_frame: the centre pixel of an odd frame and layer stack is the centre
    p = S.from_frame((0.4, 0.5, 0.6), (2.0, 0.0, 0.0), (0.0, 0.0, -3.0), 5, 3, 0.1, 3, 0.05)
    assert np.allclose(RS.positions(p, 1)[:, 1, 2], (0.4, 0.5, 0.6), atol=1e-7)
    assert np.allclose(p.du, (0.1, 0, 0)) and np.allclose(p.dv, (0, 0, -0.1)) and np.allclose(p.dw, (0, 0.05, 0))
    for a in (((0, 0, 0), (0, 0, 0), (0, 1, 0)), ((0, 0, 0), (1, 0, 0), (2, 0, 0))):
        with pytest.raises(ValueError):
            S.from_frame(*a, 4, 4, 0.1)
    with pytest.raises(ValueError):
        S.from_frame((0, 0, 0), (1, 0, 0), (0, 1, 0), 4, 4, 0.0)


def test_python_wrappers_raise_before_any_c_call():
    torch = pytest.importorskip("torch")
    import volumerenderer_amd as vr
    from volumerenderer_amd import render as R
    for name in ("SlicePlane", "reslice", "reslice_partial"):
        assert callable(getattr(vr, name)), name
    plane = R.SlicePlane.axis_aligned((4, 4, 4), 2, 1)
    with pytest.raises(ValueError):
        R._check_plane(None)
    with pytest.raises(ValueError):
        R._slice_out(torch.zeros((4, 4, 3)), plane, torch.device("cpu"))            # not width * height * 4 floats
    with pytest.raises(ValueError):
        R._check_plane(plane.desc())                                                # a ctypes struct is not a SlicePlane


def test_slab_plane_is_slab_params_twin():
    pytest.importorskip("torch")
    from volumerenderer_amd import distributed as D
    from volumerenderer_amd import render as R
    dims = (29, 23, 31)
    plane = R.SlicePlane.axis_aligned(dims, 1, 4, layers=3)
    for axis in (0, 1, 2):
        for world in (2, 3, 5):
            for halo in (0, 1):
                for r in range(world):
                    p, local, span = D.slab_plane(plane, dims, axis, r, world, halo)
                    P, local0, span0 = D.slab_params(R.default_params(8, 8, dims), dims, axis, r, world, halo)
                    assert local == local0 and span == span0
                    dp = p.desc()
                    assert tuple(dp.box_min) == tuple(P.box_min) and tuple(dp.box_max) == tuple(P.box_max)
                    assert tuple(dp.global_dims) == tuple(P.global_dims) and tuple(dp.vol_origin) == tuple(P.vol_origin)
                    assert (p.origin, p.du, p.dv, p.dw, p.layers) == (plane.origin, plane.du, plane.dv, plane.dw, 3)
    assert plane.box_max == (1.0, 1.0, 1.0) and plane.global_dims == (0, 0, 0)     # the original is left alone
    with pytest.raises(ValueError):
        D.slab_plane(plane, dims, 3, 0, 2, 1)
    with pytest.raises(ValueError):
        D.slab_plane(plane, dims, 0, 2, 2, 1)


# ---- the float32 reference against float64 -----------------------------------------------------------------------------
@pytest.mark.parametrize("which", [0, 1, 2])
def test_float32_reference_is_within_the_frame_tolerance_of_float64(which):
    """The same float32 positions (and so the same taken samples) evaluated in double: the fetch, the reductions and the
    finish.  2e-3 is the project's frame tolerance; the measured maximum is printed."""
    pytest.importorskip("torch")
    from test_gpu_transfer_function import smooth_table
    from volumerenderer_amd.render import transfer_function_table
    vol = scene_volume()
    lut = transfer_function_table(smooth_table(np.random.default_rng(5)))
    worst = 0.0
    for layers in (1, 7):
        for flt in (RS.NEAREST, RS.LINEAR):
            plane = oblique_plane(which, 72, 54, layers, flt)
            for op in RS.OPS:
                p32, p64 = RS.partial(vol, plane, op), RS.partial(vol, plane, op, np.float64)
                assert p32.dtype == np.float32 and np.array_equal(p32[..., 1], p64[..., 1])
                assert (p32[..., 1] > 0).any() and ((p32[..., 1] == 0).any() == (which == 2))
                scale = np.maximum(p64[..., 1], 1) if op == RS.MEAN else 1.0
                d = float(np.abs((p32[..., 0] - p64[..., 0]) / scale).max())
                for window, table in (((0.0, 1.0), None), ((0.1, 0.9), lut)):
                    f32 = RS.finish(p32, op, window, (0.2, 0.4, 0.6), table)
                    f64 = RS.finish(p64, op, window, (0.2, 0.4, 0.6), table, np.float64)
                    assert f32.dtype == np.float32
                    d = max(d, float(np.abs(f32 - f64).max()))
                worst = max(worst, d)
                assert d <= TOL, (which, layers, flt, op, d)
    print("plane", which, "float32 against float64: max", worst)


# ---- the C++ surface ---------------------------------------------------------------------------------------------------
def compile_example(out_dir):
    """examples/slice.cpp (vrhip::Slicer) built with g++ against libvrhip.so; returns the program's path."""
    import __graft_entry__ as g
    g.build()
    exe = os.path.join(str(out_dir), "slice")
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-std=c++14", "-O2", "-Wall", "-Werror", "-pthread", "-I" + os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "examples", "slice.cpp"), "-L" + lib, "-lvrhip", "-Wl,-rpath," + lib,
                           "-o", exe])
    return exe


def test_cpp_example_compiles_and_is_loud_without_a_gpu(L, tmp_path):
    exe = compile_example(tmp_path)
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    r = subprocess.run([exe], capture_output=True, text=True)
    if n.value > 0:
        assert r.returncode == 0 and r.stdout.count("fnv1a64") == 2, r.stdout + r.stderr
    else:
        assert r.returncode != 0 and "no usable HIP device" in (r.stdout + r.stderr)
