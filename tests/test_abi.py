"""CPU tests of the drop-in boundary: the C-ABI library loads, exports every symbol
include/vrhip.h declares, and refuses to compute without a GPU (no CPU fallback)."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    return _lib.lib()


def test_header_symbols_all_exported(L):
    from volumerenderer_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    declared = set(re.findall(r"\b(vr_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    for name in declared:
        assert hasattr(L, name), "libvrhip.so does not export %s" % name
    # and the binding covers exactly the header
    assert declared == set(_lib.SIGNATURES), declared ^ set(_lib.SIGNATURES)


def test_struct_layouts_match_header():
    from volumerenderer_amd import _lib
    assert C.sizeof(_lib.TreeInfo) == 88
    assert C.sizeof(_lib.Camera) == 48
    assert C.sizeof(_lib.RenderParams) == 32 + 24 + 48 + 8 + 8


def test_header_limits():
    """The limits a caller may build on: VR_MAX_BRICKS is the largest brick count every batched launch accepts (the brick
    index is the grid's second axis, of which an MI355X allows 65536)."""
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    limits = {k: int(v) for k, v in re.findall(r"#define\s+(VR_MAX_\w+|VR_POOL_STAGE_BRICKS)\s+(\d+)", hdr)}
    assert limits["VR_MAX_BRICKS"] == 65535
    assert limits["VR_MAX_EPOCHS"] == 1024
    assert limits["VR_POOL_STAGE_BRICKS"] == 32


def test_status_strings(L):
    assert L.vr_status_string(0) == b"ok"
    assert b"no CPU fallback" in L.vr_status_string(-2)
    assert L.vr_version().startswith(b"vrhip")


def test_argument_validation_and_no_cpu_fallback(L):
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    h = C.c_void_p()
    dims = (C.c_int64 * 3)(16, 16, 16)
    bad = (C.c_int64 * 3)(1 << 21, 16, 16)       # an axis beyond 2^20 (or 2^31 voxels and more): unsupported
    assert L.vr_brickset_create(None, 1, dims, 1, 2, 0) == -1           # VR_ERR_INVALID
    assert L.vr_brickset_create(C.byref(h), 1, dims, -1, 2, 0) == -1    # negative tolerance
    assert L.vr_brickset_create(C.byref(h), 1, bad, 1, 2, 0) == -7      # VR_ERR_UNSUPPORTED
    assert L.vr_brickset_create(C.byref(h), 65536, dims, 1, 2, 0) == -7 and not h   # more than VR_MAX_BRICKS bricks
    # vr_compositor_create_with_transport: argument checks first, whatever the device
    noop = C.CFUNCTYPE(C.c_int32, C.c_void_p)(lambda ctx: 0)
    xfer = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p)(lambda *a: 0)
    table = (C.c_void_p * 4)(*[C.cast(f, C.c_void_p) for f in (noop, noop, xfer, xfer)])
    for k in range(4):                                                   # one null member at a time
        holed = (C.c_void_p * 4)(*table)
        holed[k] = None
        assert L.vr_compositor_create_with_transport(C.byref(h), holed, None, 0, 2, 64, 48) == -1
    assert L.vr_compositor_create_with_transport(C.byref(h), None, None, 0, 2, 64, 48) == -1     # no table
    assert L.vr_compositor_create_with_transport(None, table, None, 0, 2, 64, 48) == -1
    for rank, world, w, hh in ((0, 0, 64, 48), (2, 2, 64, 48), (-1, 2, 64, 48), (0, 5, 64, 4), (0, 2, 0, 48)):
        assert L.vr_compositor_create_with_transport(C.byref(h), table, None, rank, world, w, hh) == -1, (rank, world, w, hh)
    # vr_raycast: extents checked before the device (tex3d would clamp to -1 and read before the volume; >= 2^31 would
    # be narrowed to int), as vr_skip_grid_build does
    from volumerenderer_amd import render as R
    cam, P = R.default_camera(), R.default_params(8, 8, (16, 16, 16))
    vol = (C.c_uint8 * 64)()
    img = (C.c_float * (8 * 8 * 4))()
    for d in ((0, 16, 16), (16, -1, 16), (16, 16, -(1 << 40)), (1 << 31, 1, 1), (1, 1 << 31, 1), (1, 1, 1 << 40), (-1, -1, 1)):
        assert L.vr_raycast(vol, (C.c_int64 * 3)(*d), C.byref(cam), C.byref(P), img, None) == -1, d
        assert L.vr_skip_grid_build(vol, (C.c_int64 * 3)(*d), 8, vol, None) == -1, d
    if n.value == 0:
        # CPU-only box: every compute entry point must fail loudly
        assert L.vr_raycast(vol, (C.c_int64 * 3)(4, 4, 4), C.byref(cam), C.byref(P), img, None) == -2
        assert L.vr_raycast(vol, (C.c_int64 * 3)(1, 1, 1), C.byref(cam), C.byref(P), img, None) == -2
        assert L.vr_brickset_create(C.byref(h), 1, dims, 1, 2, 0) == -2  # VR_ERR_NO_DEVICE
        assert L.vr_set_device(0) == -2
        buf = (C.c_uint8 * 16)()
        assert L.vr_query_error(buf, buf, 16, buf, None) == -2
        assert L.vr_measure_error(buf, buf, 16, None, None, None) == -2
        assert L.vr_composite_over(buf, buf, 1, None) == -2
        assert L.vr_compositor_create_with_transport(C.byref(h), table, None, 0, 2, 64, 48) == -2
        assert L.vr_compositor_create_with_transport(C.byref(h), table, None, 0, 1, 64, 1) == -2


# the six ray-casting entry points: (source, style)
RAYCAST_ENTRIES = {"vr_raycast": ("dense", "grey"), "vr_raycast_pool": ("pool", "grey"),
                   "vr_raycast_tf": ("dense", "table"), "vr_raycast_pool_tf": ("pool", "table"),
                   "vr_raycast_tf_shaded": ("dense", "lit"), "vr_raycast_pool_tf_shaded": ("pool", "lit")}


@pytest.mark.parametrize("entry", sorted(RAYCAST_ENTRIES))
def test_raycast_entries_reject_bad_arguments_before_the_device(L, entry):
    """Every ray-casting entry point faces the bad inputs of its source kind (dense volume or pool) and its style
    (greyscale, table, lit): each pointer null in turn, the frame, the extents, the mode, the table and the lighting."""
    import math
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_transfer_function_cpu import _Bufs
    from volumerenderer_amd import _lib
    from volumerenderer_amd import render as R
    source, style = RAYCAST_ENTRIES[entry]
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    B = _Bufs(L, n.value)
    I64 = C.c_int64 * 3
    fn = getattr(L, entry)
    valid_mode = _lib.RENDER_SHADED if style == "lit" else _lib.RENDER_COMPOSITE

    def params(**kw):
        P = R.default_params(8, 8, (4, 4, 4), valid_mode)
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(P, k)[:] = v
            else:
                setattr(P, k, v)
        return P

    def tf(lut=B.lut, unit=0.0, bg=(1.0, 1.0, 1.0)):
        t = _lib.TransferFunctionDesc()
        t.lut_dev, t.opacity_unit = lut, unit
        t.background[:] = bg
        return t

    def sh(**kw):
        s = R.Shading().desc()
        for k, v in kw.items():
            if k == "light_dir":
                s.light_dir[:] = v
            else:
                setattr(s, k, v)
        return s

    def call(**kw):
        a = dict(vol=B.vol, dims=I64(4, 4, 4), pool=B.vol, table=B.table, bd=I64(4, 4, 4), grid=I64(1, 1, 1),
                 cam=R.default_camera(), P=params(), tf=tf(), sh=sh(), rgba=B.img)
        a.update(kw)
        ref = [None if a[k] is None else C.byref(a[k]) for k in ("cam", "P", "tf", "sh")]
        cam, P, t, s = ref
        if source == "dense":
            head = [a["vol"], a["dims"]]
        else:
            head = [a["pool"], a["table"], a["bd"], a["grid"]]
        tail = {"grey": [], "table": [t], "lit": [t, s]}[style]
        return fn(*head, cam, P, *tail, a["rgba"], None)

    try:
        bad = []
        # every pointer argument null in turn
        ptrs = ["vol", "dims"] if source == "dense" else ["pool", "table", "bd", "grid"]
        ptrs += ["cam", "P", "rgba"] + {"grey": [], "table": ["tf"], "lit": ["tf", "sh"]}[style]
        bad += [{p: None} for p in ptrs]
        # the frame
        bad += [{"P": params(width=0)}, {"P": params(width=-8)}, {"P": params(height=0)}, {"P": params(height=-1)},
                {"P": params(max_samples=-1)}]
        if source == "dense":
            for d in ((0, 16, 16), (16, -1, 16), (16, 16, -(1 << 40)), (1 << 31, 1, 1), (1, 1 << 31, 1), (1, 1, 1 << 40),
                      (-1, -1, 1)):
                bad.append({"dims": I64(*d)})
        else:
            for b in ((4, 6, 4), (0, 4, 4), (4, -4, 4), (4, 4, 3), (-(1 << 40), 4, 4)):     # not positive powers of two
                bad.append({"bd": I64(*b)})
            for g in ((0, 1, 1), (1, -1, 1), (1, 1, 0)):
                bad.append({"grid": I64(*g)})
            # a virtual extent of 2^31 voxels or more
            bad += [{"grid": I64(1 << 29, 1, 1)}, {"grid": I64(1, 1 << 40, 1)}, {"bd": I64(1 << 31, 4, 4)},
                    {"bd": I64(4, 4, 1 << 20), "grid": I64(1, 1, 1 << 11)}]
            for k in range(3):
                o = [0, 0, 0]
                o[k] = 1
                bad.append({"P": params(vol_origin=tuple(o))})
                o[k] = -1
                bad.append({"P": params(vol_origin=tuple(o))})
                gd = [4, 4, 4]
                gd[k] = 8
                bad.append({"P": params(global_dims=tuple(gd))})
                gd[k] = -4
                bad.append({"P": params(global_dims=tuple(gd))})
        # the mode of the style
        modes = {"grey": (-1, 3, 4), "table": (-1, 1, 2, 3, 4), "lit": (-1, 0, 1, 2, 4)}[style]
        bad += [{"P": params(mode=m)} for m in modes]
        if style != "grey":
            bad += [{"tf": t} for t in (tf(lut=None), tf(lut=B.lut + 4), tf(lut=B.lut + 8), tf(unit=-1e-6),
                                        tf(unit=math.inf), tf(unit=math.nan), tf(bg=(1.0, math.nan, 1.0)),
                                        tf(bg=(math.inf, 0.0, 0.0)), tf(bg=(0.0, 0.0, -math.inf)))]
        if style == "lit":
            for f in ("ambient", "diffuse", "specular", "shininess", "grad_min"):
                bad += [{"sh": sh(**{f: v})} for v in (-1e-6, math.nan, math.inf)]
            bad += [{"sh": sh(light_dir=(0.0, math.nan, 1.0))}, {"sh": sh(light_dir=(math.inf, 0.0, 0.0))}]
        for k, kw in enumerate(bad):
            assert call(**kw) == -1, (entry, k, sorted(kw))
        if n.value == 0:
            # valid arguments reach the device check: no CPU fallback
            assert call() == -2
            if source == "pool":
                assert call(P=params(global_dims=(4, 4, 4))) == -2
            if style == "lit":
                assert call(sh=sh(light_dir=(-1.0, -2.0, 0.5), ambient=0.0, shininess=0.0, grad_min=0.0)) == -2
    finally:
        B.free()


def test_product_never_imports_oracle():
    """The oracle and the reference builds beside it (oracle/_ref/libvkref.so, the codec; oracle/_ref/libvkfrag.so, the
    fragment shaders) are test infrastructure: nothing under volumerenderer_amd/ or include/ may reference any of them."""
    for base in ("volumerenderer_amd", "include"):
        for dp, _, fs in os.walk(os.path.join(ROOT, base)):
            for f in fs:
                if f.endswith((".py", ".h", ".hpp", ".hip", ".cpp")):
                    txt = open(os.path.join(dp, f), errors="ignore").read()
                    for needle in ("import oracle", "from oracle", "liboracle", "oracle/", "_ref/", "libvkref", "vkref_",
                                   "RefTree", "ref_lib", "libvkfrag", "vkfrag_", "RefShader", "frag_lib"):
                        assert needle not in txt, "%s references the oracle (%s)" % (f, needle)


def test_loopback_transport_compiles(tmp_path):
    """The loopback vr_transport the GPU compositor tests run the exchange with is plain C++ on the HIP runtime API:
    it builds with g++ and -Werror here too, and exports what those tests call."""
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_compositor import build_loopback
    so = build_loopback(tmp_path)
    lb = C.CDLL(so)
    for name in ("lb_create", "lb_destroy", "lb_rank_ctx", "lb_transport", "lb_fail_at", "lb_count_delta", "lb_log_size",
                 "lb_log_entry", "lb_log_clear", "lb_errors"):
        assert hasattr(lb, name), name
    src = open(os.path.join(ROOT, "tests", "loopback_transport.cpp")).read()
    code = "\n".join(line.split("//")[0] for line in src.splitlines())
    for sync in ("hipStreamSynchronize", "hipDeviceSynchronize", "hipEventSynchronize", "hipStreamQuery", "hipMemcpy("):
        assert sync not in code, "the fake must not synchronise (%s)" % sync

