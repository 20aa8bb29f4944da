"""The edge cases of the slice views (vr_reslice, vr_reslice_partial) and an independent float64 reference, shared by
test_slice_edge_cases_cpu.py (the references held to each other) and test_gpu_slice_edges.py (the kernel held to both).
Data and small builders only: nothing here needs a GPU.

ref64 is written from the rule in include/vrhip.h, not from refslice.py: the positions are formed in double from the
plane's float32 fields, the taken test, the NEAREST voxel and LINEAR's eight-tap weighted sum are in double.  What the
two may decide differently is bounded per pixel by a SLACK (see ref64); a pixel with slack > 1 is decided.

A case is a dict:
  name, family, exact (every product and sum of its positions is exact in float32: nothing is masked), vol (the
  [Z][Y][X] volume the call is handed), geo (the keywords of render.SlicePlane but the filter), hits (what the case must
  reach: test_slice_edge_cases_cpu.py asserts each), round32 (deep stacks only: see ref64), slabs (exact slabs only:
  [(geo, local volume)] per rank) and, for the faces and the rim, column = (axis, index): every sample's voxel has that
  index along that axis.  What a family knows without a reference rides along: owns (faces, rim), still ("pixels" or
  "layers") and count (deep stacks); check_known reads them."""
import collections
import functools

import numpy as np

from test_reslice_cpu import OBLIQUE, SCENE_DIMS, TOL, scene_volume  # noqa: F401  (TOL: no new number)

NEAREST, LINEAR = 0, 1
MAX, MIN, MEAN = 0, 1, 2
OPS = (MAX, MIN, MEAN)
OP_NAMES = ("max", "min", "mean")
FILTER_NAMES = ("nearest", "linear")
CAP = 0.05                          # a general-family frame masks at most this share of its pixels; an exact one none
U = 2.0 ** -24                      # the unit roundoff of float32
F32_MAX = float(np.finfo(np.float32).max)
F32_OVER = F32_MAX + 2.0 ** 103     # a product or sum of this magnitude rounds to inf in float32
TINY = float(np.float32(2.0 ** -149))               # the smallest positive float32
BELOW_ONE = float(np.nextafter(np.float32(1), np.float32(0)))

# the planes of the general families: test_reslice_cpu.OBLIQUE and the body diagonal, which leaves the cube at every corner
PLANES = OBLIQUE + [((0.5, 0.5, 0.5), (1.0, 1.0, 1.0), (1.0, -1.0, 0.0), 1.9, 0.019)]
VOLUME_DIMS = [(1, 1, 1), (7, 1, 3), (16, 8, 4), SCENE_DIMS, (1, 1, 300)]             # x, y, z

Ref = collections.namedtuple("Ref", "v n slack voxel")


def f32(v):
    return tuple(float(np.float32(q)) for q in v)


@functools.lru_cache(maxsize=None)
def volume(dims):
    """The [Z][Y][X] volume of `dims` = (x, y, z): the scene of test_reslice_cpu.py, or random bytes by the extents."""
    if tuple(dims) == tuple(SCENE_DIMS):
        vol = scene_volume()
    else:
        X, Y, Z = dims
        vol = np.random.default_rng(1000 * X + 10 * Y + Z).integers(0, 256, (Z, Y, X), dtype=np.uint8)
    vol.setflags(write=False)
    return vol


def plane_of(geo, flt):
    from volumerenderer_amd.render import SlicePlane
    return SlicePlane(filter=flt, **geo)


def plane(case, flt):
    return plane_of(case["geo"], flt)


# ---- the float64 reference ---------------------------------------------------------------------------------------------
def _vec(v):
    return np.array([float(np.float32(q)) for q in v], np.float64)


def _r32(x, round32):
    """A product or sum as float32 holds it.  Beyond the largest float32 it is +-inf -- what the header's "rounded to
    float32" means there, and inf - inf is the NaN the kernel meets.  round32: also rounded to float32 (through double,
    once: a product of two float32 is exact in double and a correctly rounded double sum rounds to float32 innocuously)."""
    with np.errstate(invalid="ignore", over="ignore"):
        x = np.where(np.abs(x) >= F32_OVER, np.copysign(np.inf, x), x)
        return x.astype(np.float32).astype(np.float64) if round32 else x


def positions64(pl, round32=False):
    """(pos, bound), both [L][3][H][W] in double: pos_k = ((origin_k + px du_k) + py dv_k) + l dw_k from the plane's float32
    fields, and the bound of the issue on the float32 rounding of pos_k: four units of 2^-24 on |origin| + |px du| + |py dv|
    + |l dw| (0 with round32: the position is then the float32 one)."""
    o, du, dv, dw = _vec(pl.origin), _vec(pl.du), _vec(pl.dv), _vec(pl.dw)
    px = np.arange(pl.width, dtype=np.float64)[None, None, None, :]
    py = np.arange(pl.height, dtype=np.float64)[None, None, :, None]
    l = np.arange(pl.layers, dtype=np.float64)[:, None, None, None]
    shape = (pl.layers, 3, pl.height, pl.width)
    c = (1, 3, 1, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        a, b, d = _r32(px * du.reshape(c), round32), _r32(py * dv.reshape(c), round32), _r32(l * dw.reshape(c), round32)
        pos = _r32(_r32(_r32(o.reshape(c) + a, round32) + b, round32) + d, round32)
        mag = np.abs(o).reshape(c) + np.abs(a) + np.abs(b) + np.abs(d)
    bound = np.zeros(shape) if round32 else np.broadcast_to(4 * U * mag, shape)
    return np.broadcast_to(pos, shape), bound


def _ratio(dist, bound):
    """dist / bound per sample; a sample on a threshold has 0, a sample with no rounding at all away from it inf, and a
    position that is not finite (never taken, whatever the precision) inf."""
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(dist > 0, dist / bound, 0.0)
    return np.where(np.isfinite(dist), r, np.inf)


def _dims_of(vol, pl):
    Z, Y, X = vol.shape
    n = (X, Y, Z)
    G = tuple(int(pl.global_dims[k]) if int(pl.global_dims[k]) > 0 else n[k] for k in range(3))
    return n, G, tuple(int(q) for q in pl.vol_origin)


def _local(idx, G, org, n):
    """A global voxel index, clamped to the global volume, then located in the local one (vrhip.h)."""
    return np.clip(np.clip(idx, 0, G - 1) - org, 0, n - 1)


@functools.lru_cache(maxsize=64)
def _ref64_ops(key):
    vol, pl, round32 = _KEYED[key]
    n, G, org = _dims_of(vol, pl)
    pos, bound = positions64(pl, round32)
    bmin, bmax = _vec(pl.box_min), _vec(pl.box_max)
    c = (1, 3, 1, 1)
    finite = np.isfinite(pos)
    p = np.clip(np.where(finite, pos, -1.0), -1.0, 2.0)   # outside is outside: -1 and 2 stand for everything beyond them
    in_cube = ((p > 0) & (p < 1)).all(1)
    taken = in_cube & ((p >= bmin.reshape(c)) & (p < bmax.reshape(c))).all(1)
    # the slack: the distance to every decision threshold over the bound on the position
    with np.errstate(invalid="ignore"):
        dist = np.minimum(np.minimum(np.abs(pos), np.abs(pos - 1)),
                          np.minimum(np.abs(pos - bmin.reshape(c)), np.abs(pos - bmax.reshape(c))))
    dist = np.where(finite, dist, np.inf)
    slack = _ratio(dist, bound).min(1)                                                  # [L][H][W]
    Gf = np.array(G, np.float64).reshape(c)
    if pl.filter == NEAREST:
        g = p * Gf
        vdist = np.abs(g - np.rint(g)) / Gf
        vslack = _ratio(np.where(in_cube[:, None], vdist, np.inf), bound + 2 * U * np.abs(p)).min(1)
        slack = np.minimum(slack, vslack)
        idx = [_local(np.floor(g[:, k]).astype(np.int64), G[k], org[k], n[k]) for k in range(3)]
        voxel = vol[idx[2], idx[1], idx[0]].astype(np.int64)
        smp = voxel / 255.0
    else:
        voxel = None
        x = p * Gf - 0.5
        x0 = np.floor(x)
        w1 = x - x0
        base = x0.astype(np.int64)
        smp = np.zeros(taken.shape)
        for tz in (0, 1):
            for ty in (0, 1):
                for tx in (0, 1):
                    t = (tx, ty, tz)
                    i = [_local(base[:, k] + t[k], G[k], org[k], n[k]) for k in range(3)]
                    w = np.ones(taken.shape)
                    for k in range(3):
                        w = w * (w1[:, k] if t[k] else 1.0 - w1[:, k])
                    smp = smp + w * (vol[i[2], i[1], i[0]] / 255.0)
    out = {}
    shape = taken.shape[1:]
    count = taken.sum(0)
    for op in OPS:
        v = np.full(shape, np.inf if op == MIN else 0.0)
        q = np.full(shape, 255 if op == MIN else 0, np.int64)
        for l in range(pl.layers):                        # ascending layer order
            if op == MEAN:
                v = np.where(taken[l], v + smp[l], v)
            else:
                v = np.where(taken[l], (np.minimum if op == MIN else np.maximum)(v, smp[l]), v)
                if voxel is not None:
                    q = np.where(taken[l], (np.minimum if op == MIN else np.maximum)(q, voxel[l]), q)
        out[op] = Ref(np.where(count > 0, v, 0.0), count, slack.min(0), q if voxel is not None and op != MEAN else None)
    return out


_KEYED = {}


def ref64(vol, pl, op, round32=False):
    """The slice in double, from the header's rule: Ref(v, n, slack, voxel), each [H][W].  n counts the taken samples, v
    is their maximum from 0, minimum from +inf or sum in ascending layer order (0 where n == 0); voxel is the largest
    (MAX) or smallest (MIN) NEAREST voxel among them, None otherwise.
    slack: the smallest distance, over the pixel's samples and the three axes, from pos_k to a decision threshold -- 0, 1,
    box_min_k, box_max_k and, for NEAREST inside the cube, the nearest voxel boundary j / G_k -- over the bound of
    positions64 (plus two units of 2^-24 on |pos| at the voxel boundary, for the product with G).  Where slack > 1 no
    float32 evaluation in the documented order can decide differently.
    round32 rounds every product and sum of the position to float32: the header's rule taken literally, for the stacks
    whose step is not dyadic and whose every pixel has samples within rounding of a threshold."""
    key = (hash(vol.tobytes()), vol.shape, pl.filter, pl.width, pl.height, pl.layers, f32(pl.origin), f32(pl.du), f32(pl.dv), f32(pl.dw),
           f32(pl.box_min), f32(pl.box_max), tuple(pl.global_dims), tuple(pl.vol_origin), bool(round32))
    _KEYED[key] = (vol, pl, bool(round32))
    return _ref64_ops(key)[op]


def decided(case, ref):
    """The pixels compared: all of an exact case, those with slack > 1 otherwise."""
    return np.ones(ref.slack.shape, bool) if case["exact"] else ref.slack > 1


def check_cap(case, ref):
    """The masked count of a frame, held to the cap (a condition, not a measurement)."""
    masked = int((~decided(case, ref)).sum())
    assert masked <= CAP * ref.slack.size, (case["name"], masked, ref.slack.size)
    return masked


# ---- transformations the GPU module applies ----------------------------------------------------------------------------
def reversed_geo(geo):
    """The same samples, the stack walked backwards: origin on the last layer, dw negated.  On the exact families the
    positions are identical."""
    g = dict(geo)
    L = geo["layers"]
    g["origin"] = tuple(float(np.float32(geo["origin"][k]) + np.float32(L - 1) * np.float32(geo["dw"][k])) for k in range(3))
    g["dw"] = tuple(-q for q in geo["dw"])
    return g


def rotated(vol, geo):
    """Volume and plane with the axes rotated x -> y -> z -> x: v' = (v_z, v_x, v_y)."""
    def r(v):
        return (v[2], v[0], v[1])
    g = dict(geo)
    for k in ("origin", "du", "dv", "dw", "box_min", "box_max", "global_dims", "vol_origin"):
        if k in g:
            g[k] = r(g[k])
    return np.ascontiguousarray(vol.transpose(1, 2, 0)), g


# ---- the cases ---------------------------------------------------------------------------------------------------------
def _geo(width, height, origin, du, dv, dw=(0.0, 0.0, 0.0), layers=1, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
    return dict(width=width, height=height, origin=f32(origin), du=f32(du), dv=f32(dv), dw=f32(dw), layers=layers,
                box_min=f32(box_min), box_max=f32(box_max))


def _case(family, name, dims, geo, exact=True, hits=(), **kw):
    c = dict(family=family, name=name, dims=tuple(dims), vol=volume(tuple(dims)), geo=geo, exact=exact, hits=tuple(hits),
             round32=False, slabs=None, column=None)
    c.update(kw)
    return c


def _axes(v, axis):
    """(normal, across, down) components placed for a slice whose normal is `axis`: the image axes of render.py."""
    cu, cv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
    out = [0.0, 0.0, 0.0]
    out[axis], out[cu], out[cv] = v
    return tuple(out)


LATTICE = dict(origin=(-1 / 8, -1 / 8, 1 / 2), du=(1 / 32, 0, 0), dv=(0, 1 / 32, 0), dw=(0, 0, 1 / 64))
BOUNDARIES = ("zero", "one", "box_min", "box_max", "voxel_boundary")
ON_VOXELS = VOLUME_DIMS[2:]         # multiples of 1 / 32 and 1 / 64 meet no voxel boundary of 1 x 1 x 1 and 7 x 1 x 3 inside the cube


@functools.lru_cache(maxsize=None)
def cases():
    cs = []
    # lattice: samples exactly on 0, 1, box_min, box_max and on voxel boundaries
    for d in VOLUME_DIMS:
        cs.append(_case("lattice", "lattice %dx%dx%d" % d, d,
                        _geo(41, 41, layers=5, box_min=(1 / 4, 0, 0), box_max=(3 / 4, 1, 17 / 32), **LATTICE),
                        hits=BOUNDARIES[:4 + (d in ON_VOXELS)]))
    # ... turned and reversed: columns along z, rows along -y, layers along -x, the whole cube as box
    for d in VOLUME_DIMS:
        cs.append(_case("turned", "turned %dx%dx%d" % d, d,
                        _geo(41, 41, (1 / 2, 9 / 8, -1 / 8), (0, 0, 1 / 32), (0, -1 / 32, 0), (-1 / 16, 0, 0), 9),
                        hits=("zero", "one") + BOUNDARIES[4:4 + (d in ON_VOXELS)]))
    # ... sheared: the layers step along x too, so a pixel's stack crosses box_min and box_max one layer at a time.  The two
    # lattices above have n in {0, 2} and {0, 8} by construction; this one takes every value from 0 to its 5 layers.  Its
    # box_max is 2 along y and z, as a last rank's is: there `pos < 1` alone keeps the samples ON 1 out (a box_max of 1
    # would hide a `<=` in the cube test).
    cs.append(_case("sheared", "sheared 16x8x4", (16, 8, 4),
                    _geo(41, 41, LATTICE["origin"], LATTICE["du"], LATTICE["dv"], (1 / 32, 0, 1 / 64), 5, (1 / 4, 0, 0), (3 / 4, 2, 2)),
                    hits=BOUNDARIES + ("every_n",)))
    # faces: a plane ON a face owns nothing, one ulp inside it owns the face's voxels.  Across the plane the samples sit
    # on voxel centres (16 x 8 x 4, exact) or inside the half-voxel rim of voxel 0 (7 x 1 x 3, where no centre is a float32)
    for d in ((7, 1, 3), (16, 8, 4)):
        for axis in (0, 1, 2):
            cu, cv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
            if d == (16, 8, 4):
                su, sv = 1 / 8, 1 / 4                                  # 8 x 4 pixels on voxel centres
                ou, ov = 0.5 / d[cu] if d[cu] <= 8 else 0.5 / 16, 0.5 / d[cv] if d[cv] <= 4 else 0.5 / 8
            else:
                su, sv, ou, ov = 1 / 128, 1 / 64, 1 / 128, 1 / 16     # all within 1/14 resp. 1/6 of the near faces
            for at, name in ((0.0, "on 0"), (1.0, "on 1"), (BELOW_ONE, "below 1"), (TINY, "above 0")):
                own = at not in (0.0, 1.0)
                cs.append(_case("faces", "face %s=%s %dx%dx%d" % ("xyz"[axis], name, *d), d,
                                _geo(8, 4, _axes((at, ou, ov), axis), _axes((0, su, 0), axis), _axes((0, 0, sv), axis)),
                                hits=(() if own else ("all_empty", "zero" if at == 0.0 else "one")),
                                column=(axis, (d[axis] - 1 if at == BELOW_ONE else 0)) if own else None, owns=own))
    # rim: within half a voxel of a face along the normal both taps clamp to the face's voxel
    d = (16, 8, 4)
    for axis in (0, 1, 2):
        cu, cv = {0: (1, 2), 1: (0, 2), 2: (0, 1)}[axis]
        half = 0.5 / d[axis]
        for at, index in ((half / 2, 0), (half, 0), (1 - half / 2, d[axis] - 1), (1 - half, d[axis] - 1)):
            cs.append(_case("rim", "rim %s=%g" % ("xyz"[axis], at), d,
                            _geo(d[cu], d[cv], _axes((at, 0.5 / d[cu], 0.5 / d[cv]), axis), _axes((0, 1 / d[cu], 0), axis),
                                 _axes((0, 0, 1 / d[cv]), axis)), column=(axis, index), owns=True))
    # still steps
    cs.append(_case("still", "still du=dv=0", SCENE_DIMS,
                    _geo(17, 3, (5 / 16, 19 / 32, 7 / 16), (0, 0, 0), (0, 0, 0), (1 / 64, 1 / 128, -1 / 64), 5), still="pixels"))
    for layers in (2, 64):
        cs.append(_case("still", "still dw=0 x%d" % layers, (16, 8, 4),
                        _geo(9, 5, (3 / 64, 5 / 64, 9 / 32), (7 / 64, 0, 1 / 128), (0, 13 / 64, 1 / 128), (0, 0, 0), layers),
                        still="layers"))
    # overflowing steps: (float)px * du is inf from px = 2 on, and inf - inf is NaN at pixel (2, 2)
    cs.append(_case("overflow", "overflow", (16, 8, 4), _geo(3, 3, (1 / 2, 1 / 2, 1 / 2), (2e38, 0, 0), (-2e38, 0, 0)),
                    hits=("nan", "zero")))
    # deep stacks: 1000 layers.  1 / 800 is no dyadic number: layer 100 and 900 land within rounding of 0 and 1 (in float32
    # ON them), and every eighth layer within rounding of a voxel boundary of the 300 voxels, so ref64 rounds as float32 does
    for d in ((1, 1, 300), (16, 8, 4)):
        cs.append(_case("deep", "deep %dx%dx%d" % d, d,
                        _geo(3, 3, (3 / 16, 5 / 16, -1 / 8), (5 / 16, 0, 0), (0, 3 / 16, 0), (0, 0, 1 / 800), 1000),
                        round32=True, count=799))
    # exact slabs: the lattice on 16 x 8 x 4 as a global volume, cut along each axis with one halo layer
    from volumerenderer_amd import distributed as D
    d = (16, 8, 4)
    for layers in (5, 1):
        for axis, worlds in ((0, (2, 3, 4, 5, 8)), (1, (2, 3, 4, 8)), (2, (2, 4))):
            for world in worlds:
                geo = _geo(41, 41, layers=layers, **LATTICE)
                slabs = []
                for r in range(world):
                    p, local, (a0, a1) = D.slab_plane(plane_of(geo, "nearest"), d, axis, r, world, 1)
                    sl = [slice(None)] * 3
                    sl[2 - axis] = slice(a0, a1)
                    sub = np.ascontiguousarray(volume(d)[tuple(sl)])
                    sub.setflags(write=False)
                    g = dict(geo, box_min=f32(p.box_min), box_max=f32(p.box_max), global_dims=p.global_dims, vol_origin=p.vol_origin)
                    assert tuple(local) == sub.shape[::-1] and g["box_min"] == tuple(p.box_min)      # the faces are dyadic
                    slabs.append((g, sub))
                cs.append(_case("slabs", "slabs %s%d x%d" % ("xyz"[axis], world, layers), d, geo, slabs=slabs,
                                hits=("box_min", "box_max")))
    # general families: masked and capped
    from volumerenderer_amd.render import SlicePlane
    for which, (center, right, down, extent, lp) in enumerate(PLANES):
        for d in (SCENE_DIMS, (7, 1, 3)):
            for layers in (1, 7):
                p = SlicePlane.from_frame(center, right, down, 65, 63, extent / 65, layers, lp)
                cs.append(_case("general", "plane %d %dx%dx%d x%d" % (which, *d, layers), d,
                                _geo(65, 63, p.origin, p.du, p.dv, p.dw, layers), exact=False))
    assert len({c["name"] for c in cs}) == len(cs)
    return cs


def family(name):
    return [k for k, c in enumerate(cases()) if c["family"] == name]


def hit(case, what):
    """Whether the case reaches `what`: a sample exactly at 0.0, at 1.0, on box_min, on box_max (of a rank's box for the
    exact slabs) or with pos * G integral inside the cube, a NaN position, an all-empty frame, or n taking every value
    from 0 to layers."""
    geos = [(case["geo"], case["vol"])] + list(case["slabs"] or [])
    if what in ("every_n", "all_empty"):
        n = ref64(case["vol"], plane(case, NEAREST), MAX, case["round32"]).n
        return not n.any() if what == "all_empty" else set(range(case["geo"]["layers"] + 1)) <= set(n.ravel().tolist())
    for geo, vol in geos:
        pl = plane_of(geo, NEAREST)
        pos, _ = positions64(pl)
        _, G, _ = _dims_of(vol, pl)
        c = (1, 3, 1, 1)
        with np.errstate(invalid="ignore"):
            inner = ((pos > 0) & (pos < 1)).all(1, keepdims=True)
            g = pos * np.array(G, np.float64).reshape(c)
            found = {"zero": pos == 0.0, "one": pos == 1.0, "nan": np.isnan(pos),
                     "box_min": (pos == _vec(pl.box_min).reshape(c)) & (pos > 0),
                     "box_max": (pos == _vec(pl.box_max).reshape(c)) & (pos < 1),
                     "voxel_boundary": inner & (g == np.rint(g))}[what]
        if found.any():
            return True
    return False


# ---- the checks both modules run, on a float32 partial of refslice or of the kernel --------------------------------------
K255 = np.float32(1) / np.float32(255)


def ref32(vol, pl, op):
    """refslice.partial; positions beyond float32 are part of the table, so NumPy's warnings about them are not."""
    import refslice as RS
    with np.errstate(all="ignore"):
        return RS.partial(vol, pl, op)


def compare(case, vol, geo, flt, op, part):
    """A float32 partial [H][W][4] held to ref64 on the decided pixels: n equal; NEAREST's MAX and MIN the float32 of
    ref64's voxel bit for bit; LINEAR, and MEAN over max(n, 1), within TOL.  Returns (largest difference, masked count)."""
    pl = plane_of(geo, flt)
    ref = ref64(vol, pl, op, case["round32"])
    ok = decided(case, ref)
    masked = check_cap(case, ref)
    assert part.dtype == np.float32 and part.shape == ok.shape + (4,) and not part[..., 2:].any(), case["name"]
    assert np.array_equal(part[..., 1][ok], ref.n[ok].astype(np.float32)), (case["name"], flt, op, "n")
    if flt == NEAREST and op != MEAN:
        want = np.where(ref.n > 0, ref.voxel.astype(np.float32) * K255, np.float32(0))
        assert np.array_equal(part[..., 0][ok], want[ok]), (case["name"], flt, op, "voxel")
        return 0.0, masked
    scale = np.maximum(ref.n, 1) if op == MEAN else 1
    err = float((np.abs(part[..., 0].astype(np.float64) - ref.v) / scale)[ok].max()) if ok.any() else 0.0
    assert err <= TOL, (case["name"], flt, op, err)
    return err, masked


def check_known(case, flt, op, part, run):
    """The answers a family knows without any reference.  run(vol, geo, flt, op) is the partial's source, for the one
    comparison that needs a second slice."""
    fam, geo, vol = case["family"], case["geo"], case["vol"]
    v, n = part[..., 0], part[..., 1]
    if case.get("owns") is False:
        assert not part.any(), case["name"]                            # a plane on a face owns nothing
    if case["column"] is not None:
        axis, index = case["column"]
        pos, _ = positions64(plane_of(geo, flt))
        idx = [np.clip(np.floor(pos[0, k] * case["dims"][k]).astype(np.int64), 0, case["dims"][k] - 1) for k in range(3)]
        idx[axis] = np.full_like(idx[axis], index)
        assert (n == 1).all() and np.array_equal(v, vol[idx[2], idx[1], idx[0]].astype(np.float32) * K255), (case["name"], flt, op)
    if case.get("still") == "pixels":
        assert (n > 0).all() and (part == part[0, 0]).all(), case["name"]
    if case.get("still") == "layers":
        one = run(vol, dict(geo, layers=1), flt, op)
        assert (one[..., 1] == 1).all() and (n == geo["layers"]).all(), case["name"]
        want = one[..., 0]
        if op == MEAN:
            want = np.zeros_like(want)
            for _ in range(geo["layers"]):
                want = want + one[..., 0]                               # the float32 running sum
        assert np.array_equal(v, want), (case["name"], flt, op)
    if fam == "overflow":
        want = np.zeros((3, 3), np.float32)
        want[0, 0] = 1
        assert np.array_equal(n, want) and not v[n == 0].any(), case["name"]
    if fam == "deep":
        assert (n == case["count"]).all(), (case["name"], n)            # layers 101 .. 899: 100 and 900 are ON 0 and 1 in float32


def check_reversed(case, flt, op, part, run):
    """The stack walked backwards (exact cases: the positions are identical): n, MAX and MIN bit-identical, MEAN the same n."""
    back = run(case["vol"], reversed_geo(case["geo"]), flt, op)
    assert np.array_equal(back[..., 1], part[..., 1]), (case["name"], flt, op)
    assert op == MEAN or np.array_equal(back, part), (case["name"], flt, op)


def check_rotated(case, flt, op, part, run):
    """Volume and plane rotated x -> y -> z -> x: NEAREST bit-identical for every op (each axis is decided on its own and
    MEAN adds the same values in the same order), LINEAR within TOL (the taps are blended in another order)."""
    vol, geo = rotated(case["vol"], case["geo"])
    turned = run(vol, geo, flt, op)
    assert np.array_equal(turned[..., 1], part[..., 1]), (case["name"], flt, op)
    if flt == NEAREST:
        assert np.array_equal(turned, part), (case["name"], flt, op)
    else:
        scale = np.maximum(part[..., 1], 1) if op == MEAN else 1
        assert (np.abs(turned[..., 0].astype(np.float64) - part[..., 0]) / scale).max() <= TOL, (case["name"], flt, op)
