"""A NumPy float32 restatement of the slice views (vr_reslice; the rule is in include/vrhip.h).  The library is built with
-ffp-contract=off, so float32 NumPy reproduces every operation bit for bit: the positions, inside, ownership, the fetch
in tex3d's order, the reductions in layer order and the projection's finish.  dtype=np.float64 evaluates the same
float32 positions in double (the yardstick of the float32 restatement itself).  Used by test_reslice_cpu.py and
test_gpu_reslice.py."""
import numpy as np

F = np.float32
NEAREST, LINEAR = 0, 1
MAX, MIN, MEAN = 0, 1, 2
OPS = (MAX, MIN, MEAN)


def _f3(v):
    return np.array([float(q) for q in v], F)


def _global_dims(plane, local_dims):
    return [int(plane.global_dims[k]) if int(plane.global_dims[k]) > 0 else int(local_dims[k]) for k in range(3)]


def positions(plane, layer):
    """pos_k = ((origin_k + (float)px * du_k) + (float)py * dv_k) + (float)l * dw_k, float32: [3][H][W]."""
    o, du, dv, dw = _f3(plane.origin), _f3(plane.du), _f3(plane.dv), _f3(plane.dw)
    px = np.arange(plane.width, dtype=F)[None, :]
    py = np.arange(plane.height, dtype=F)[:, None]
    with np.errstate(over="ignore", invalid="ignore"):
        return np.stack([((o[k] + px * du[k]) + py * dv[k]) + F(layer) * dw[k] for k in range(3)]).astype(F)


def taken(plane, pos):
    """inside(pos) (strictly inside the unit cube) and pos in [box_min, box_max) on every axis."""
    bmin, bmax = _f3(plane.box_min), _f3(plane.box_max)
    t = np.ones(pos.shape[1:], bool)
    with np.errstate(invalid="ignore"):
        for k in range(3):
            t &= (pos[k] > 0) & (pos[k] < 1) & (pos[k] >= bmin[k]) & (pos[k] < bmax[k])
    return t


def _locate(idx, G, org, n):
    """A global voxel index in the local volume, as tex3d locates a tap."""
    return np.clip(np.clip(idx, 0, G - 1) - org, 0, n - 1)


def linear_taps(pos, G, dtype=F):
    """tex3d's base voxel (unclamped) and weights per axis at positions pos [3][...]."""
    base, frac = [], []
    for k in range(3):
        x = pos[k].astype(dtype) * dtype(G[k]) - dtype(0.5)
        x0 = np.floor(x)
        base.append(x0.astype(np.int64))
        frac.append((x - x0).astype(dtype))
    return base, frac


def fetch(vol, plane, pos, dtype=F):
    """The value of a sample at float32 positions pos [3][...] of the local volume vol [Z][Y][X] by plane.filter.
    Positions that are not taken are fetched too (harmlessly: every index is clamped)."""
    Z, Y, X = vol.shape
    n = (X, Y, Z)
    G = _global_dims(plane, n)
    org = [int(q) for q in plane.vol_origin]
    k255 = dtype(1) / dtype(255)
    pos = np.where(np.isfinite(pos), pos, F(0))
    if plane.filter == NEAREST:
        idx = [_locate(np.floor(pos[k].astype(dtype) * dtype(G[k])).astype(np.int64), G[k], org[k], n[k]) for k in range(3)]
        return vol[idx[2], idx[1], idx[0]].astype(dtype) * k255
    base, (fx, fy, fz) = linear_taps(pos, G, dtype)
    a = [_locate(base[k], G[k], org[k], n[k]) for k in range(3)]
    b = [_locate(base[k] + 1, G[k], org[k], n[k]) for k in range(3)]

    def c(ix, iy, iz):
        return vol[iz, iy, ix].astype(dtype) * k255

    c000, c100, c010, c110 = c(a[0], a[1], a[2]), c(b[0], a[1], a[2]), c(a[0], b[1], a[2]), c(b[0], b[1], a[2])
    c001, c101, c011, c111 = c(a[0], a[1], b[2]), c(b[0], a[1], b[2]), c(a[0], b[1], b[2]), c(b[0], b[1], b[2])
    c00, c10 = c000 + fx * (c100 - c000), c010 + fx * (c110 - c010)
    c01, c11 = c001 + fx * (c101 - c001), c011 + fx * (c111 - c011)
    c0, c1 = c00 + fy * (c10 - c00), c01 + fy * (c11 - c01)
    return c0 + fz * (c1 - c0)


def partial(vol, plane, op, dtype=F):
    """The projection partial [H][W][4] = (v, n, 0, 0) of the slice, reduced in ascending layer order."""
    shape = (plane.height, plane.width)
    n = np.zeros(shape, dtype)
    v = np.full(shape, {MAX: 0.0, MIN: np.inf, MEAN: 0.0}[op], dtype)
    for l in range(plane.layers):
        pos = positions(plane, l)
        t = taken(plane, pos)
        s = fetch(vol, plane, pos, dtype)
        n = n + t.astype(dtype)
        if op == MAX:
            v = np.where(t, np.maximum(v, s), v)
        elif op == MIN:
            v = np.where(t, np.minimum(v, s), v)
        else:
            v = np.where(t, v + s, v)
    out = np.zeros(shape + (4,), dtype)
    out[..., 0] = np.where(n > 0, v, 0)
    out[..., 1] = n
    return out


def finish(part, op, window=(0.0, 1.0), background=(0.0, 0.0, 0.0), lut=None, dtype=F):
    """finish_proj (raymarch.hip) in `dtype`: n == 0: (background, 0); m = v or v / n; the window; grey or the lookup."""
    v, n = part[..., 0].astype(dtype), part[..., 1].astype(dtype)
    lo, hi = dtype(F(window[0])), dtype(F(window[1]))
    bg = _f3(background).astype(dtype)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = v / n if op == MEAN else v
        w = np.minimum(np.maximum((m - lo) / (hi - lo), dtype(0)), dtype(1))
    w = np.where(n > 0, w, dtype(0))
    out = np.empty(v.shape + (4,), dtype)
    if lut is None:
        out[..., :3] = w[..., None]
        out[..., 3] = 1
    else:
        lut = np.asarray(lut, F).astype(dtype)
        x = np.minimum(np.maximum(w * dtype(255), dtype(0)), dtype(255))
        li = np.minimum(x.astype(np.int64), 254)
        f = x - li.astype(dtype)
        e0, e1 = lut[li], lut[li + 1]
        ea = np.minimum(np.maximum(e0[..., 3] + f * (e1[..., 3] - e0[..., 3]), dtype(0)), dtype(1))
        tb = dtype(1) - ea
        for c in range(3):
            col = e0[..., c] + f * (e1[..., c] - e0[..., c])
            out[..., c] = ea * col + tb * bg[c]
        out[..., 3] = ea
    empty = n == 0
    out[empty, :3] = bg
    out[empty, 3] = 0
    return out

