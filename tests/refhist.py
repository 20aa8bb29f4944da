"""NumPy restatements of the histogram rules of vrhip.h ("volume histograms"): test infrastructure only."""
import numpy as np

BINS, GRAD_BINS = 256, 111


def hist_bricks(data, num_bricks):
    """(bricks, total): per-brick uint32 (B, 256) and the uint64 (256,) sum of `data`'s B equal bricks."""
    d = np.ascontiguousarray(data, np.uint8).reshape(num_bricks, -1)
    rows = np.repeat(np.arange(num_bricks, dtype=np.int64) * BINS, d.shape[1])
    bricks = np.bincount(rows + d.reshape(-1), minlength=num_bricks * BINS).astype(np.uint32).reshape(num_bricks, BINS)
    return bricks, bricks.astype(np.uint64).sum(0)


def hist_pool(pool, table, brick_dims, grid):
    """(cells, total) of the virtual volume of a pool: stored voxels weighted by the box they stand for, an absent cell
    X*Y*Z in bin 0.  table: POOL_ENTRY rows, x fastest."""
    X, Y, Z = (int(q) for q in brick_dims)
    cells = np.zeros((len(table), BINS), np.uint32)
    for c, e in enumerate(table):
        if e["offset"] < 0:
            cells[c, 0] = X * Y * Z
            continue
        sx, sy, sz = (int(q) for q in e["shift"])
        n = (X >> sx) * (Y >> sy) * (Z >> sz)
        stored = pool[int(e["offset"]):int(e["offset"]) + n]
        cells[c] = np.bincount(stored, weights=np.full(n, 1 << (sx + sy + sz), np.float64), minlength=BINS).astype(np.uint32)
    return cells, cells.astype(np.uint64).sum(0)


def isqrt(s):
    """The exact integer square root of a non-negative integer array: a float sqrt corrected by one step either way."""
    s = np.asarray(s, np.int64)
    r = np.sqrt(s.astype(np.float64)).astype(np.int64)
    r = np.where(r * r > s, r - 1, r)
    return np.where((r + 1) * (r + 1) <= s, r + 1, r)


def hist2d(volume, global_dims=None, vol_origin=(0, 0, 0), own_lo=None, own_hi=None):
    """The (111, 256) uint64 table of the owned voxels.  volume: [Z][Y][X] uint8, the voxels [vol_origin, vol_origin +
    dims) of a volume of global_dims = (X, Y, Z) voxels; the own box in global coordinates, (x, y, z)."""
    v = np.asarray(volume, np.uint8).astype(np.int64)
    dims = v.shape[::-1]
    G = tuple(dims) if global_dims is None else tuple(int(g) or int(d) for g, d in zip(global_dims, dims))
    org = tuple(int(q) for q in vol_origin)
    lo = org if own_lo is None else tuple(int(q) for q in own_lo)
    hi = tuple(o + d for o, d in zip(org, dims)) if own_hi is None else tuple(int(q) for q in own_hi)
    p = [np.arange(lo[k], hi[k]) for k in range(3)]                      # global coordinates of the owned voxels

    def local(k, off):
        idx = np.clip(p[k] + off, 0, G[k] - 1) - org[k]
        assert idx.min() >= 0 and idx.max() < dims[k], "the volume does not hold a clamped neighbour"
        return idx

    def at(ox, oy, oz):
        return v[np.ix_(local(2, oz), local(1, oy), local(0, ox))]

    val = at(0, 0, 0)
    dx, dy, dz = at(1, 0, 0) - at(-1, 0, 0), at(0, 1, 0) - at(0, -1, 0), at(0, 0, 1) - at(0, 0, -1)
    r = isqrt(dx * dx + dy * dy + dz * dz) >> 2
    return np.bincount((r * BINS + val).reshape(-1), minlength=GRAD_BINS * BINS).astype(np.uint64).reshape(GRAD_BINS, BINS)


def window(hist, first_bin, lo_fraction, hi_fraction):
    """vr_window_from_histogram's rule, restated: (window_lo, window_hi) as float32, or None where it refuses."""
    h = [int(q) for q in hist]
    if not 0 <= first_bin <= 255 or not (0.0 <= lo_fraction <= 1.0) or not (0.0 <= hi_fraction <= 1.0) or lo_fraction > hi_fraction:
        return None
    n = sum(h[first_bin:])
    if n == 0:
        return None
    cum, lo_k, hi_k = 0, None, None
    for k in range(first_bin, 256):
        cum += h[k]
        if lo_k is None and float(cum) > lo_fraction * float(n):
            lo_k = k
        if hi_k is None and float(cum) >= hi_fraction * float(n):
            hi_k = k
    if lo_k is None:
        lo_k = max(k for k in range(first_bin, 256) if h[k])
    if hi_k <= lo_k:
        hi_k = lo_k + 1
    if hi_k > 255:
        lo_k, hi_k = lo_k - 1, hi_k - 1
    return np.float32(lo_k) / np.float32(255.0), np.float32(hi_k) / np.float32(255.0)
