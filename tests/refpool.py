"""The level-of-detail pool as vrhip.h defines it by its bytes ("the table contract", at vr_pool_entry), in plain NumPy:
test infrastructure only.  A table of POOL_ENTRY rows (one per grid cell, x fastest) gives an offset and a shift[3] per
cell; virtual voxel (x, y, z) of cell (x / X, y / Y, z / Z) is

    pool[e.offset + (lx >> sx) + (X >> sx) * ((ly >> sy) + (Y >> sy) * (lz >> sz))]

with (lx, ly, lz) the position in the brick, and 0 where e.offset is negative.  expand() is that formula vectorised,
expand_naive() the formula as it reads; make_pool() writes pools no producer of the project would (any shift triple, slots
at any byte in any order, noise everywhere else); classes() counts what a geometry makes the readers do."""
import numpy as np

# vr_pool_entry, restated (volumerenderer_amd.render.POOL_ENTRY; test_pool_contract_cpu.py asserts them equal)
POOL_ENTRY = np.dtype([("offset", "<i8"), ("shift", "u1", (3,)), ("pad", "u1", (5,))])


def ilog2(v):
    n = int(v).bit_length() - 1
    assert v > 0 and 1 << n == v, "%r is not a power of two" % (v,)
    return n


class SegPool:
    """Pool bytes given as a few segments [(start, uint8 array)] of a buffer too large to hold on the host: indexable by
    an int64 index array like the array it stands for.  An index outside every segment is an error (the test that uses
    it places noise tails so that a plausible wrong address still lands in a segment)."""

    def __init__(self, segments, size):
        self.segments = [(int(s), np.ascontiguousarray(a, np.uint8)) for s, a in segments]
        self.size = int(size)

    def __getitem__(self, idx):
        idx = np.asarray(idx, np.int64)
        out = np.zeros(idx.shape, np.uint8)
        hit = np.zeros(idx.shape, bool)
        for s, a in self.segments:
            m = (idx >= s) & (idx < s + a.size)
            out[m] = a[idx[m] - s]
            hit |= m
        if not hit.all():
            raise IndexError("address %d lies in no segment" % int(idx[~hit].reshape(-1)[0]))
        return out


def expand(pool, table, brick_dims, grid):
    """The dense virtual volume [Z][Y][X] (uint8) of a pool, by the header's formula, one cell at a time."""
    X, Y, Z = (int(q) for q in brick_dims)
    gx, gy, gz = (int(q) for q in grid)
    table = np.asarray(table).view(POOL_ENTRY).reshape(-1)
    assert table.size == gx * gy * gz
    vol = np.zeros((gz * Z, gy * Y, gx * X), np.uint8)
    for c, e in enumerate(table):
        off = int(e["offset"])
        if off < 0:
            continue
        sx, sy, sz = (int(q) for q in e["shift"])
        lx, ly, lz = np.arange(X) >> sx, np.arange(Y) >> sy, np.arange(Z) >> sz
        idx = off + lx[None, None, :] + (X >> sx) * (ly[None, :, None] + (Y >> sy) * lz[:, None, None])
        i, j, k = c % gx, (c // gx) % gy, c // (gx * gy)
        vol[k * Z:(k + 1) * Z, j * Y:(j + 1) * Y, i * X:(i + 1) * X] = pool[idx.astype(np.int64)]
    return vol


def expand_naive(pool, table, brick_dims, grid):
    """expand(), one voxel at a time, in the header's words (for the CPU module only)."""
    X, Y, Z = (int(q) for q in brick_dims)
    gx, gy, gz = (int(q) for q in grid)
    table = np.asarray(table).view(POOL_ENTRY).reshape(-1)
    vol = np.zeros((gz * Z, gy * Y, gx * X), np.uint8)
    one = isinstance(pool, np.ndarray)
    for z in range(gz * Z):
        for y in range(gy * Y):
            for x in range(gx * X):
                e = table[(x // X) + gx * ((y // Y) + gy * (z // Z))]
                if e["offset"] < 0:
                    continue
                sx, sy, sz = (int(q) for q in e["shift"])
                lx, ly, lz = x % X, y % Y, z % Z
                a = int(e["offset"]) + (lx >> sx) + (X >> sx) * ((ly >> sy) + (Y >> sy) * (lz >> sz))
                vol[z, y, x] = pool[a] if one else pool[np.array([a])][0]
    return vol


def kd_shifts(brick_dims, cut):
    """The shift triple vr_lod_pool_layout gives a brick cut at `cut` (the split rule of vrhip.h): depth d splits axis
    d % 3, or the next axis that still has an extent above 1; shift_k = log2(extent_k) - the splits on k among depths
    0 .. min(cut, D) - 1."""
    ext = [int(q) for q in brick_dims]
    full = [ilog2(q) for q in ext]
    n = [0, 0, 0]
    for d in range(min(int(cut), sum(full))):
        k = d % 3
        while ext[k] == 1:
            k = (k + 1) % 3
        ext[k] //= 2
        n[k] += 1
    return tuple(full[k] - n[k] for k in range(3))


def smooth_field(dims):
    """A smooth [Z][Y][X] float field over the virtual volume, in 0 .. 255: crosses 100 (the iso value the frames use) on a
    tilted wavy sheet, whatever the extents."""
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    u, v, w = (x + 0.5) / X, (y + 0.5) / Y, (z + 0.5) / Z
    h = 0.45 + 0.18 * np.sin(5.1 * u + 0.4) + 0.14 * np.cos(4.3 * v)
    f = 128.0 + 118.0 * np.tanh((w - h) * 5.0) + 9.0 * np.sin(23.0 * u + 17.0 * v + 11.0 * w)
    return np.clip(f, 0.0, 255.0)


def make_pool(rng, brick_dims, grid, shifts, order=None, gap=0, absent=(), base=0, values="noise", alias=None):
    """(pool, table): pool bytes (uint8) and a POOL_ENTRY table.
      shifts  one triple for every cell, or a (cells, 3) array; shift_k <= log2(brick_dims_k)
      order   the cells in the order their slots lie in the pool (a permutation of range(cells); default: cell order)
      gap     bytes of noise between one slot and the next, or "round256": every slot at the next multiple of 256
      absent  cells with offset -1 (and a shift of noise, which nothing may read)
      base    the byte offset of the first slot
      values  "noise": every stored voxel random; "smooth": smooth_field at the box's min corner
      alias   {cell: other}: the cell gets no slot of its own and names the other's (offset and shifts)
    Everything outside the slots is noise, and the pool ends in a noise tail as long as the largest slot (at least 64
    bytes): an address one byte, one row or one plane off reads other data, not zeros, and stays inside the buffer."""
    X, Y, Z = (int(q) for q in brick_dims)
    gx, gy, gz = (int(q) for q in grid)
    cells = gx * gy * gz
    full = (ilog2(X), ilog2(Y), ilog2(Z))
    sh = np.broadcast_to(np.asarray(shifts, np.int64).reshape(-1, 3), (cells, 3)).copy()
    assert (sh >= 0).all() and (sh <= np.array(full)).all(), "a shift beyond log2 of its extent"
    order = list(range(cells)) if order is None else [int(c) for c in order]
    assert sorted(order) == list(range(cells))
    alias = dict(alias or {})
    absent = set(int(c) for c in absent)
    for c, o in alias.items():
        sh[c] = sh[o]
        assert o not in alias and o not in absent and c not in absent
    size = lambda c: (X >> sh[c, 0]) * (Y >> sh[c, 1]) * (Z >> sh[c, 2])   # noqa: E731
    table = np.zeros(cells, POOL_ENTRY)
    at, largest = int(base), 64
    for c in order:
        if c in absent or c in alias:
            continue
        if gap == "round256":
            at = (at + 255) & ~255
        table["offset"][c] = at
        at += int(size(c)) + (0 if gap == "round256" else int(gap))
        largest = max(largest, int(size(c)))
    pool = rng.integers(0, 256, at + largest + int(X), dtype=np.uint8)
    field = smooth_field((gx * X, gy * Y, gz * Z)) if values == "smooth" else None
    for c in range(cells):
        table["shift"][c] = sh[c]
        if c in absent:
            table["offset"][c] = -1
            table["shift"][c] = rng.integers(0, 256, 3)
            continue
        if c in alias:
            table["offset"][c] = table["offset"][alias[c]]
            continue
        if field is not None:
            i, j, k = c % gx, (c // gx) % gy, c // (gx * gy)
            sx, sy, sz = (int(q) for q in sh[c])
            box = field[k * Z:(k + 1) * Z:1 << sz, j * Y:(j + 1) * Y:1 << sy, i * X:(i + 1) * X:1 << sx]
            o = int(table["offset"][c])
            pool[o:o + box.size] = np.rint(box).astype(np.uint8).reshape(-1)
    return pool, table


CLASSES = ("tap_one_cell", "tap_across", "tap_one_cell_absent", "box_one_cell", "box_across", "box_one_cell_absent",
           "pair_step1", "pair_same_coarse", "clamp_x", "clamp_y", "clamp_z", "beside_absent_x", "beside_absent_y",
           "beside_absent_z", "row_1", "row_2", "row_3", "row_4plus")
# what the one-cell branches of tex3d_pool and of the pool gather tell apart
ONE_CELL_CLASSES = ("tap_one_cell", "tap_one_cell_absent", "box_one_cell", "box_one_cell_absent", "pair_step1",
                    "pair_same_coarse", "clamp_x", "clamp_y", "clamp_z")


def classes(brick_dims, grid, table):
    """The census of a geometry: counts over all lattice origins (x0, y0, z0), each axis from -1 to G - 1 (the floor of
    every sample position a ray can take inside the cube), of
      tap_one_cell / tap_across      the eight trilinear taps clamp(x0), clamp(x0 + 1) ... lie in one cell / do not
      tap_one_cell_absent            ... in one cell, which is absent
      box_one_cell / box_across      the gradient's taps clamp(x0 - 1) .. clamp(x0 + 2) per axis, likewise
      box_one_cell_absent
      pair_step1 / pair_same_coarse  one-cell tap sets of a present cell whose stored x indices are lb == la + 1 (the 16-bit
                                     row load) / lb == la although xb != xa (one stored voxel for both taps)
      clamp_x, _y, _z                one-cell tap sets whose two taps on that axis the clamp collapses (xb == xa)
      beside_absent_x, _y, _z        neighbouring cells along the axis of which exactly one is absent
      row_1, _2, _3, _4plus          present cells by the bytes of a stored row, X >> sx."""
    bd = [int(q) for q in brick_dims]
    g = [int(q) for q in grid]
    t = np.asarray(table).view(POOL_ENTRY).reshape(g[2], g[1], g[0])
    present = t["offset"] >= 0
    ax = []
    for k in range(3):
        G = g[k] * bd[k]
        x0 = np.arange(-1, G)
        a, b = np.clip(x0, 0, G - 1), np.clip(x0 + 1, 0, G - 1)
        m, p = np.clip(x0 - 1, 0, G - 1), np.clip(x0 + 2, 0, G - 1)
        ax.append(dict(n=x0.size, a=a, b=b, cell=a // bd[k], pair=(a // bd[k]) == (b // bd[k]),
                       box=(m // bd[k]) == (p // bd[k]), boxcell=m // bd[k], flat=a == b))
    out = dict.fromkeys(CLASSES, 0)
    total = ax[0]["n"] * ax[1]["n"] * ax[2]["n"]
    out["tap_one_cell"] = int(np.prod([q["pair"].sum() for q in ax]))
    out["tap_across"] = total - out["tap_one_cell"]
    out["box_one_cell"] = int(np.prod([q["box"].sum() for q in ax]))
    out["box_across"] = total - out["box_one_cell"]
    for k, name in enumerate(("clamp_x", "clamp_y", "clamp_z")):
        out[name] = int(np.prod([(q["flat"] if j == k else q["pair"]).sum() for j, q in enumerate(ax)]))
    for cz in range(g[2]):
        for cy in range(g[1]):
            for cx in range(g[0]):
                cc = (cx, cy, cz)
                taps = [q["pair"] & (q["cell"] == cc[k]) for k, q in enumerate(ax)]
                boxes = [q["box"] & (q["boxcell"] == cc[k]) for k, q in enumerate(ax)]
                ntap, nbox = int(np.prod([s.sum() for s in taps])), int(np.prod([s.sum() for s in boxes]))
                if not present[cz, cy, cx]:
                    out["tap_one_cell_absent"] += ntap
                    out["box_one_cell_absent"] += nbox
                    continue
                sx = int(t["shift"][cz, cy, cx][0])
                la, lb = (ax[0]["a"] % bd[0]) >> sx, (ax[0]["b"] % bd[0]) >> sx
                nyz = int(taps[1].sum() * taps[2].sum())
                out["pair_step1"] += int((taps[0] & (lb == la + 1)).sum()) * nyz
                out["pair_same_coarse"] += int((taps[0] & (lb == la) & ~ax[0]["flat"]).sum()) * nyz
                row = bd[0] >> sx
                out["row_%s" % ("4plus" if row >= 4 else row)] += 1
    out["beside_absent_x"] = int((present[:, :, 1:] != present[:, :, :-1]).sum())
    out["beside_absent_y"] = int((present[:, 1:, :] != present[:, :-1, :]).sum())
    out["beside_absent_z"] = int((present[1:, :, :] != present[:-1, :, :]).sum())
    return out
