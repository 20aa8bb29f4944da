"""The hand-built pools of the pool contract, shared by test_pool_contract_cpu.py (the references alone: the formula
against itself, the census, that wrong formulas are seen) and test_gpu_pool_contract.py (every pool reader against its
dense call on refpool.expand).  Data and small builders only: nothing here needs a GPU.

A case is a dict: name, geo (its geometry's index), bd, grid, shifts ((cells, 3)), order, gap, base, absent, alias, values,
view (the byte offset of the pool tensor in its allocation on the GPU), seed.  build(k) gives its pool bytes and table.
Per geometry the shift sets, as far as its extents allow (a shift is cut down to log2 of its extent; a set that repeats
an earlier one is dropped), each with the next table shape of a rotation; then the presence patterns, an alias and the
256-rounded layout on per-cell random shifts."""
import functools

import numpy as np

import refpool as R

# (brick_dims, grid): each the smallest at which its path can go wrong
GEOMETRIES = [
    ((1, 1, 1), (5, 3, 2)),        # every tap is a cell of its own; lx = ly = lz = 0
    ((2, 1, 4), (3, 4, 1)),        # extents of 1 and 2 mixed; a grid axis of 1
    ((4, 4, 4), (1, 1, 1)),        # the gradient box fits a brick at exactly one origin per axis
    ((4, 4, 4), (3, 2, 2)),
    ((8, 2, 16), (2, 5, 1)),       # non-cubic; every gradient box crosses y
    ((2, 2, 2), (64, 1, 1)),       # a long table row
    ((32, 32, 32), (2, 2, 2)),     # the existing family, now with hand-made tables
]
BASES = (0, 1, 3, 7)
VIEWS = (0, 1, 2, 3, 15)
GAPS = (0, 0, 1, 0, 5)
ORDERS = ("cell", "reversed", "random")


def ncells(grid):
    return grid[0] * grid[1] * grid[2]


def _order(kind, cells, rng):
    if kind == "cell":
        return list(range(cells))
    if kind == "reversed":
        return list(range(cells))[::-1]
    return [int(c) for c in rng.permutation(cells)]


def shift_sets(bd, grid, rng):
    """[(name, (cells, 3) shifts)] of a geometry."""
    full = np.array([R.ilog2(q) for q in bd])
    cells = ncells(grid)
    D = int(full.sum())
    one = lambda t: np.tile(np.minimum(np.array(t), full), (cells, 1))     # noqa: E731
    sets = [("zero", one((0, 0, 0))), ("full", one(full)), ("full-x", one((full[0], 0, 0))),
            ("full-y", one((0, full[1], 0))), ("full-z", one((0, 0, full[2]))), ("half-x", one((1, 0, 0))),
            ("0-3-1", one((0, 3, 1))),
            ("kd", np.array([R.kd_shifts(bd, c % (D + 1)) for c in range(cells)]).reshape(cells, 3)),
            ("random", np.stack([rng.integers(0, full + 1) for _ in range(cells)]))]
    out = []
    for name, s in sets:
        if not any(np.array_equal(s, q) for _, q in out):
            out.append((name, s))
    return out


def presence_patterns(grid):
    """[(name, absent cells)]: all absent, a checkerboard, a single present cell at a corner and in the middle."""
    gx, gy, gz = grid
    cells = ncells(grid)
    every = set(range(cells))
    board = {c for c in range(cells) if (c % gx + (c // gx) % gy + c // (gx * gy)) % 2}
    mid = (gx // 2) + gx * ((gy // 2) + gy * (gz // 2))
    return [("all-absent", every), ("checkerboard", board), ("corner-only", every - {cells - 1}), ("middle-only", every - {mid})]


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for geo, (bd, grid) in enumerate(GEOMETRIES):
        rng = np.random.default_rng(1000 + geo)
        cells = ncells(grid)
        sets = shift_sets(bd, grid, rng)
        rnd = sets[-1][1]

        def add(name, shifts, absent=(), alias=None, gap=None, values=None):
            i = len(out)
            out.append(dict(name="%dx%dx%d on %dx%dx%d %s" % (bd + grid + (name,)), geo=geo, bd=bd, grid=grid, shifts=shifts,
                            order=_order(ORDERS[i % 3], cells, rng), gap=GAPS[i % len(GAPS)] if gap is None else gap,
                            base=BASES[i % 4] if gap is None else 0, absent=frozenset(absent), alias=alias,
                            values=values or ("smooth" if i % 2 == 0 else "noise"), view=VIEWS[(i // 3) % 5], seed=7000 + i))

        for name, s in sets:
            add(name, s)
        for name, absent in presence_patterns(grid):
            if name != "all-absent" and len(absent) in (0, cells):
                continue                               # one cell: present is the shift sets', absent is all-absent
            add(name, sets[0][1] if name == "checkerboard" else rnd, absent=absent, values="smooth")
        if cells > 1:
            add("alias", rnd, alias={cells - 1: 0}, values="smooth")
        add("round256", rnd, gap="round256", values="smooth")
    return out


@functools.lru_cache(maxsize=None)
def build(k):
    """(pool, table) of case k."""
    c = cases()[k]
    return R.make_pool(np.random.default_rng(c["seed"]), c["bd"], c["grid"], c["shifts"], c["order"], c["gap"], c["absent"],
                       c["base"], c["values"], c["alias"])


@functools.lru_cache(maxsize=None)
def volume(k):
    """refpool.expand of case k: computed once, shared, never written."""
    c = cases()[k]
    pool, table = build(k)
    v = R.expand(pool, table, c["bd"], c["grid"])
    v.setflags(write=False)
    return v


def of_geometry(geo):
    return [k for k, c in enumerate(cases()) if c["geo"] == geo]


# ---- the high-offset case: one slot beyond 2^32, a different one at the same offset modulo 2^32 -----------------------
HIGH_BD, HIGH_GRID = (8, 4, 4), (2, 1, 1)
HIGH_BYTES = (1 << 32) + (1 << 20)
HIGH_AT = ((1 << 32) + 4099, 4099)


@functools.lru_cache(maxsize=None)
def high_offset():
    """(segments, table, SegPool): cell 0's slot at 2^32 + 4099 and cell 1's at 4099, each a segment of slot + noise tail
    (and 64 bytes of noise before it).  No slot lies between 2^31 and 2^32: a sign-wrapped offset would leave the pool."""
    rng = np.random.default_rng(99)
    n = HIGH_BD[0] * HIGH_BD[1] * HIGH_BD[2]
    table = np.zeros(2, R.POOL_ENTRY)
    segments = []
    for c, at in enumerate(HIGH_AT):
        table["offset"][c] = at
        segments.append((at - 64, rng.integers(0, 256, 64 + 2 * n + 64, dtype=np.uint8)))
    return segments, table, R.SegPool(segments, HIGH_BYTES)
