"""The pool contract without a GPU: the references of test_gpu_pool_contract.py against each other, the census of what
its case list contains, and that the comparison would see a wrong address formula.

  * refpool.expand (vectorised) == refpool.expand_naive (the header's sentence, a voxel at a time) on every case;
  * refhist.hist_pool == the per-cell bincount of expand; _grid_def of test_gpu_raymarch_edges.py, imported, is the
    skip-grid reference the GPU module uses;
  * the census (refpool.classes): every class occurs over the list, every class the one-cell branches distinguish in at
    least two geometries, and where a geometry cannot hold a class the impossibility is asserted;
  * nine one-term errors in expand's formula each change at least one case's volume."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import poolcases as PC  # noqa: E402
import refhist  # noqa: E402
import refpool as R  # noqa: E402
from test_gpu_raymarch_edges import _grid_def  # noqa: E402

SKIP_CELLS = (1, 3, 8, 31, 64)


def test_entry_layout_is_the_packages():
    from volumerenderer_amd.render import POOL_ENTRY
    assert R.POOL_ENTRY == POOL_ENTRY and R.POOL_ENTRY.itemsize == 16
    assert [R.POOL_ENTRY.fields[n][1] for n in ("offset", "shift", "pad")] == [0, 8, 11]


def test_kd_shifts_are_the_layouts():
    """refpool.kd_shifts restates the split rule; vr_lod_pool_layout (host only) is the rule."""
    import volumerenderer_amd as vr
    for bd in [g[0] for g in PC.GEOMETRIES] + [(128, 8, 4), (4, 1, 2)]:
        D = sum(R.ilog2(q) for q in bd)
        for cut in range(D + 2):
            t, _ = vr.lod_pool_layout(bd, np.array([(0, 0, 0)]), (1, 1, 1), [cut], D, D + 1)
            assert tuple(int(q) for q in t[0]["shift"]) == R.kd_shifts(bd, cut), (bd, cut)


def test_case_list_has_every_table_shape():
    cs = PC.cases()
    assert {c["geo"] for c in cs} == set(range(len(PC.GEOMETRIES)))
    assert {c["base"] for c in cs if c["gap"] == 0} == set(PC.BASES)
    assert {c["view"] for c in cs} == set(PC.VIEWS)
    assert {c["gap"] for c in cs} >= {0, 1, 5, "round256"}
    orders = {("cell" if c["order"] == sorted(c["order"]) else "reversed" if c["order"] == sorted(c["order"])[::-1] else "random")
              for c in cs if len(c["order"]) > 2}
    assert orders == {"cell", "reversed", "random"}
    for geo, (bd, grid) in enumerate(PC.GEOMETRIES):
        names = {cs[k]["name"].split()[-1] for k in PC.of_geometry(geo)}
        assert {"zero", "all-absent", "round256"} <= names, (geo, names)
        if PC.ncells(grid) > 1:
            assert {"checkerboard", "corner-only", "middle-only", "alias"} <= names, (geo, names)
        if max(bd) > 1:
            assert {"full", "random"} <= names, (geo, names)
    for k, c in enumerate(cs):
        pool, table = PC.build(k)
        n = [(c["bd"][0] >> s[0]) * (c["bd"][1] >> s[1]) * (c["bd"][2] >> s[2]) for s in table["shift"].astype(int)]
        live = [i for i in range(table.size) if table["offset"][i] >= 0]
        assert all(table["offset"][i] + n[i] <= pool.size - max([n[j] for j in live]) for i in live), c["name"]
        if c["alias"]:
            (a, b), = c["alias"].items()
            assert table["offset"][a] == table["offset"][b] >= 0


@pytest.mark.parametrize("geo", range(len(PC.GEOMETRIES)))
def test_expand_is_the_naive_formula(geo):
    for k in PC.of_geometry(geo):
        c = PC.cases()[k]
        pool, table = PC.build(k)
        if c["bd"] == (32, 32, 32) and k != PC.of_geometry(geo)[-1]:
            # 262144 voxels a case: the naive walk over cell 0's brick, and over the geometry's last case whole
            sub = R.expand_naive(pool, table[:1], c["bd"], (1, 1, 1))
            assert np.array_equal(sub, PC.volume(k)[:32, :32, :32]), c["name"]
            continue
        assert np.array_equal(R.expand_naive(pool, table, c["bd"], c["grid"]), PC.volume(k)), c["name"]


def test_expand_high_offset():
    _, table, seg = PC.high_offset()
    a, b = R.expand(seg, table, PC.HIGH_BD, PC.HIGH_GRID), R.expand_naive(seg, table, PC.HIGH_BD, PC.HIGH_GRID)
    assert np.array_equal(a, b)
    X = PC.HIGH_BD[0]
    assert not np.array_equal(a[:, :, :X], a[:, :, X:])        # the two slots hold different data
    assert all(not (1 << 31) <= s < (1 << 32) and not (1 << 31) <= s + v.size < (1 << 32) for s, v in seg.segments)


def _cell_blocks(vol, bd, grid):
    X, Y, Z = bd
    for c in range(PC.ncells(grid)):
        i, j, k = c % grid[0], (c // grid[0]) % grid[1], c // (grid[0] * grid[1])
        yield c, vol[k * Z:(k + 1) * Z, j * Y:(j + 1) * Y, i * X:(i + 1) * X]


def test_hist_pool_is_the_histogram_of_expand():
    for k, c in enumerate(PC.cases()):
        pool, table = PC.build(k)
        cells, total = refhist.hist_pool(pool, table, c["bd"], c["grid"])
        for i, blk in _cell_blocks(PC.volume(k), c["bd"], c["grid"]):
            assert np.array_equal(cells[i], np.bincount(blk.reshape(-1), minlength=256)), (c["name"], i)
        assert np.array_equal(total, np.bincount(PC.volume(k).reshape(-1), minlength=256))


def test_grid_def_of_expand():
    """The skip-grid reference on expand's volumes: cells larger than a brick and cells that divide nothing give one
    (min, max) per cell, and between them the volume's own extremes."""
    for k in [PC.of_geometry(g)[-3] for g in range(len(PC.GEOMETRIES))]:
        c, vol = PC.cases()[k], PC.volume(k)
        for S in SKIP_CELLS:
            g = _grid_def(vol, S).reshape(-1, 2)
            n = [(q + S - 1) // S for q in vol.shape]
            assert g.shape[0] == n[0] * n[1] * n[2] and (g[:, 0] <= g[:, 1]).all()
            assert g[:, 0].min() == vol.min() and g[:, 1].max() == vol.max(), (c["name"], S)


# ---- the census ------------------------------------------------------------------------------------------------------
def _census():
    return [R.classes(c["bd"], c["grid"], PC.build(k)[1]) for k, c in enumerate(PC.cases())]


def test_census_every_class_occurs():
    cen = _census()
    for name in R.CLASSES:
        n = sum(1 for q in cen if q[name])
        if name == "row_3":
            # brick extents are powers of two (every reader refuses others), so X >> sx is one: a stored row of 3 bytes is
            # in no pool of the contract
            assert n == 0
            continue
        assert n > 0, name
    for name in R.ONE_CELL_CLASSES:
        geos = {c["geo"] for c, q in zip(PC.cases(), cen) if q[name]}
        assert len(geos) >= 2, (name, geos)


def test_census_impossibilities():
    cen, cs = _census(), PC.cases()
    for q, c in zip(cen, cs):
        bd, grid = c["bd"], c["grid"]
        G = [bd[k] * grid[k] for k in range(3)]
        assert q["tap_one_cell"] + q["tap_across"] == q["box_one_cell"] + q["box_across"] == (G[0] + 1) * (G[1] + 1) * (G[2] + 1)
        if bd == (1, 1, 1):
            # a cell is one voxel: two taps share a cell only where the clamp makes them one voxel, i.e. at the eight
            # corners of the lattice; no 4-tap box fits (its first and last index differ on a 5 x 3 x 2 volume); every
            # stored row is one byte
            assert q["tap_one_cell"] == q["clamp_x"] == q["clamp_y"] == q["clamp_z"] == 8
            assert q["box_one_cell"] == q["pair_step1"] == q["pair_same_coarse"] == q["row_2"] == q["row_4plus"] == 0
        if bd == (2, 1, 4):
            # Y = 1 on four cells: one-cell tap sets all collapse on y (the two ends), a 4-tap box never fits on y; one
            # cell along z: nothing beside it; rows of 1 or 2 bytes
            assert q["tap_one_cell"] == q["clamp_y"] and q["box_one_cell"] == 0
            assert q["beside_absent_z"] == 0 and q["row_4plus"] == 0
        if bd == (4, 4, 4) and grid == (1, 1, 1):
            assert q["tap_across"] == q["box_across"] == 0 and not any(q["beside_absent_" + a] for a in "xyz")
        if bd == (4, 4, 4) and grid == (3, 2, 2):
            # per axis a box fits a brick at one unclamped origin (4c + 1) and at the two clamped origins of either end
            assert q["box_one_cell"] == (3 + 4) * (2 + 4) * (2 + 4)
        if bd == (8, 2, 16):
            # y: Y = 2, so a 4-tap box fits only clamped, at y0 = -1 and y0 = GY - 1; x: origins 1 .. 5 of each brick and
            # two clamped ones per end; z: one cell, every origin
            assert q["box_one_cell"] == (5 * 2 + 4) * 2 * 17
        if bd == (2, 2, 2):
            assert q["beside_absent_y"] == q["beside_absent_z"] == 0 and q["row_4plus"] == 0


# ---- the comparisons must bite ---------------------------------------------------------------------------------------
WRONG = ("sy-sz-swapped", "neighbour-shift", "mask-dropped", "row-stride-unshifted", "offset-32-bits", "absent-read",
         "plane-stride-unshifted", "sx-for-sy", "x-unshifted")


def _wrong_expand(kind, pool, table, bd, grid):
    """expand with one term wrong.  An address that leaves the buffer wraps round (the GPU module runs no such kernel:
    this only has to differ)."""
    X, Y, Z = bd
    gx, gy, gz = grid
    table = np.asarray(table).view(R.POOL_ENTRY).reshape(-1)
    vol = np.zeros((gz * Z, gy * Y, gx * X), np.uint8)
    for c, e in enumerate(table):
        off = int(e["offset"])
        i, j, k = c % gx, (c // gx) % gy, c // (gx * gy)
        if off < 0 and kind != "absent-read":
            continue
        sx, sy, sz = (int(q) for q in (table[(c + 1) % table.size] if kind == "neighbour-shift" else e)["shift"])
        if off < 0:
            sx = sy = sz = 0
        rx, ry = X >> sx, Y >> sy
        if kind == "sy-sz-swapped":
            sy, sz = sz, sy
        if kind == "sx-for-sy":
            sy = sx
        if kind == "offset-32-bits":
            off &= 0xFFFFFFFF
        x, y, z = np.arange(X), np.arange(Y), np.arange(Z)
        if kind == "mask-dropped":
            x, y, z = x + i * X, y + j * Y, z + k * Z
        lx, ly, lz = x >> (0 if kind == "x-unshifted" else sx), y >> sy, z >> sz
        if kind == "row-stride-unshifted":
            rx = X
        if kind == "plane-stride-unshifted":
            ry = Y
        idx = off + lx[None, None, :] + rx * (ly[None, :, None] + ry * lz[:, None, None])
        if isinstance(pool, np.ndarray):
            idx = idx % pool.size
        vol[k * Z:(k + 1) * Z, j * Y:(j + 1) * Y, i * X:(i + 1) * X] = pool[idx.astype(np.int64)]
    return vol


@pytest.mark.parametrize("kind", WRONG)
def test_a_wrong_formula_is_seen(kind):
    seen = []
    for k, c in enumerate(PC.cases()):
        pool, table = PC.build(k)
        if not np.array_equal(_wrong_expand(kind, pool, table, c["bd"], c["grid"]), PC.volume(k)):
            seen.append(c["name"])
    _, table, seg = PC.high_offset()
    try:
        if not np.array_equal(_wrong_expand(kind, seg, table, PC.HIGH_BD, PC.HIGH_GRID), R.expand(seg, table, PC.HIGH_BD, PC.HIGH_GRID)):
            seen.append("high offset")
    except IndexError:
        pass                                           # (an address in no segment: not this case's to see)
    print("WRONG %-24s seen by %d cases" % (kind, len(seen)))
    assert seen, kind
    if kind == "offset-32-bits":
        assert seen == ["high offset"]                 # every other pool is far below 2^32 bytes
