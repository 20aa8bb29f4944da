"""The iso-surface mesh rule of include/vrhip.h ("iso-surface meshes") restated in NumPy, from the header's text alone:
lattice, inside test, six Kuhn tetrahedra per cell, edge vertices, triangles, ownership and order, gradients.  Loops over
points and cells: for test sizes only.

The winding is not a table here: every (permutation, inside mask) is decided from geometry, the sign of
cross(b - a, c - a) . (a - an inside corner) with every edge vertex at its edge's midpoint, so a mistake in the kernel's
table cannot be shared.  Volumes are [Z][Y][X] uint8 arrays of the GLOBAL volume; coordinates are (x, y, z)."""
import itertools

import numpy as np

F = np.float32
PERMS = list(itertools.permutations(range(3)))          # lexicographic: xyz, xzy, yxz, yzx, zxy, zyx
UNIT = np.eye(3, dtype=np.int64)


def cell_range(G, cap):
    """(lo, hi): the cells lo <= c < hi that exist per axis."""
    return ((-1,) * 3, tuple(G)) if cap else ((0,) * 3, tuple(g - 1 for g in G))


def _tet_corners(perm):
    a0 = np.zeros(3, np.int64)
    a1 = a0 + UNIT[perm[0]]
    a2 = a1 + UNIT[perm[1]]
    return [a0, a1, a2, np.ones(3, np.int64)]


_TRIS = {}


def tet_triangles(pi, m):
    """The triangles of tetrahedron `pi` with inside flags m = (m0, m1, m2, m3): a list of triangles, each three edges
    (i, j), i < j, wound counter-clockwise seen from the outside."""
    key = (pi, tuple(bool(q) for q in m))
    if key in _TRIS:
        return _TRIS[key]
    m = key[1]
    ins, outs = [i for i in range(4) if m[i]], [i for i in range(4) if not m[i]]
    pair = lambda i, j: (min(i, j), max(i, j))
    if len(ins) in (0, 4):
        tris = []
    elif len(ins) in (1, 3):
        i = ins[0] if len(ins) == 1 else outs[0]
        tris = [[pair(i, j) for j in range(4) if j != i]]
    else:
        (i, j), (k, l) = ins, outs
        q = [pair(i, k), pair(i, l), pair(j, l), pair(j, k)]
        tris = [[q[0], q[1], q[2]], [q[0], q[2], q[3]]]
    if tris:
        a = _tet_corners(PERMS[pi])
        mid = lambda e: (a[e[0]] + a[e[1]]) / 2.0

        def outward(t):
            p0, p1, p2 = mid(t[0]), mid(t[1]), mid(t[2])
            s = float(np.dot(np.cross(p1 - p0, p2 - p0), p0 - a[ins[0]]))
            assert s != 0.0
            return s > 0.0
        if not outward(tris[0]):
            if len(tris) == 1:
                t = tris[0]
                tris = [[t[0], t[2], t[1]]]
            else:
                tris = [[q[0], q[3], q[2]], [q[0], q[2], q[1]]]
        assert all(outward(t) for t in tris)
    _TRIS[key] = tris
    return tris


class RefMesh:
    def __init__(self, positions, gradients, triangles):
        self.positions, self.gradients, self.triangles = positions, gradients, triangles

    @property
    def counts(self):
        return len(self.positions), len(self.triangles)


def _corner_specs(pi, m):
    """tet_triangles(pi, m) with every edge (i, j) as (offset of a_i from the cell's low corner, type e)."""
    a = _tet_corners(PERMS[pi])
    out = []
    for t in tet_triangles(pi, m):
        row = []
        for (i, j) in t:
            d = a[j] - a[i]
            row.append((tuple(int(q) for q in a[i]), int(d[0] + 2 * d[1] + 4 * d[2] - 1)))
        out.append(row)
    return out


def mesh(vol, iso_value, cap=False, own_lo=None, own_hi=None, gradients=False):
    """The mesh of the cells own_lo <= c < own_hi (default: every cell) of the global volume `vol`: RefMesh of
    positions (V, 3) float32, gradients (V, 3) float32 or None, triangles (T, 3) uint32."""
    vol = np.asarray(vol)
    assert vol.dtype == np.uint8 and vol.ndim == 3
    G = vol.shape[::-1]
    clo, chi = cell_range(G, cap)
    lo = tuple(clo if own_lo is None else own_lo)
    hi = tuple(chi if own_hi is None else own_hi)
    assert all(clo[k] <= lo[k] <= hi[k] <= chi[k] for k in range(3))
    level = F(iso_value) * F(255.0)
    assert level.dtype == np.float32
    # v and v^ over the lattice and one point beyond, index q + 2: zeros around the volume (the cap's virtual layer; v^
    # zero-extended), or the edge values repeated (v^ clamped, without cap; v is then never read outside the volume)
    val = np.pad(vol.astype(np.int64), 2, mode="constant" if cap else "edge")
    ins = val.astype(np.float32) >= level
    v = lambda q: int(val[q[2] + 2, q[1] + 2, q[0] + 2])

    def grad(q):
        return [F(v(tuple(q[j] + (j == k) for j in range(3))) - v(tuple(q[j] - (j == k) for j in range(3)))) for k in range(3)]

    pos, grd, index, tris = [], [], {}, []
    if all(lo[k] < hi[k] for k in range(3)):
        box = ins[lo[2] + 2:hi[2] + 3, lo[1] + 2:hi[1] + 3, lo[0] + 2:hi[0] + 3]       # the closed point box
        nz, ny, nx = box.shape
        # vertices: the crossing edges with both ends in the point box, by owner point (x fastest), then type
        found = []
        for e in range(7):
            dx, dy, dz = (e + 1) & 1, ((e + 1) >> 1) & 1, (e + 1) >> 2
            cross = box[:nz - dz, :ny - dy, :nx - dx] != box[dz:, dy:, dx:]
            z, y, x = np.nonzero(cross)
            found.append(np.stack([z, y, x, np.full(len(z), e)], 1))
        found = np.concatenate(found)
        found = found[np.lexsort((found[:, 3], found[:, 2], found[:, 1], found[:, 0]))]
        for z, y, x, e in found.tolist():
            p = (lo[0] + x, lo[1] + y, lo[2] + z)
            d = ((e + 1) & 1, ((e + 1) >> 1) & 1, (e + 1) >> 2)
            q = tuple(p[k] + d[k] for k in range(3))
            va, vb = F(v(p)), F(v(q))
            t = (level - va) / (vb - va)
            index[p + (e,)] = len(pos)
            pos.append([F(p[k]) + (t if d[k] else F(0.0)) for k in range(3)])
            if gradients:
                ga, gb = grad(p), grad(q)
                grd.append([ga[k] + t * (gb[k] - ga[k]) for k in range(3)])
        # triangles: by cell (x fastest), tetrahedron, then the rule's order
        offs = [[tuple(int(q) for q in a) for a in _tet_corners(perm)] for perm in PERMS]
        for cz in range(lo[2], hi[2]):
            for cy in range(lo[1], hi[1]):
                for cx in range(lo[0], hi[0]):
                    cube = ins[cz + 2:cz + 4, cy + 2:cy + 4, cx + 2:cx + 4]
                    if cube.all() or not cube.any():
                        continue                               # every tetrahedron has four equal corners
                    for pi in range(6):
                        m = tuple(bool(cube[o[2], o[1], o[0]]) for o in offs[pi])
                        for t in _SPECS.get((pi, m)) or _SPECS.setdefault((pi, m), _corner_specs(pi, m)):
                            tris.append([index[(cx + o[0], cy + o[1], cz + o[2], e)] for o, e in t])
    P = np.array(pos, np.float32).reshape(-1, 3)
    Gd = np.array(grd, np.float32).reshape(-1, 3) if gradients else None
    return RefMesh(P, Gd, np.array(tris, np.uint32).reshape(-1, 3))


_SPECS = {}


# ---- combinatorial and metric properties -------------------------------------------------------------------------------
def directed_edges(tris):
    """{(a, b): how many triangles run a -> b}."""
    out = {}
    for t in np.asarray(tris).tolist():
        for k in range(3):
            e = (t[k], t[(k + 1) % 3])
            out[e] = out.get(e, 0) + 1
    return out


def undirected_edges(tris):
    out = {}
    for (a, b), n in directed_edges(tris).items():
        e = (min(a, b), max(a, b))
        out[e] = out.get(e, 0) + n
    return out


def is_closed(tris):
    """Every undirected edge in exactly two triangles, once in each direction."""
    de = directed_edges(tris)
    return all(n == 1 for n in de.values()) and all((b, a) in de for (a, b) in de)


def is_oriented(tris):
    """No directed edge used twice."""
    return all(n == 1 for n in directed_edges(tris).values())


def euler(num_vertices, tris):
    return num_vertices - len(undirected_edges(tris)) + len(tris)


def signed_volume(positions, tris):
    p = np.asarray(positions, np.float64)
    t = np.asarray(tris, np.int64)
    a, b, c = p[t[:, 0]], p[t[:, 1]], p[t[:, 2]]
    return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)


def triangle_soup(positions, tris):
    """(T, 9): the three corner positions of every triangle, in order."""
    return np.asarray(positions)[np.asarray(tris, np.int64).reshape(-1)].reshape(-1, 9)


def ball(n=12, radius=None):
    """A radial ramp: 255 at the centre of an n^3 volume falling linearly to 0 at `radius` (default n / 2 - 1)."""
    radius = n / 2.0 - 1.0 if radius is None else radius
    z, y, x = np.meshgrid(*[np.arange(n) - (n - 1) / 2.0] * 3, indexing="ij")
    r = np.sqrt(x * x + y * y + z * z)
    return np.clip(np.rint(255.0 * (1.0 - r / radius)), 0, 255).astype(np.uint8)
