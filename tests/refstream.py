"""Grammar-random tree streams and plain NumPy references of their decode.

No project code is imported here.  The definition these references restate:

  grammar   subtree := 3 | code subtree subtree   (depth < D)
                     | 3 | code branch            (depth D)          code in {0, 1, 2}
            branch  := up to seven codes, ended by a 3 unless all seven are present
            2-bit tokens, preorder, four per byte: element i in byte i / 4 at bits 2 (i & 3)
  splits    depth d splits axis d % 3 (x = 0), or the next axis (cyclically) whose extent is not 1; lower half first
  values    root = dmap[0]; a node at depth j <= cut applies its token to its parent's value: 1 adds dmap[j] (clamped
            to 255), 2 subtracts it (clamped to 0), 0 and 3 leave it; the c-th branch code below a leaf has depth D + c;
            a voxel takes the value of its terminal node's ancestor at depth min(cut, depth of the terminal); M = D + 7

gen_stream / gen_levels make streams family by family, level by level in heap order (no Python recursion: a 128^3
stream has up to 18.9 M tokens); decode_levels is the vectorised reference (every cut from one pass);
decode_recursive is the definition above written down as it reads, for small extents; write_file writes the
reference's file layout; census says what a stream contains.

General extents (any X, Y, Z; D = floor(log2 X) + floor(log2 Y) + floor(log2 Z)) keep the grammar and
the values and change the boxes: a box [lo, hi) of more than one cell is cut at (lo + hi) / 2, a box of one cell goes to
both children, and below a live leaf every branch node (the terminating 3 included) first halves the box like a left
child; only the terminal node's box is written, the cells that fell out stay 0, and a progressive cut stops the scalar
updates, never the halvings.  make_general makes such streams (a stream needs only D), decode_recursive_general is that
definition as it reads, Decoded.at of such a stream the vectorised reference (the per-rank values of decode_levels
through voxel_geometry and branch_nodes), census_general what the boxes make of a stream.
"""
import functools
import struct

import numpy as np

CHAIN = 7
FAMILIES = ("dense7", "dense0", "leafprune", "blockprune", "shallow", "root3", "root_children3", "mono_up", "mono_down",
            "zeros", "mixed")
LAWS = ("std", "sat", "zero", "chain_ns")
STD_CHAIN = tuple(64 >> i for i in range(CHAIN))


def log2i(n):
    k = int(n).bit_length() - 1
    if n < 1 or (1 << k) != n:
        raise ValueError("extent %r is not a power of two" % (n,))
    return k


def depth_of(dims):
    return sum(log2i(d) for d in dims)


def depth_general(dims):
    """D of any extents: floor(log2 X) + floor(log2 Y) + floor(log2 Z) (depth_of where every extent is a power of two)."""
    if min(int(d) for d in dims) < 1:
        raise ValueError("extents %r" % (tuple(dims),))
    return sum(int(d).bit_length() - 1 for d in dims)


def split_axes(dims):
    """[(axis, coordinate bit)] for depths 0 .. D-1 of a power-of-two box (every node of a depth splits alike)."""
    ext = [int(d) for d in dims]
    out = []
    for d in range(depth_of(dims)):
        a = d % 3
        while ext[a] == 1:
            a = (a + 1) % 3
        ext[a] //= 2
        out.append((a, log2i(ext[a])))
    return out


@functools.lru_cache(maxsize=8)
def rank_of_voxels(dims):
    """int64 [Z][Y][X], read-only: the leaf rank (D bits, depth 0 = most significant, lower half = 0) of every voxel."""
    X, Y, Z = dims
    D = depth_of(dims)
    coord = [np.arange(X, dtype=np.int64)[None, None, :], np.arange(Y, dtype=np.int64)[None, :, None],
             np.arange(Z, dtype=np.int64)[:, None, None]]
    r = np.zeros((Z, Y, X), np.int64)
    for d, (a, bit) in enumerate(split_axes(dims)):
        r = r | (((coord[a] >> bit) & 1) << (D - 1 - d))
    r.setflags(write=False)
    return r


def pack(tokens):
    """2-bit tokens -> bytes, element i in byte i / 4 at bits 2 (i & 3); the last byte is zero padded."""
    t = np.asarray(tokens, np.uint8)
    n = (t.size + 3) // 4
    p = np.zeros(n * 4, np.uint8)
    p[:t.size] = t
    p = p.reshape(n, 4)
    return (p[:, 0] | (p[:, 1] << 2) | (p[:, 2] << 4) | (p[:, 3] << 6)).astype(np.uint8)


def unpack(data, n):
    b = np.asarray(data, np.uint8)
    t = np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)
    return t[:n].copy()


def write_file(path, dims, tokens, dmap):
    """The reference's file: an 88-byte header (rootMin, rootMax as int64[3], maxDepth, origDepth as int32, X, Y, Z,
    numActive as int64), then dmap[0 .. M], then the packed tokens."""
    X, Y, Z = (int(d) for d in dims)
    D = depth_general(dims)
    dmap = np.asarray(dmap, np.uint8)
    assert dmap.size == D + CHAIN + 1
    with open(path, "wb") as f:
        f.write(struct.pack("<6q2i4q", 0, 0, 0, X, Y, Z, D + CHAIN, D, X, Y, Z, int(np.asarray(tokens).size)))
        f.write(dmap.tobytes())
        f.write(pack(tokens).tobytes())


# ---- distance maps ----

def gen_dmap(rng, D, law, family="mixed"):
    """dmap[0 .. D + 7] under one of LAWS.  The mono families take interior distances that sum to 200 .. 250 under
    `std` (the deepest leaves end just below the clamp, which their grown branches then reach) and start from the end
    of the range they move away from (dmap[0] = 0 going up, 255 going down)."""
    m = np.zeros(D + CHAIN + 1, np.int64)
    m[0] = rng.integers(0, 256)
    m[D + 1:] = STD_CHAIN
    if law == "std":
        m[1:D + 1] = rng.integers(1, 61, D)
        if family in ("mono_up", "mono_down") and D > 0:
            total = int(rng.integers(200, 251))
            m[1:D + 1] = total // D
            m[1 + rng.choice(D, total % D, replace=False)] += 1
    elif law == "sat":
        m[1:D + 1] = rng.choice([0, 1, 127, 128, 255], D)
    elif law == "zero":
        pass
    elif law == "chain_ns":
        m[1:D + 1] = rng.integers(1, 61, D)
        while tuple(m[D + 1:]) == STD_CHAIN:
            m[D + 1:] = rng.integers(0, 256, CHAIN)
    else:
        raise ValueError(law)
    if family == "mono_up":
        m[0] = 0
    if family == "mono_down":
        m[0] = 255
    return m.astype(np.uint8)


# ---- streams, level by level ----

class Levels:
    """A stream in heap order.  tok[d]: uint8 [2^d], the token of every node of depth d, 255 where the node does not
    exist (an ancestor was pruned).  chain_len: int8 [2^D], branch codes below each leaf (-1: the leaf is not live);
    chain_tok: uint8 [2^D][7], those codes (entries at and after chain_len unused).  A live leaf with fewer than seven
    codes is followed by a terminating 3.  general: the boxes are those of the general-extent walk (any X, Y, Z, with
    D = depth_general); the stream itself knows nothing of them."""

    def __init__(self, dims, tok, chain_len, chain_tok, dmap, general=False):
        self.dims = tuple(int(d) for d in dims)
        self.general = bool(general)
        self.D = depth_general(dims) if general else depth_of(dims)
        self.M = self.D + CHAIN
        self.tok, self.chain_len, self.chain_tok = tok, chain_len, chain_tok
        self.dmap = np.asarray(dmap, np.uint8)
        self._tokens = None

    @property
    def tokens(self):
        if self._tokens is None:
            self._tokens = assemble(self)
        return self._tokens


def _profile(family, D):
    """Prune probability per depth 0 .. D."""
    p = np.zeros(D + 1)
    if family == "leafprune":
        p[max(D - 3, 1):] = 0.25
    elif family == "blockprune":
        p[max(D - 12, 1):max(D - 5, 1)] = 0.5
    elif family == "shallow":
        p[1:max(D - 12, 1)] = 0.3
    elif family in ("mixed", "mono_up", "mono_down", "zeros"):
        p[2:] = 0.03
    return p


def gen_levels(rng, dims, family, law="std", dmap=None, general=False):
    if family not in FAMILIES:
        raise ValueError(family)
    D = depth_general(dims) if general else depth_of(dims)       # all a stream needs of the extents
    if dmap is None:
        dmap = gen_dmap(rng, D, law, family)
    prob = _profile(family, D)
    fixed = {"mono_up": 1, "mono_down": 2, "zeros": 0}.get(family)
    tok = []
    present = np.ones(1, bool)
    for d in range(D + 1):
        n = 1 << d
        codes = np.full(n, fixed, np.uint8) if fixed is not None else rng.integers(0, 3, n).astype(np.uint8)
        prune = (rng.random(n) < prob[d]) & present
        if prob[d] > 0 and present.sum() >= 2:
            idx = np.flatnonzero(present)
            if not prune.any():                  # every depth of a profile holds a prune ...
                prune[rng.choice(idx)] = True
            if prune[idx].all():                 # ... and a survivor
                prune[rng.choice(idx)] = False
        if family == "root3" and d == 0:
            prune[:] = True
        if family == "root_children3" and d == 1:
            prune[:] = True
        t = np.where(prune, 3, codes).astype(np.uint8)
        t[~present] = 255
        tok.append(t)
        present = np.repeat(present & ~prune, 2) if d < D else present & ~prune
    live = present
    nl = 1 << D
    if family == "dense7":
        length = np.full(nl, 7)
    elif family == "dense0":
        length = np.zeros(nl, np.int64)
    else:
        # all lengths 0 .. 7, and seven tokens both ways: six codes and a 3, seven codes and no terminator
        length = rng.choice(8, nl, p=[0.16, 0.12, 0.1, 0.1, 0.1, 0.1, 0.16, 0.16])
    chain_len = np.where(live, length, -1).astype(np.int8)
    chain_tok = np.full((nl, CHAIN), fixed, np.uint8) if fixed is not None else rng.integers(0, 3, (nl, CHAIN)).astype(np.uint8)
    return Levels(dims, tok, chain_len, chain_tok, dmap, general)


def assemble(lv):
    """Levels -> the preorder token array: subtree sizes bottom-up, token offsets top-down, one scatter."""
    D = lv.D
    cl = lv.chain_len.astype(np.int64)
    ctoks = np.where(cl >= 0, np.minimum(cl + 1, CHAIN), 0)           # chain tokens, terminator included
    size = [None] * (D + 1)
    size[D] = (lv.tok[D] != 255).astype(np.int64) + ctoks
    for d in range(D - 1, -1, -1):
        below = size[d + 1].reshape(-1, 2)
        size[d] = np.where(lv.tok[d] == 255, 0, 1 + below[:, 0] + below[:, 1])
    out = np.empty(int(size[0][0]), np.uint8)
    off = np.zeros(1, np.int64)
    for d in range(D + 1):
        here = lv.tok[d] != 255
        out[off[here]] = lv.tok[d][here]
        if d < D:
            nxt = np.empty(2 << d, np.int64)
            nxt[0::2] = off + 1
            nxt[1::2] = off + 1 + size[d + 1][0::2]
            off = nxt
    livei = np.flatnonzero(cl >= 0)
    n = ctoks[livei]
    start = np.repeat(off[livei] + 1, n)
    within = np.arange(int(n.sum()), dtype=np.int64) - np.repeat(np.cumsum(n) - n, n)
    leaf = np.repeat(livei, n)
    out[start + within] = np.where(within < cl[leaf], lv.chain_tok[leaf, np.minimum(within, CHAIN - 1)], 3)
    return out


def gen_stream(rng, dims, family, law="std"):
    """(tokens, dmap): one 2-bit token per element of `tokens` (pack() gives the bytes)."""
    lv = gen_levels(rng, dims, family, law)
    return lv.tokens, lv.dmap


# ---- the vectorised reference ----

def _apply(v, tok, dist):
    """v: int16 values; returns (new values, clamped at 255, clamped at 0)."""
    step = np.array([0, int(dist), -int(dist), 0], np.int16)     # per token; 255 (no node) reads as 3
    s = v + step[tok & 3]
    return np.clip(s, 0, 255), s > 255, s < 0


class Decoded:
    """Every cut of one stream.  val[j]: uint8, the value of every depth-min(j, D) position at cut j (pruned nodes
    carry their value down)."""

    def __init__(self, lv, val, clamps):
        self.lv, self.val, self.clamps = lv, val, clamps
        self._rank = None

    def leaves(self, cut=None):
        """uint8 [2^D]: the decode at `cut` (None: full depth) per leaf rank."""
        D, M = self.lv.D, self.lv.M
        cut = M if cut is None else int(cut)
        assert 0 <= cut <= M
        v = self.val[cut]
        return np.repeat(v, 1 << (D - cut)) if cut < D else v

    def at(self, cut=None):
        """uint8 [Z][Y][X]: the decode at `cut` (None: full depth).  General boxes: a voxel takes the value of the leaf
        that owns it where that leaf's grown branch has no more nodes than halvings the voxel survives, else 0; the
        boxes are those of the full walk whatever the cut."""
        if self.lv.general:
            g = voxel_geometry(tuple(self.lv.dims))
            kept = branch_nodes(self.lv)[g.owner] <= g.surv
            return np.where(kept, self.leaves(cut)[g.owner], 0).astype(np.uint8)
        if self._rank is None:
            self._rank = rank_of_voxels(tuple(self.lv.dims))
        return self.leaves(cut)[self._rank]


def decode_levels(lv):
    """One pass over the levels of `lv` (a Levels): the decode at every cut 0 .. M, and per leaf whether an addition
    on its path left [0, 255] (upwards / downwards, at interior depths 1 .. D / in the grown branch)."""
    D, dmap = lv.D, lv.dmap
    v = np.full(1, int(dmap[0]), np.int16)
    val = [v.astype(np.uint8)]
    hiI = np.zeros(1, bool)
    loI = np.zeros(1, bool)
    for d in range(1, D + 1):
        v, hi, lo = _apply(np.repeat(v, 2), lv.tok[d], dmap[d])
        hiI, loI = np.repeat(hiI, 2) | hi, np.repeat(loI, 2) | lo
        val.append(v.astype(np.uint8))
    hiC = np.zeros(1 << D, bool)
    loC = np.zeros(1 << D, bool)
    for c in range(1, CHAIN + 1):
        tok = np.where(lv.chain_len >= c, lv.chain_tok[:, c - 1], 3)
        v, hi, lo = _apply(v, tok, dmap[D + c])
        hiC, loC = hiC | hi, loC | lo
        val.append(v.astype(np.uint8))
    return Decoded(lv, val, dict(hi_interior=hiI, lo_interior=loI, hi_chain=hiC, lo_chain=loC))


# ---- general extents: the geometry, voxel by voxel and node by node ----

def _split_axis(ext, depth):
    """ext: int64 [3][n].  (axis [n], more [n]): the axis a box at `depth` is cut on -- depth % 3, advanced cyclically
    past axes of extent 1 -- and whether it holds more than one cell (only then is it cut)."""
    n = ext.shape[1]
    col = np.arange(n)
    more = ext[0] * ext[1] * ext[2] > 1
    a = np.full(n, depth % 3, np.int64)
    for i in (1, 2):
        a = np.where(more & (ext[a, col] == 1), (depth + i) % 3, a)
    return a, more


class VoxelGeometry:
    """owner: int64 [Z][Y][X], the rank of the last leaf in preorder whose box of the full walk holds the voxel;
    surv: int64 [Z][Y][X], how many halvings of that leaf's box along its grown branch the voxel survives (255: all
    seven); single_at: int64 [Z][Y][X], the depth at which the voxel's box first held one cell (D: not above the
    leaves)."""

    def __init__(self, owner, surv, single_at):
        self.owner, self.surv, self.single_at = owner, surv, single_at
        for a in (owner, surv, single_at):
            a.setflags(write=False)


@functools.lru_cache(maxsize=16)
def voxel_geometry(dims):
    """The box rules followed down from the root by every voxel at once: a box of several cells is cut at
    (lo + hi) / 2 and the voxel goes to its side; a box of one cell goes to both children, of which the later one (bit
    1) writes last; below depth D every branch node halves the box like a left child, and a voxel in the upper half is
    dropped at that node."""
    X, Y, Z = (int(d) for d in dims)
    D = depth_general(dims)
    V = X * Y * Z
    v = np.arange(V, dtype=np.int64)
    c = np.stack([v % X, (v // X) % Y, v // (X * Y)])
    col = np.arange(V)
    lo = np.zeros((3, V), np.int64)
    hi = np.repeat(np.array([[X], [Y], [Z]], np.int64), V, axis=1)
    r = np.zeros(V, np.int64)
    single_at = np.full(V, D, np.int64)
    for d in range(D):
        a, more = _split_axis(hi - lo, d)
        single_at = np.where(~more & (single_at == D), d, single_at)
        mid = (lo[a, col] + hi[a, col]) // 2
        up = more & (c[a, col] >= mid)
        down = more & ~up
        lo[a[up], col[up]] = mid[up]
        hi[a[down], col[down]] = mid[down]
        r = (r << 1) | np.where(more, up, True)
    surv = np.full(V, 255, np.int64)
    alive = np.ones(V, bool)
    for j in range(CHAIN):
        a, more = _split_axis(hi - lo, D + j)
        alive = alive & more                       # one cell left: the voxel's own, at every further node
        mid = (lo[a, col] + hi[a, col]) // 2
        drop = alive & (c[a, col] >= mid)
        surv[drop] = j                             # the (j + 1)-th halving drops the voxel
        alive = alive & ~drop
        hi[a[alive], col[alive]] = mid[alive]
    shape = (Z, Y, X)
    return VoxelGeometry(r.reshape(shape), surv.reshape(shape), single_at.reshape(shape))


def branch_nodes(lv):
    """int64 [2^D]: the nodes of the grown branch below every leaf rank -- its codes and the terminating 3, seven
    without one -- and 0 where the leaf or an ancestor is pruned (the pruned node writes its whole box)."""
    cl = lv.chain_len.astype(np.int64)
    return np.where(cl >= 0, np.minimum(cl + 1, CHAIN), 0)


@functools.lru_cache(maxsize=16)
def node_boxes(dims):
    """Per depth 0 .. D, in heap order: (lo, hi, cuts), each int64 [3][2^d] -- every node's box [lo, hi) and how often
    the path to it cut each axis.  Children 2 i and 2 i + 1 are the lower and upper half; a box of one cell is handed to
    both."""
    D = depth_general(dims)
    lo = np.zeros((3, 1), np.int64)
    hi = np.array([[int(d)] for d in dims], np.int64)
    cuts = np.zeros((3, 1), np.int64)
    out = [(lo, hi, cuts)]
    for d in range(D):
        n = 1 << d
        col = np.arange(n)
        a, more = _split_axis(hi - lo, d)
        mid = (lo[a, col] + hi[a, col]) // 2
        lo2, hi2, cuts2 = (np.repeat(t, 2, axis=1) for t in (lo, hi, cuts))
        hi2[a[more], 2 * col[more]] = mid[more]
        lo2[a[more], 2 * col[more] + 1] = mid[more]
        cuts2[a[more], 2 * col[more]] += 1
        cuts2[a[more], 2 * col[more] + 1] += 1
        lo, hi, cuts = lo2, hi2, cuts2
        out.append((lo, hi, cuts))
    for t in out:
        for arr in t:
            arr.setflags(write=False)
    return out


# ---- the definition, as it reads ----

def decode_recursive(dims, tokens, dmap, cut=None):
    """The plain recursive walker over the flat token array: uint8 [Z][Y][X].  Raises ValueError on a stream the
    grammar does not produce (it ends early, or tokens are left over)."""
    import sys
    X, Y, Z = (int(d) for d in dims)
    D = depth_of(dims)
    cut = D + CHAIN if cut is None else int(cut)
    tokens = [int(t) for t in np.asarray(tokens).reshape(-1)]
    dmap = [int(t) for t in dmap]
    out = np.zeros((Z, Y, X), np.uint8)
    pos = [0]

    def step(v, tok, j):
        if j > cut or j == 0:
            return v
        if tok == 1:
            return min(v + dmap[j], 255)
        if tok == 2:
            return max(v - dmap[j], 0)
        return v

    def take():
        if pos[0] >= len(tokens):
            raise ValueError("the stream ends early")
        pos[0] += 1
        return tokens[pos[0] - 1]

    def node(lo, ext, j, parent):
        tok = take()
        v = step(parent, tok, j)
        if tok != 3 and j < D:
            a = j % 3
            while ext[a] == 1:
                a = (a + 1) % 3
            half = list(ext)
            half[a] //= 2
            hi = list(lo)
            hi[a] += half[a]
            node(lo, half, j + 1, v)
            node(hi, half, j + 1, v)
            return
        if tok != 3:
            for c in range(1, CHAIN + 1):
                t = take()
                if t == 3:
                    break
                v = step(v, t, D + c)
        out[lo[2]:lo[2] + ext[2], lo[1]:lo[1] + ext[1], lo[0]:lo[0] + ext[0]] = v

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 200 + 4 * D))
    try:
        node([0, 0, 0], [X, Y, Z], 0, dmap[0])
    finally:
        sys.setrecursionlimit(old)
    if pos[0] != len(tokens):
        raise ValueError("tokens left over")
    return out


def decode_recursive_general(dims, tokens, dmap, cut=None, writes=None):
    """The same walker over boxes [lo, hi) of any extents, D = depth_general(dims): uint8 [Z][Y][X].  A box of more
    than one cell is cut at (lo + hi) / 2 on axis depth % 3, advanced cyclically past axes of extent 1; a box of one
    cell goes to both children unsplit (the later leaf wins); below a live leaf every branch node, the terminating 3
    included, first halves the box like a left child, and only the terminal node's box is written: the cells that fell
    out stay 0.  A cut stops the scalar updates, never the halvings.  writes (a list): every write as (lo, hi, value),
    in order.  Raises ValueError on a stream the grammar does not produce."""
    import sys
    X, Y, Z = (int(d) for d in dims)
    D = depth_general(dims)
    cut = D + CHAIN if cut is None else int(cut)
    tokens = [int(t) for t in np.asarray(tokens).reshape(-1)]
    dmap = [int(t) for t in dmap]
    out = np.zeros((Z, Y, X), np.uint8)
    pos = [0]

    def step(v, tok, j):
        if j > cut or j == 0:
            return v
        if tok == 1:
            return min(v + dmap[j], 255)
        if tok == 2:
            return max(v - dmap[j], 0)
        return v

    def take():
        if pos[0] >= len(tokens):
            raise ValueError("the stream ends early")
        pos[0] += 1
        return tokens[pos[0] - 1]

    def axis(lo, hi, depth):
        ext = [hi[k] - lo[k] for k in range(3)]
        if ext[0] * ext[1] * ext[2] <= 1:
            return None
        a, i = depth % 3, 0
        while ext[a] == 1:
            i += 1
            a = (depth + i) % 3
        return a

    def write(lo, hi, v):
        out[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] = v
        if writes is not None:
            writes.append((tuple(lo), tuple(hi), v))

    def node(lo, hi, j, parent):
        tok = take()
        v = step(parent, tok, j)
        if tok == 3:
            write(lo, hi, v)
            return
        if j < D:
            a = axis(lo, hi, j)
            if a is None:
                node(lo, hi, j + 1, v)
                node(lo, hi, j + 1, v)
                return
            mid = (lo[a] + hi[a]) // 2
            left_hi, right_lo = list(hi), list(lo)
            left_hi[a] = right_lo[a] = mid
            node(lo, left_hi, j + 1, v)
            node(right_lo, hi, j + 1, v)
            return
        hi = list(hi)
        for c in range(1, CHAIN + 1):
            a = axis(lo, hi, D + c - 1)
            if a is not None:
                hi[a] = (lo[a] + hi[a]) // 2
            t = take()
            if t == 3:
                break
            v = step(v, t, D + c)
        write(lo, hi, v)

    old = sys.getrecursionlimit()
    sys.setrecursionlimit(max(old, 200 + 4 * D))
    try:
        node([0, 0, 0], [X, Y, Z], 0, dmap[0])
    finally:
        sys.setrecursionlimit(old)
    if pos[0] != len(tokens):
        raise ValueError("tokens left over")
    return out


# ---- what a stream contains ----

def census(lv, dec=None):
    """prunes[d]: pruned nodes at depth d; chain_codes[k]: live leaves with k branch codes; seven_with_3 /
    seven_without_3: grown branches of seven tokens ending in a 3 / of seven codes; block_tokens: tokens of every
    4096-leaf block (a depth-(D-12) subtree; 0: its root does not exist), when D >= 12; regions_dead /
    regions_alternating: 128 x 16 x 16 regions whose eight 16^3 blocks are all dead / change between live and dead at
    least twice along x (a dead block: its depth-(D-12) root is pruned or does not exist), when the extents hold whole
    regions; with `dec` (decode_levels of lv) the clamp fractions and counts."""
    D = lv.D
    c = {"tokens": int(lv.tokens.size), "prunes": [int((t == 3).sum()) for t in lv.tok],
         "chain_codes": [int((lv.chain_len == k).sum()) for k in range(CHAIN + 1)]}
    c["seven_with_3"] = c["chain_codes"][6]
    c["seven_without_3"] = c["chain_codes"][7]
    X, Y, Z = lv.dims
    if D >= 12:
        cl = lv.chain_len.astype(np.int64)
        size = (lv.tok[D] != 255).astype(np.int64) + np.where(cl >= 0, np.minimum(cl + 1, CHAIN), 0)
        for d in range(D - 1, D - 13, -1):
            size = np.where(lv.tok[d] == 255, 0, 1 + size[0::2] + size[1::2])
        c["block_tokens"] = size
        if not lv.general and X >= 128 and Y >= 16 and Z >= 16 and _blocks_are_cubes(lv.dims):
            t = lv.tok[D - 12]
            dead = (t == 255) | (t == 3)
            rank = rank_of_voxels(tuple(lv.dims))[::16, ::16, ::16] >> 12
            grid = dead[rank].reshape(Z // 16, Y // 16, X // 128, 8)
            c["regions_dead"] = int(grid.all(axis=3).sum())
            c["regions_alternating"] = int(((grid[..., 1:] != grid[..., :-1]).sum(axis=3) >= 2).sum())
    if dec is not None:
        n = float(1 << D)
        k = dec.clamps
        c["clamp_hi_fraction"] = float((k["hi_interior"] | k["hi_chain"]).sum()) / n
        c["clamp_lo_fraction"] = float((k["lo_interior"] | k["lo_chain"]).sum()) / n
        for name, a in k.items():
            c["clamp_" + name] = int(a.sum())
    return c


def census_general(lv, dec, cut=None):
    """What the general boxes make of a stream, at one cut of its decode (None: full depth).  dropped: voxels left 0
    because a halving along their owner's grown branch dropped them (a count of the geometry and the branch lengths:
    the same at every cut); kept_at_edge / dropped_at_edge: voxels whose owner's branch has exactly as many nodes as
    halvings they survive (written) / one more (0); multi_writer_cells: cells whose box held one cell above depth D, so that every leaf below
    that node writes them; overwritten_differently: those of them where some earlier writer's value is not the last
    one's; pruned_multicell_off_grid: pruned nodes (depth 0 .. D) whose box has several cells and, on some axis cut n
    times on the way, another extent than X >> n -- boxes no power-of-two brick holds."""
    D = lv.D
    g = voxel_geometry(lv.dims)
    nb = branch_nodes(lv)[g.owner]
    out = {"voxels": int(g.owner.size), "dropped": int((nb > g.surv).sum()),
           "kept_at_edge": int((nb == g.surv).sum()), "dropped_at_edge": int((nb == g.surv + 1).sum())}
    multi = g.single_at < D
    out["multi_writer_cells"] = int(multi.sum())
    vals = dec.leaves(cut)
    differs = 0
    for d in np.unique(g.single_at[multi]):
        below = vals.reshape(-1, 1 << (D - int(d)))            # the ranks below every depth-d node, in write order
        changed = (below != below[:, -1:]).any(axis=1)
        differs += int(changed[g.owner[multi & (g.single_at == d)] >> (D - int(d))].sum())
    out["overwritten_differently"] = differs
    dims = np.array(lv.dims, np.int64)[:, None]
    n = 0
    for d, (lo, hi, cuts) in enumerate(node_boxes(lv.dims)):
        ext = hi - lo
        n += int(((lv.tok[d] == 3) & (ext.prod(axis=0) > 1) & (ext != (dims >> cuts)).any(axis=0)).sum())
    out["pruned_multicell_off_grid"] = n
    return out


def _blocks_are_cubes(dims):
    """The twelve deepest levels split every axis four times: a depth-(D-12) subtree is a 16^3 box."""
    ax = [a for a, _ in split_axes(dims)[-12:]]
    return len(ax) == 12 and all(ax.count(k) == 4 for k in range(3))


# ---- the streams the test modules share ----

# streams whose name alone seeds a draw that misses a census condition of tests/test_stream_grammar_cpu.py
SALT = {((128, 128, 64), "shallow", "sat"): 20}


def make(dims, family, law="std"):
    """The stream of (dims, family, law) that both test modules use: seeded by its own name, so the census conditions
    asserted on the CPU describe the very streams the GPU decodes."""
    import zlib
    key = (tuple(int(d) for d in dims), family, law)
    seed = zlib.crc32(repr(key + ((SALT[key],) if key in SALT else ())).encode())
    return gen_levels(np.random.default_rng(seed), dims, family, law)


# the same for make_general and the census conditions of tests/test_stream_grammar_general_cpu.py
SALT_GENERAL = {}                                                   # (no draw misses one so far)


def make_general(dims, family, law="std"):
    """The stream of (general dims, family, law) that tests/test_stream_grammar_general_cpu.py and
    tests/test_gpu_foreign_general.py share: D = depth_general(dims), boxes of the general walk.  Seeded by its own
    name, apart from make's (a power-of-two extent on the general path, 2048 x 2 x 2, is another stream here)."""
    import zlib
    key = ("general", tuple(int(d) for d in dims), family, law)
    seed = zlib.crc32(repr(key + ((SALT_GENERAL[key],) if key in SALT_GENERAL else ())).encode())
    return gen_levels(np.random.default_rng(seed), dims, family, law, general=True)
