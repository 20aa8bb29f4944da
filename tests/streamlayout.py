"""The block layout of a contiguous tree stream, read off the stream alone, and the census of the paths of k_concat12
that such a layout takes.  Plain NumPy / Python: no project code is imported here.

The stream is the preorder 2-bit stream of tests/refstream.py (a node is `3`, or a code and two subtrees; at depth D a
code and a branch of up to seven codes ended by a `3`).  k_concat12 assembles it from pieces: every depth-(D-12) block b
(4096 leaves) contributes the tokens of depth < D-12 whose leftmost block it is (its spine: a pruned ancestor's `3`
counts for the block that holds its first leaf) and then the tokens at depth >= D-12 under its root (its string), if that
root exists.  `layout` finds those pieces again by parsing; `classes` sorts blocks and workgroups of 16 blocks into the
cases the kernel tells apart (at most 32 tokens: one lane; 16 tokens per word, 4 words per 16-byte chunk, 256 * 4 chunks
per trip), so that a test can say which of them its inputs reach and which one owns a differing byte.
"""
import numpy as np

SUB = 12                    # log2 of the leaves per block
CHAIN = 7                   # longest branch below a leaf
MAX_CNT = 36863             # 4095 + 4096 * (1 + CHAIN): tokens of a block in which nothing is pruned and every branch is full
WG_BLOCKS = 16              # blocks per workgroup
TRIP_CHUNKS = 256 * 4       # 16-byte chunks per workgroup and trip

MANDATORY = ("S1", "S2", "S3", "S4", "S5", "S6", "S7", "L2", "L3_w0_0", "L3_w0_1", "L3_w0_2", "L3_w0_3", "L3_wl_0",
             "L3_wl_1", "L3_wl_2", "L3_wl_3", "L4", "L5", "L6", "L7", "L8", "W1", "W2", "W3", "W4_first", "W4_last", "W5",
             "W6", "W7", "W8_nblk1", "W8_nblk4")
OPTIONAL = ("S8", "L1")


def _unpack(data, n):
    b = np.asarray(data, np.uint8).reshape(-1)
    if 4 * b.size < n:
        raise ValueError("%d tokens do not fit %d bytes" % (n, b.size))
    return np.stack([(b >> s) & 3 for s in (0, 2, 4, 6)], axis=1).reshape(-1)[:n]


def layout(tree_bytes, num_tokens, D):
    """dict of int64 [2^(D-12)] arrays g0, nsp, cnt, tot, w0, wl (w0, wl mean something where tot > 0).  g0 is the
    position of the first token the block owns as the parse meets it; a block that owns none gets the position of the
    next owned token (the token count behind the last).  Raises ValueError on a stream the grammar does not produce."""
    D, n = int(D), int(num_tokens)
    if D < SUB:
        raise ValueError("no 4096-leaf block in a tree of depth %d" % D)
    tok = _unpack(tree_bytes, n)
    three = np.flatnonzero(tok == 3)
    nxt3 = np.append(three, n)[np.searchsorted(three, np.arange(n + 1))].tolist()    # first 3 at or behind a position
    t = tok.tolist()
    db = D - SUB
    nb = 1 << db
    first, nsp, cnt = [-1] * nb, [0] * nb, [0] * nb
    pos = 0
    stack = [(0, 0)]                                    # (depth, rank within the depth), depth <= db
    while stack:
        d, r = stack.pop()
        if pos >= n:
            raise ValueError("the stream ends early")
        b = r << (db - d)
        if first[b] < 0:
            first[b] = pos
        if d < db:
            nsp[b] += 1
            if t[pos] != 3:
                stack.append((d + 1, 2 * r + 1))
                stack.append((d + 1, 2 * r))
            pos += 1
            continue
        start = pos
        below = [0]                                     # the block's own subtree: levels below its root
        while below:
            k = below.pop()
            if pos >= n:
                raise ValueError("the stream ends early")
            c = t[pos]
            pos += 1
            if c == 3:
                continue
            if k < SUB:
                below.append(k + 1)
                below.append(k + 1)
            else:
                codes = nxt3[pos] - pos
                pos += CHAIN if codes >= CHAIN else codes + 1
                if pos > n:
                    raise ValueError("the stream ends early")
        cnt[b] = pos - start
    if pos != n:
        raise ValueError("tokens left over: %d of %d parsed" % (pos, n))
    g0 = np.array(first, np.int64)
    nxt = n
    for b in range(nb - 1, -1, -1):
        if g0[b] < 0:
            g0[b] = nxt
        nxt = g0[b]
    nsp, cnt = np.array(nsp, np.int64), np.array(cnt, np.int64)
    tot = nsp + cnt
    return dict(g0=g0, nsp=nsp, cnt=cnt, tot=tot, w0=g0 >> 4, wl=(g0 + tot - 1) >> 4)


def _chunks(w0, wl):
    """16-byte destination chunks of a long block: the kernel's count, from the aligned word at or before w0"""
    return (wl - (w0 & ~3)) // 4 + 1


def block_classes(lay, b):
    """names of the block-level classes of block b (empty list: the block owns no token)"""
    g0, nsp, cnt, tot, w0, wl = (int(lay[k][b]) for k in ("g0", "nsp", "cnt", "tot", "w0", "wl"))
    out = []
    if tot == 0:
        return out
    if tot <= 32:
        out.append("S%d" % (wl - w0 + 1))
        if 1 <= cnt <= 16:
            out.append("S4")
        if 17 <= cnt <= 32:
            out.append("S5")
        if nsp >= 1 and cnt == 0:
            out.append("S6")
        if nsp >= 1 and cnt >= 1:
            out.append("S7")
        if tot == 32:
            out.append("S8")
        return out
    if tot == 33:
        out.append("L1")
    wA = w0 & ~3
    if not any(wA + 4 * q > w0 and wA + 4 * q + 3 < wl for q in range(_chunks(w0, wl))):
        out.append("L2")
    out += ["L3_w0_%d" % (w0 & 3), "L3_wl_%d" % (wl & 3)]
    if nsp >= 1 and (g0 & 15) + nsp > 16:
        out.append("L4")
    if nsp >= 1 and g0 & 15:
        out.append("L5")
    out.append("L6" if cnt % 16 == 0 else "L7")
    if cnt == MAX_CNT:
        out.append("L8")
    return out


def classes(lay):
    """The census: how many blocks (S*, L*), workgroups (W1 .. W6, W8_*) or destination words (W7) of the layout fall in
    each class.  Every name of MANDATORY and OPTIONAL is a key.

    S1 S2 S3: short blocks (1 <= tot <= 32) over one, two, three words; S4: 1 <= cnt <= 16; S5: 17 <= cnt <= 32 (the
    second source word); S6: spine only; S7: spine and string; S8: tot = 32.  L1: tot = 33; L2: no chunk of the block
    is stored whole; L3_w0_k / L3_wl_k: first / last word at k mod 4; L4: the spine's bits land in two words; L5: a
    spine that does not start a word; L6 / L7: the string ends with / inside a word; L8: the longest string.
    W1 / W2: the first live block of a workgroup behind a busy one starts inside / at the start of a word; W3: an
    empty workgroup behind a busy one; W4_first: a full workgroup whose only block with a token is its first;
    W4_last: a full workgroup whose only long block is its last (a workgroup whose only *live* block is its last does
    not exist: the workgroup's root belongs to its first block, and a node's sibling always has a token); W5: more
    chunks than one trip takes; W6: 16 blocks of the longest string; W7: words that get bits from three or more
    blocks of a workgroup; W8_nblk1 / W8_nblk4: a brick of one / four blocks (a partial workgroup)."""
    c = dict.fromkeys(MANDATORY + OPTIONAL, 0)
    nb = lay["tot"].size
    for b in range(nb):
        for name in block_classes(lay, b):
            c[name] += 1
    g0, cnt, tot, w0, wl = (lay[k] for k in ("g0", "cnt", "tot", "w0", "wl"))
    prev_busy = False
    for k in range(0, nb, WG_BLOCKS):
        sl = slice(k, min(k + WG_BLOCKS, nb))
        live = np.flatnonzero(tot[sl] > 0)
        full = sl.stop - sl.start == WG_BLOCKS
        if k and prev_busy and live.size:
            c["W1" if g0[k + live[0]] & 15 else "W2"] += 1
        if k and prev_busy and not live.size:
            c["W3"] += 1
        if full and live.size == 1 and live[0] == 0:
            c["W4_first"] += 1
        long_ = tot[sl] > 32
        if full and int(long_.sum()) == 1 and long_[WG_BLOCKS - 1]:
            c["W4_last"] += 1
        if int(_chunks(w0[sl][long_], wl[sl][long_]).sum()) > TRIP_CHUNKS:
            c["W5"] += 1
        if full and (cnt[sl] == MAX_CNT).all():
            c["W6"] += 1
        lw0, lwl = w0[sl][live], wl[sl][live]
        for w in np.unique(np.concatenate([lw0, lwl])):
            if int(((lw0 <= w) & (w <= lwl)).sum()) >= 3:
                c["W7"] += 1
        prev_busy = bool(live.size)
    if nb in (1, 4):
        c["W8_nblk%d" % nb] += 1
    return c


def add(a, b):
    return {k: a[k] + b[k] for k in a}


def describe(lay, got, want):
    """One line about the first byte at which `got` differs from `want`: the byte, its word, the block that owns it and
    that block's classes -- what a failing comparison prints."""
    got, want = np.asarray(got, np.uint8).reshape(-1), np.asarray(want, np.uint8).reshape(-1)
    if got.size != want.size:
        return "lengths differ: %d bytes for %d" % (got.size, want.size)
    bad = np.flatnonzero(got != want)
    if not bad.size:
        return "equal"
    i = int(bad[0])
    # the first differing token of that byte
    x = int(got[i]) ^ int(want[i])
    tk = 4 * i + next(s for s in range(4) if (x >> (2 * s)) & 3)
    hit = np.flatnonzero((lay["tot"] > 0) & (lay["g0"] <= tk) & (tk < lay["g0"] + lay["tot"]))
    b = int(hit[0]) if hit.size else -1
    line = "%d bytes differ, the first at byte %d (word %d, token %d): 0x%02x for 0x%02x" % (bad.size, i, i >> 2, tk, got[i], want[i])
    if b < 0:
        return line + "; no block owns that token"
    return line + "; block %d (workgroup %d) g0 %d nsp %d cnt %d w0 %d wl %d, token %d of its %d, classes %s" % (
        b, b // WG_BLOCKS, lay["g0"][b], lay["nsp"][b], lay["cnt"][b], lay["w0"][b], lay["wl"][b], tk - lay["g0"][b],
        lay["tot"][b], " ".join(block_classes(lay, b)))
