"""The decode kernels on grammar-random foreign streams: vr_brickset_set_tree / vr_brickset_open accept any stream of
the grammar of SURVEY.md Appendix A.4 with any distance map, not only what an encoder emits.  Streams and references
come from tests/refstream.py (plain NumPy; tests/test_stream_grammar_cpu.py pins them to the oracle and asserts what
the streams contain).  Everything is bit-exact against decode_levels: no tolerance, no masked voxel."""
import json
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402

pytestmark = pytest.mark.gpu

VR_ERR_FORMAT = -6
POISON = 0xA5
SWITCHES = ("decode_quad", "decode_fine_v1", "decode_walk")
BIG = ("dense7", "blockprune", "mixed")


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _tiled_extents():
    """The smallest extents with a tile and a region plan for each place of x in the deepest triple of split levels
    (tests/golden/decode_plans.json: [X, Y, Z, tile, region, ...], tile = [ok, jx, ...])."""
    plans = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "decode_plans.json")))["plans"]
    out = {}
    for p in plans:
        if p[3][0] and p[4][0]:
            jx = p[3][1]
            if jx not in out or p[0] * p[1] * p[2] < np.prod(out[jx]):
                out[jx] = tuple(p[:3])
    return sorted(out.values(), key=lambda d: d[0] * d[1] * d[2])


TILED = _tiled_extents()
SMALL = [(128, 8, 4), (16, 8, 4), (4, 1, 2)]      # k_decode_lane with K = 6 (two of them), and D < 6


def test_tiled_extents_are_the_expected_three():
    assert TILED == [(128, 64, 64), (128, 128, 64), (128, 128, 128)]


def cut_list(D, M, cuts):
    return sorted({c for c in cuts if 0 <= c <= M}, reverse=True)


def main_cuts(D, M):
    return [None] + cut_list(D, M, [M - 1, D + 4, D + 1, D, D - 1, D - 2, D - 3, D - 4, D - 6, D - 7, 3, 0])


def install(vr, lv, bricks=1, brick=0, bs=None):
    if bs is None:
        bs = vr.BrickSet(bricks, lv.dims)
    bs.set_tree(brick, R.pack(lv.tokens), lv.tokens.size, lv.dmap)
    return bs


def decode(bs, cut):
    X, Y, Z = bs.dims
    out = bs.decode() if cut is None else bs.decode(cut_depth=cut)
    return out.cpu().numpy().reshape(bs.num_bricks, Z, Y, X)


def check_switches(bs, decs, cuts, tag):
    """Default, each switch in turn, default again: every decode equals the reference, and the last default decode is
    the first one's bytes.  decs: one Decoded per brick."""
    want = {c: np.stack([d.at(c) for d in decs]) for c in cuts}
    first = {c: decode(bs, c) for c in cuts}
    for c in cuts:
        assert np.array_equal(first[c], want[c]), (tag, "default", c)
    for name in SWITCHES:
        bs.set_switch(name, 1)
        got = {c: decode(bs, c) for c in cuts}
        bs.set_switch(name, 0)
        for c in cuts:
            assert np.array_equal(got[c], want[c]), (tag, name, c)
    for c in cuts:
        assert decode(bs, c).tobytes() == first[c].tobytes(), (tag, "default again", c)


def _ids(d):
    return "%dx%dx%d" % d


# ---- a. per kernel, per family ----

@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("dims", TILED[:2], ids=_ids)
def test_families_on_tiled_extents(vr, dims, family):
    for law in ("std", "sat"):
        lv = R.make(dims, family, law)
        check_switches(install(vr, lv), [R.decode_levels(lv)], main_cuts(lv.D, lv.M), (family, law))


@pytest.mark.parametrize("law", ["std", "sat"])
@pytest.mark.parametrize("family", BIG)
def test_families_on_128_cubed(vr, family, law):
    lv = R.make(TILED[2], family, law)
    check_switches(install(vr, lv), [R.decode_levels(lv)], main_cuts(lv.D, lv.M), (family, law))


@pytest.mark.parametrize("dims", SMALL, ids=_ids)
def test_families_on_small_extents(vr, dims):
    for family in R.FAMILIES:
        for law in ("std", "sat"):
            lv = R.make(dims, family, law)
            check_switches(install(vr, lv), [R.decode_levels(lv)], main_cuts(lv.D, lv.M), (family, law))


# ---- b. grown-branch distances other than 64 >> i ----

def test_non_standard_chain_distances(vr):
    """A stream whose map holds other grown-branch distances decodes by that map (the chain table of the region and quad
    kernels holds the constants 64 >> i, so vr_brickset_set_tree keeps such a brick away from them): alone under every switch and cut,
    and in a set beside standard bricks; reinstalling a brick flips its flag either way, and a shorter stream leaves
    nothing of the longer one behind."""
    dims = TILED[0]
    ns = R.make(dims, "mixed", "chain_ns")
    D, M = ns.D, ns.M
    assert tuple(ns.dmap[D + 1:]) != R.STD_CHAIN
    dec_ns = R.decode_levels(ns)
    std_map = ns.dmap.copy()
    std_map[D + 1:] = R.STD_CHAIN
    same_tokens_std = R.decode_levels(R.Levels(dims, ns.tok, ns.chain_len, ns.chain_tok, std_map))
    assert any((dec_ns.leaves(c) != same_tokens_std.leaves(c)).any() for c in range(D + 1, M + 1))
    assert np.array_equal(dec_ns.leaves(D), same_tokens_std.leaves(D))
    check_switches(install(vr, ns), [dec_ns], [None] + list(range(M, -1, -1)), "chain_ns")

    cuts = [None, D + 2, D - 3, D - 7]
    lvs = [R.make(dims, "leafprune", "std"), ns, R.make(dims, "dense7", "std")]
    bs = vr.BrickSet(3, dims)
    for b, lv in enumerate(lvs):
        install(vr, lv, brick=b, bs=bs)
    check_switches(bs, [R.decode_levels(lv) for lv in lvs], cuts, "std, chain_ns, std")
    # brick 1 again, with a standard stream shorter than the one it replaces
    lvs[1] = R.make(dims, "blockprune", "std")
    assert lvs[1].tokens.size < ns.tokens.size // 4
    install(vr, lvs[1], brick=1, bs=bs)
    assert bs.info(1)["num_active_nodes"] == lvs[1].tokens.size
    assert np.array_equal(bs.tree(1), R.pack(lvs[1].tokens))
    check_switches(bs, [R.decode_levels(lv) for lv in lvs], cuts, "std, std, std")
    # brick 0 with other distances (a longer stream than the one it replaces)
    lvs[0] = R.make(dims, "dense7", "chain_ns")
    install(vr, lvs[0], brick=0, bs=bs)
    check_switches(bs, [R.decode_levels(lv) for lv in lvs], cuts, "chain_ns, std, std")


# ---- c. per-brick cuts, a brick never installed ----

def test_per_brick_cuts_with_a_brick_never_installed(vr):
    import torch
    from volumerenderer_amd.render import POOL_ENTRY
    dims = TILED[0]
    X, Y, Z = dims
    fams = ["dense7", "blockprune", "leafprune", None, "mono_up"]
    lvs = [None if f is None else R.make(dims, f, "sat" if b == 1 else "std") for b, f in enumerate(fams)]
    bs = vr.BrickSet(5, dims)
    for b, lv in enumerate(lvs):
        if lv is not None:
            install(vr, lv, brick=b, bs=bs)
    decs = [None if lv is None else R.decode_levels(lv) for lv in lvs]
    D, M = lvs[0].D, lvs[0].M
    pool_cuts = [-1, 0, D - 7, D - 3, D + 2, M]
    plans = [[pool_cuts[(r + b) % len(pool_cuts)] for b in range(5)] for r in range(len(pool_cuts))]
    plans.append([M, D - 3, D + 2, -1, D - 7])
    ijk, grid = np.array([(b, 0, 0) for b in range(5)], np.int64), (5, 1, 1)
    for cuts in plans:
        cuts = np.array(cuts, np.int32)
        cuts[3] = -1
        out = torch.full((5 * X * Y * Z,), POISON, dtype=torch.uint8, device="cuda")
        bs.decode_lod(cuts, out=out)
        got = out.cpu().numpy().reshape(5, Z, Y, X)
        for b, c in enumerate(cuts):
            if c < 0:
                assert np.all(got[b] == POISON), (list(cuts), b)
            else:
                assert np.array_equal(got[b], decs[b].at(int(c))), (list(cuts), b)
        # the same cuts into a pool that stores each brick at the resolution of its cut (the layout's rule)
        want_t, nbytes = vr.lod_pool_layout(dims, ijk, grid, cuts, D, M)
        pool = torch.full((nbytes + 4096,), POISON, dtype=torch.uint8, device="cuda")
        table = torch.full((5 * 16,), 0x5A, dtype=torch.uint8, device="cuda")
        bs.decode_lod_pool(cuts, ijk, grid, pool=pool, table=table)
        assert np.array_equal(np.frombuffer(table.cpu().numpy().tobytes(), POOL_ENTRY), want_t)
        p = pool.cpu().numpy()
        used = np.zeros(p.size, bool)
        for b, c in enumerate(cuts):
            e = want_t[b]
            if c < 0:
                assert e["offset"] == -1
                continue
            sx, sy, sz = (int(v) for v in e["shift"])
            n = (X >> sx) * (Y >> sy) * (Z >> sz)
            o = int(e["offset"])
            assert o % 256 == 0 and o + n <= nbytes
            used[o:o + n] = True
            stored = p[o:o + n].reshape(Z >> sz, Y >> sy, X >> sx)
            up = np.repeat(np.repeat(np.repeat(stored, 1 << sz, 0), 1 << sy, 1), 1 << sx, 2)
            assert np.array_equal(up, decs[b].at(int(c))), (list(cuts), b)
        assert np.all(p[~used] == POISON)


# ---- d. 64-bit token offsets ----

@pytest.mark.parametrize("family", ["dense7", "blockprune"])
def test_foreign_streams_with_64_bit_offsets(vr, monkeypatch, family):
    """VRHIP_FORCE_IDX64 (read when the set is created) takes the set through the block-relative index and the
    zeroed bases that set_tree writes for an installed stream."""
    monkeypatch.setenv("VRHIP_FORCE_IDX64", "1")
    lv = R.make(TILED[0], family, "std")
    bs = install(vr, lv)
    monkeypatch.delenv("VRHIP_FORCE_IDX64")
    dec = R.decode_levels(lv)
    D = lv.D
    cuts = [None, D, D - 3, D - 4, D - 7]
    first = {c: decode(bs, c) for c in cuts}
    for c in cuts:
        assert np.array_equal(first[c][0], dec.at(c)), ("default", c)
    bs.set_switch("decode_walk", 1)
    for c in cuts:
        assert np.array_equal(decode(bs, c)[0], dec.at(c)), ("decode_walk", c)
    bs.set_switch("decode_walk", 0)
    for c in cuts:
        assert decode(bs, c).tobytes() == first[c].tobytes(), ("default again", c)


# ---- e. bytes in, bytes out ----

@pytest.mark.parametrize("dims", [TILED[0], (128, 8, 4)], ids=_ids)
def test_bytes_in_bytes_out(vr, tmp_path, dims):
    for family, law in [(f, "std") for f in R.FAMILIES] + [("mixed", "chain_ns")]:
        lv = R.make(dims, family, law)
        packed = R.pack(lv.tokens)
        bs = install(vr, lv)
        info = bs.info(0)
        assert info["num_active_nodes"] == lv.tokens.size and info["tree_bytes"] == packed.size, family
        assert info["orig_tree_depth"] == lv.D and info["max_tree_depth"] == lv.M
        assert np.array_equal(bs.tree(0), packed), family
        assert np.array_equal(bs.distance_map(0), lv.dmap), family
        want, got = str(tmp_path / "want.bin"), str(tmp_path / "got.bin")
        R.write_file(want, dims, lv.tokens, lv.dmap)
        bs.save(got)
        assert open(got, "rb").read() == open(want, "rb").read(), (family, law)
        opened = vr.BrickSet.open(want)
        assert opened.dims == tuple(dims)
        dec = R.decode_levels(lv)
        assert np.array_equal(decode(opened, None)[0], dec.at()), (family, law)
        assert np.array_equal(decode(opened, lv.D - 2)[0], dec.at(lv.D - 2)), (family, law)


# ---- f. refusals: nothing is launched for a stream the grammar does not produce ----

@pytest.mark.parametrize("dims", [TILED[0], (16, 8, 4)], ids=_ids)
def test_malformed_streams_are_refused_and_change_nothing(vr, dims):
    held = R.make(dims, "mixed", "std")
    bs = install(vr, held)
    before = decode(bs, None).copy()
    assert np.array_equal(before[0], R.decode_levels(held).at())
    lv = R.make(dims, "dense7", "sat")
    t = lv.tokens
    for what, bad in (("last token dropped", t[:-1]), ("a token appended", np.append(t, 0).astype(np.uint8)),
                      ("ends inside a grown branch", t[:-3])):
        with pytest.raises(vr.VrError) as e:
            bs.set_tree(0, R.pack(bad), bad.size, lv.dmap)
        assert e.value.status == VR_ERR_FORMAT, what
        assert bs.info(0)["num_active_nodes"] == held.tokens.size, what
        assert np.array_equal(bs.tree(0), R.pack(held.tokens)), what
        assert decode(bs, None).tobytes() == before.tobytes(), what


# ---- the stream that found a bug ----

def test_golden_chain_distance_stream(vr):
    """tests/golden/foreign_chain_distances.npz, 49 tokens at 128 x 64 x 64: two voxel leaves whose grown branches
    subtract more than 256 within the first four codes (200 + 180) and within the last three (220 + 150 - 90).  The
    grown-branch tables of k_decode_tile, the kernel that decodes maps with other distances than 64 >> i, kept the
    composed sum in a ten-bit field biased by 256: such a sum overwrote the entry's bounds and token count.  Every
    switch and cut, against the plain recursive walker."""
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "foreign_chain_distances.npz"))
    tokens, dmap = f["tokens"], f["dmap"]
    dims = TILED[0]
    D = R.depth_of(dims)
    M = D + R.CHAIN
    assert dmap.size == M + 1 and tuple(dmap[D + 1:]) != R.STD_CHAIN
    bs = vr.BrickSet(1, dims)
    bs.set_tree(0, R.pack(tokens), tokens.size, dmap)
    cuts = [None, M - 1, D + 5, D + 4, D + 2, D + 1, D, D - 3]
    want = {c: R.decode_recursive(dims, tokens, dmap, c) for c in cuts}
    assert want[None][0, 0, 0] == 0 and want[None][0, 0, 1] == 90
    for name in (None,) + SWITCHES:
        if name:
            bs.set_switch(name, 1)
        for c in cuts:
            assert np.array_equal(decode(bs, c)[0], want[c]), (name, c)
        if name:
            bs.set_switch(name, 0)
