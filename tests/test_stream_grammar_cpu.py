"""The references of tests/refstream.py against each other and against the oracle, on grammar-random streams that no
encoder emits, and the census conditions that keep tests/test_gpu_foreign_streams.py honest.
No GPU: the plain recursive walker == the vectorised reference == OracleTree.open(file), bit for bit."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402

SMALL = [(4, 1, 2), (8, 8, 8), (16, 8, 4), (128, 8, 4), (32, 16, 16)]
TILED = [(128, 64, 64), (128, 128, 64), (128, 128, 128)]      # x deepest, second and first in the deepest triple
NO_CODES = ("root3", "root_children3", "zeros")               # streams that change no value: every cut is dmap[0]
MONO = ("mono_up", "mono_down")
BIG = ("dense7", "blockprune", "mixed")                       # the families the GPU module decodes at 128^3


def families_at(dims):
    return BIG if dims == (128, 128, 128) else R.FAMILIES


def _open(oracle, tmp_path, lv, name="s.bin"):
    p = str(tmp_path / name)
    R.write_file(p, lv.dims, lv.tokens, lv.dmap)
    return oracle.OracleTree.open(p), p


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("dims", SMALL, ids=lambda d: "%dx%dx%d" % d)
def test_walker_equals_levels_equals_oracle(oracle, tmp_path, dims, family):
    """Every map law, every cut 0 .. M: decode_recursive == decode_levels == the oracle's levelCutProgressive, and the
    oracle's levelCut at full depth."""
    for law in R.LAWS:
        lv = R.make(dims, family, law)
        dec = R.decode_levels(lv)
        tree, _ = _open(oracle, tmp_path, lv)
        assert tree.origTreeDepth == lv.D and tree.maxTreeDepth == lv.M and tree.numActiveNodes == lv.tokens.size
        for cut in range(lv.M + 1):
            want = dec.at(cut)
            assert np.array_equal(R.decode_recursive(dims, lv.tokens, lv.dmap, cut), want), (law, cut, "walker")
            assert np.array_equal(tree.levelCutProgressive(cut), want), (law, cut, "oracle")
        assert np.array_equal(tree.levelCut(), dec.at()), law
        assert np.array_equal(R.decode_recursive(dims, lv.tokens, lv.dmap), dec.at()), law


@pytest.mark.parametrize("family", ["dense7", "blockprune", "mixed"])
@pytest.mark.parametrize("dims", TILED[:2], ids=lambda d: "%dx%dx%d" % d)
def test_levels_equal_oracle_on_tiled_extents(oracle, tmp_path, dims, family):
    lv = R.make(dims, family, "std")
    dec = R.decode_levels(lv)
    tree, _ = _open(oracle, tmp_path, lv)
    D, M = lv.D, lv.M
    assert np.array_equal(tree.levelCut(), dec.at())
    for cut in (M, M - 1, D + 1, D, D - 3, D - 6, 3, 0):
        assert np.array_equal(tree.levelCutProgressive(cut), dec.at(cut)), cut


@pytest.mark.parametrize("dims", SMALL, ids=lambda d: "%dx%dx%d" % d)
def test_reference_codec_reads_foreign_streams(oracle, tmp_path, dims):
    """The reference's own VolumeKdtree::open + levelCut, compiled in place, on the same files: equal to the walker's
    full-depth decode for every family and map law (no class of grammatical stream was found on which it differs)."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built (no reference sources)")
    for family in R.FAMILIES:
        for law in R.LAWS:
            lv = R.make(dims, family, law)
            _, p = _open(oracle, tmp_path, lv)
            ref = oracle.RefTree.open(p)
            assert ref.maxTreeDepth == lv.M and ref.numActiveNodes == lv.tokens.size
            assert np.array_equal(ref.levelCut(), R.decode_levels(lv).at()), (family, law)


def test_malformed_streams_are_not_grammatical():
    """The three malformed shapes the GPU module hands to set_tree (which must refuse them): the walker refuses them."""
    lv = R.make((16, 8, 4), "dense7", "std")
    t = lv.tokens
    for bad in (t[:-1], np.append(t, 0).astype(np.uint8), t[:-3]):
        with pytest.raises(ValueError):
            R.decode_recursive(lv.dims, bad, lv.dmap)


def test_pack_and_file_layout(tmp_path):
    lv = R.make((16, 8, 4), "mixed", "chain_ns")
    b = R.pack(lv.tokens)
    assert b.size == (lv.tokens.size + 3) // 4 and np.array_equal(R.unpack(b, lv.tokens.size), lv.tokens)
    assert all(((int(b[i >> 2]) >> (2 * (i & 3))) & 3) == lv.tokens[i] for i in range(0, lv.tokens.size, 7))
    p = str(tmp_path / "f.bin")
    R.write_file(p, lv.dims, lv.tokens, lv.dmap)
    raw = open(p, "rb").read()
    assert len(raw) == 88 + lv.M + 1 + b.size and raw[88:88 + lv.M + 1] == lv.dmap.tobytes() and raw[88 + lv.M + 1:] == b.tobytes()
    assert tuple(lv.dmap[lv.D + 1:]) != R.STD_CHAIN


# ---- the census conditions: what the streams of the GPU module contain ----

@pytest.fixture(scope="module")
def censuses():
    out = {}
    for dims in TILED:
        for family in families_at(dims):
            for law in ("std", "sat"):
                lv = R.make(dims, family, law)
                dec = R.decode_levels(lv)
                c = R.census(lv, dec)
                D = lv.D
                c["full_ne_D"] = bool((dec.leaves() != dec.leaves(D)).any())
                c["D_ne_D3"] = bool((dec.leaves(D) != dec.leaves(D - 3)).any())
                out[dims, family, law] = c
    return out


@pytest.mark.parametrize("dims", TILED, ids=lambda d: "%dx%dx%d" % d)
def test_census_structure(censuses, dims):
    """Over the families of one tiled extent together: a prune at every depth 1 .. D, every number of branch codes
    0 .. 7 and seven-token branches with and without the terminator, a 4096-leaf block of 36 863 tokens and one of a
    single token, a 128 x 16 x 16 region wholly dead and one whose blocks alternate between live and dead.  (128^3
    holds three of the families, none of which prunes at depth 1: prunes from depth 2 on there.)"""
    D = R.depth_of(dims)
    fams = families_at(dims)
    cs = [censuses[dims, f, "std"] for f in fams]
    for d in range(1 if "shallow" in fams else 2, D + 1):
        assert any(c["prunes"][d] > 0 for c in cs), d
    for k in range(R.CHAIN + 1):
        assert any(c["chain_codes"][k] > 0 for c in cs), k
    assert any(c["seven_with_3"] > 0 for c in cs) and any(c["seven_without_3"] > 0 for c in cs)
    assert int(censuses[dims, "dense7", "std"]["block_tokens"].min()) == 36863
    assert censuses[dims, "dense7", "std"]["tokens"] == (2 << D) - 1 + 7 * (1 << D)
    assert any((c["block_tokens"] == 1).any() for c in cs)
    assert censuses[dims, "blockprune", "std"]["regions_alternating"] > 0
    assert any(c.get("regions_dead", 0) > 0 for c in cs)
    if "shallow" in fams:
        assert censuses[dims, "dense0", "std"]["tokens"] == (2 << D) - 1 + (1 << D)
        assert censuses[dims, "shallow", "std"]["regions_dead"] > 0
        assert censuses[dims, "root3", "std"]["tokens"] == 1 and censuses[dims, "root_children3", "std"]["tokens"] == 3


@pytest.mark.parametrize("dims", TILED, ids=lambda d: "%dx%dx%d" % d)
def test_census_clamps(censuses, dims):
    """Additions that would leave [0, 255].  Under `sat` every family whose codes are random clamps on the paths of at
    least 1 % of the voxels at 255 and at 0, at interior depths and in grown branches (dense0 has no branch codes).
    A mono family moves one way only: mono_up can clamp at 255 alone and mono_down at 0 alone, so each is held to its
    own end, under `std` in its grown branches (its interior sums stay below the clamp there) and under `sat` at
    interior depths as well."""
    for family in families_at(dims):
        if family in NO_CODES:
            continue
        ends = {"mono_up": ("hi",), "mono_down": ("lo",)}.get(family, ("hi", "lo"))
        c = censuses[dims, family, "sat"]
        for e in ends:
            assert c["clamp_%s_fraction" % e] >= 0.01, (family, e)
            assert c["clamp_%s_interior" % e] > 0, (family, e)
            if family != "dense0":
                assert c["clamp_%s_chain" % e] > 0, (family, e)
        if family in MONO:
            c = censuses[dims, family, "std"]
            assert c["clamp_%s_fraction" % ends[0]] >= 0.01 and c["clamp_%s_chain" % ends[0]] > 0, family


@pytest.mark.parametrize("dims", TILED, ids=lambda d: "%dx%dx%d" % d)
def test_census_levels_matter(censuses, dims):
    """The full-depth decode differs from the cut-D decode and that from the cut-(D-3) decode, so a kernel that ignores
    a level cannot pass.  Not for streams that change no value (root3, root_children3, zeros); dense0 has no branch
    codes, so only its cut-D and cut-(D-3) decodes differ; and in a mono stream every node of a depth holds one value,
    so under `sat`, once an interior depth has clamped, all deeper cuts are equal: the mono families are held to this
    under `std`."""
    for family in families_at(dims):
        if family in NO_CODES:
            continue
        for law in ("std", "sat"):
            if family in MONO and law == "sat":
                continue
            c = censuses[dims, family, law]
            assert c["D_ne_D3"], (family, law)
            if family != "dense0":
                assert c["full_ne_D"], (family, law)


def test_golden_chain_distance_stream(oracle, tmp_path):
    """tests/golden/foreign_chain_distances.npz (the stream tests/test_gpu_foreign_streams.py decodes on the GPU): it is
    grammatical, its grown-branch distances are not 64 >> i, its two leaves subtract more than 256 within four branch
    codes and within the last three, and the walker agrees with the oracle on it."""
    f = np.load(os.path.join(os.path.dirname(__file__), "golden", "foreign_chain_distances.npz"))
    tokens, dmap = f["tokens"], f["dmap"]
    dims = TILED[0]
    D = R.depth_of(dims)
    assert set(f.files) == {"tokens", "dmap"} and tokens.dtype == np.uint8 and dmap.dtype == np.uint8
    assert tuple(dmap[D + 1:]) != R.STD_CHAIN
    assert int(dmap[D + 1]) + int(dmap[D + 2]) > 256 and int(dmap[D + 5]) + int(dmap[D + 6]) - int(dmap[D + 7]) > 256
    p = str(tmp_path / "g.bin")
    R.write_file(p, dims, tokens, dmap)
    tree = oracle.OracleTree.open(p)
    for cut in (D + 7, D + 5, D + 4, D + 2, D + 1, D, D - 3):
        assert np.array_equal(R.decode_recursive(dims, tokens, dmap, cut), tree.levelCutProgressive(cut)), cut
    assert np.array_equal(R.decode_recursive(dims, tokens, dmap), tree.levelCut())
