"""The general-extent references of tests/refstream.py against each other and against the oracle, on grammar-random
streams that no encoder emits, and the census conditions that keep tests/test_gpu_foreign_general.py honest.  No GPU:
the plain recursive walker over boxes == the vectorised reference == OracleTree.open(file), bit for bit, at every cut.

One condition cannot be asked of any stream: a cell written by several leaves.  A box is handed to both children only
once it holds one cell, and no box above depth D does: cutting an extent e >= 2 leaves halves of e / 2 and e - e / 2
cells, whose floor(log2) is at least floor(log2 e) - 1, so the sum of floor(log2 extent) over the three axes falls by at
most one per level, starts at D and is 0 only for a box of one cell.  test_no_box_above_the_leaves_holds_one_cell
asserts that on every extent used here; the rule stays in the walker because the definition states it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402

SMALL = [(3, 1, 1), (5, 3, 2), (7, 9, 2), (12, 6, 5), (5, 6, 12), (24, 10, 6)]
LARGE = [(40, 16, 24), (2048, 2, 2), (96, 64, 48)]
BIG = ("dense7", "blockprune", "mixed", "leafprune")            # the families of the LARGE extents
GPU_EXTENTS = [(3, 1, 1), (5, 3, 2), (7, 9, 2), (12, 6, 5), (24, 10, 6)] + LARGE    # tests/test_gpu_foreign_general.py
GPU_LAWS = ("std", "sat", "chain_ns")
NO_CODES = ("root3", "root_children3", "zeros")


def families_at(dims):
    return BIG if dims in LARGE else R.FAMILIES


def _ids(d):
    return "%dx%dx%d" % d


def _open(oracle, tmp_path, lv, name="s.bin"):
    p = str(tmp_path / name)
    R.write_file(p, lv.dims, lv.tokens, lv.dmap)
    return oracle.OracleTree.open(p), p


def test_existing_streams_are_unchanged():
    """make() of a power-of-two extent draws what it drew before the general streams existed (the census conditions of
    tests/test_stream_grammar_cpu.py are pinned to those seeds): CRC-32 of the tokens and the map, recorded from the
    parent revision."""
    import zlib
    want = {((16, 8, 4), "mixed", "std"): 1717635594, ((128, 8, 4), "leafprune", "sat"): 3353359101,
            ((4, 1, 2), "dense7", "chain_ns"): 3167432832, ((128, 64, 64), "blockprune", "std"): 4285058850,
            ((128, 128, 64), "shallow", "sat"): 276859005}          # the last one is salted
    for (dims, family, law), crc in want.items():
        lv = R.make(dims, family, law)
        assert not lv.general and lv.D == R.depth_of(dims) == R.depth_general(dims)
        assert zlib.crc32(lv.tokens.tobytes() + lv.dmap.tobytes()) == crc, (dims, family, law)


def test_depth_of_general_extents():
    for dims, D in zip(SMALL + LARGE, (1, 4, 6, 7, 7, 9, 13, 13, 17)):
        assert R.depth_general(dims) == D
    with pytest.raises(ValueError):
        R.depth_of((12, 6, 5))
    with pytest.raises(ValueError):
        R.depth_general((0, 4, 4))


@pytest.mark.parametrize("dims", SMALL + LARGE, ids=_ids)
def test_no_box_above_the_leaves_holds_one_cell(dims):
    """The module docstring's argument, checked box by box; and the two geometries (node by node in heap order, voxel
    by voxel from the root) describe the same walk: every voxel lies in the leaf box of its owner, and the leaf boxes
    of one depth tile the volume."""
    D = R.depth_general(dims)
    boxes = R.node_boxes(dims)
    for d in range(D):
        lo, hi, _ = boxes[d]
        assert ((hi - lo).prod(axis=0) > 1).all(), d
    g = R.voxel_geometry(dims)
    assert (g.single_at == D).all()
    lo, hi, cuts = boxes[D]
    assert int((hi - lo).prod(axis=0).sum()) == dims[0] * dims[1] * dims[2] and (cuts.sum(axis=0) == D).all()
    X, Y, Z = dims
    c = [np.arange(X)[None, None, :], np.arange(Y)[None, :, None], np.arange(Z)[:, None, None]]
    for a in range(3):
        assert ((lo[a][g.owner] <= c[a]) & (c[a] < hi[a][g.owner])).all(), a
    # a voxel that survives all seven halvings is the min corner of what is left; one that survives none is in the upper half
    cells = (hi - lo).prod(axis=0)
    assert ((g.surv == 255) | (g.surv < R.CHAIN)).all() and ((cells[g.owner] == 1) <= (g.surv == 255)).all()


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("dims", SMALL, ids=_ids)
def test_walker_equals_levels_equals_oracle(oracle, tmp_path, dims, family):
    """Every map law, every cut 0 .. M: decode_recursive_general == the vectorised reference == the oracle's
    levelCutProgressive, and the oracle's levelCut at full depth."""
    for law in R.LAWS:
        lv = R.make_general(dims, family, law)
        dec = R.decode_levels(lv)
        tree, _ = _open(oracle, tmp_path, lv)
        assert tree.origTreeDepth == lv.D and tree.maxTreeDepth == lv.M and tree.numActiveNodes == lv.tokens.size
        for cut in range(lv.M + 1):
            want = tree.levelCutProgressive(cut)
            assert np.array_equal(dec.at(cut), want), (law, cut, "levels")
            assert np.array_equal(R.decode_recursive_general(dims, lv.tokens, lv.dmap, cut), want), (law, cut, "walker")
        assert np.array_equal(tree.levelCut(), dec.at()), law
        assert np.array_equal(R.decode_recursive_general(dims, lv.tokens, lv.dmap), dec.at()), law


@pytest.mark.parametrize("family", BIG)
@pytest.mark.parametrize("dims", LARGE, ids=_ids)
def test_levels_equal_oracle_on_large_extents(oracle, tmp_path, dims, family):
    lv = R.make_general(dims, family, "std")
    dec = R.decode_levels(lv)
    tree, _ = _open(oracle, tmp_path, lv)
    D, M = lv.D, lv.M
    assert np.array_equal(tree.levelCut(), dec.at())
    for cut in (M, M - 1, D + 1, D, D - 3, D - 6, 3, 0):
        want = tree.levelCutProgressive(cut)
        assert np.array_equal(dec.at(cut), want), cut
        if dims == (40, 16, 24):
            assert np.array_equal(R.decode_recursive_general(dims, lv.tokens, lv.dmap, cut), want), (cut, "walker")


@pytest.mark.parametrize("dims", SMALL, ids=_ids)
def test_reference_codec_reads_foreign_streams(oracle, tmp_path, dims):
    """The reference's own VolumeKdtree::open + levelCut, compiled in place, on the same files: equal to the full-depth
    decode for every family and map law."""
    if not oracle.ref_available():
        pytest.skip("oracle/_ref is not built (no reference sources)")
    for family in R.FAMILIES:
        for law in R.LAWS:
            lv = R.make_general(dims, family, law)
            _, p = _open(oracle, tmp_path, lv)
            ref = oracle.RefTree.open(p)
            assert ref.maxTreeDepth == lv.M and ref.numActiveNodes == lv.tokens.size
            assert np.array_equal(ref.levelCut(), R.decode_levels(lv).at()), (family, law)


def test_the_walker_on_a_power_of_two_box_is_the_old_walker():
    """Where both definitions apply they are one: the general walker and reference on 8 x 4 x 2 and 2048 x 2 x 2 give
    what decode_recursive / rank_of_voxels give, at every cut."""
    for dims, family in (((8, 4, 2), "mixed"), ((2048, 2, 2), "leafprune")):
        lv = R.make_general(dims, family, "std")
        dec = R.decode_levels(lv)
        old = R.decode_levels(R.Levels(dims, lv.tok, lv.chain_len, lv.chain_tok, lv.dmap))
        for cut in ([None] + list(range(lv.M + 1)) if dims[0] == 8 else [None, lv.D, 3]):
            assert np.array_equal(dec.at(cut), old.at(cut)), (dims, cut)
            assert np.array_equal(R.decode_recursive_general(dims, lv.tokens, lv.dmap, cut), R.decode_recursive(dims, lv.tokens, lv.dmap, cut))


@pytest.mark.parametrize("dims", [(12, 6, 5), (40, 16, 24)], ids=_ids)
def test_malformed_streams_are_not_grammatical(dims):
    """The three malformed shapes the GPU module hands to set_tree and set_trees: the general walker refuses them."""
    lv = R.make_general(dims, "dense7", "sat")
    t = lv.tokens
    R.decode_recursive_general(dims, t, lv.dmap)
    for bad in (t[:-1], np.append(t, 0).astype(np.uint8), t[:-3]):
        with pytest.raises(ValueError):
            R.decode_recursive_general(dims, bad, lv.dmap)


def test_census_counts_are_the_walkers():
    """census_general counts from the geometry tables what the walker's own writes show: voxels no write covers, and
    cells written more than once."""
    for dims in SMALL:
        for family in ("mixed", "leafprune", "dense7"):
            lv = R.make_general(dims, family, "std")
            writes = []
            R.decode_recursive_general(dims, lv.tokens, lv.dmap, writes=writes)
            n = np.zeros(dims[::-1], np.int64)
            for lo, hi, _ in writes:
                n[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]] += 1
            c = R.census_general(lv, R.decode_levels(lv))
            assert c["dropped"] == int((n == 0).sum()) and c["multi_writer_cells"] == int((n > 1).sum()) == 0, (dims, family)


# ---- the census conditions: what the streams of the GPU module contain ----

@pytest.fixture(scope="module")
def censuses():
    out = {}
    for dims in GPU_EXTENTS:
        for family in families_at(dims):
            for law in GPU_LAWS:
                lv = R.make_general(dims, family, law)
                dec = R.decode_levels(lv)
                c = R.census(lv, dec)
                c.update(R.census_general(lv, dec))
                full = dec.at()
                c["cuts_above_D_that_differ"] = [k for k in range(lv.D) if (dec.at(k) != full).any()]
                c["cuts_in_branch_that_differ"] = [k for k in range(lv.D + 1, lv.M) if (dec.at(k) != full).any()]
                out[dims, family, law] = c
    return out


@pytest.mark.parametrize("dims", [d for d in GPU_EXTENTS if d != (2048, 2, 2)], ids=_ids)
def test_census_of_true_general_extents(censuses, dims):
    """Over the families of one extent, under each map law the GPU module uses: the halvings drop at least 10 % of all
    voxels (and of the `mixed` stream's alone), among them voxels at either side of the gather's comparison (a branch
    of exactly as many nodes as the voxel survives, and of one more); a pruned node's box has several cells and is none
    a power-of-two brick holds; branches of 0 .. 7 codes and both seven-token shapes; a cut above D and a cut inside
    the grown branches whose decode is not the full one.  No cell has two writers (the module docstring)."""
    fams = families_at(dims)
    for law in GPU_LAWS:
        cs = [censuses[dims, f, law] for f in fams]
        assert sum(c["dropped"] for c in cs) >= 0.10 * sum(c["voxels"] for c in cs), law
        mixed = censuses[dims, "mixed", law]
        assert mixed["dropped"] >= 0.10 * mixed["voxels"], law
        assert any(c["kept_at_edge"] > 0 for c in cs) and any(c["dropped_at_edge"] > 0 for c in cs), law
        assert any(c["pruned_multicell_off_grid"] > 0 for c in cs), law
        assert all(c["multi_writer_cells"] == 0 and c["overwritten_differently"] == 0 for c in cs), law
        assert any(c["cuts_above_D_that_differ"] for c in cs) and any(c["cuts_in_branch_that_differ"] for c in cs), law
    # branch lengths over the families and laws together (3 x 1 x 1 has two leaves a stream), and under `std` alone
    for cs in ([censuses[dims, f, law] for f in fams for law in GPU_LAWS], [censuses[dims, f, "std"] for f in fams]):
        for k in range(R.CHAIN + 1):
            assert any(c["chain_codes"][k] > 0 for c in cs), k
        assert any(c["seven_with_3"] > 0 for c in cs) and any(c["seven_without_3"] > 0 for c in cs)
    if R.depth_general(dims) >= 12:
        for f in ("mixed", "leafprune"):
            c = censuses[dims, f, "std"]
            assert c["kept_at_edge"] > 0 and c["dropped_at_edge"] > 0 and c["pruned_multicell_off_grid"] > 0, f
        assert int(censuses[dims, "dense7", "std"]["block_tokens"].min()) == 36863


def test_census_of_2048x2x2(censuses):
    """General only by its length: every leaf box is one cell, nothing is dropped, no pruned box is off the grid; the
    rest as above."""
    dims = (2048, 2, 2)
    for law in GPU_LAWS:
        cs = [censuses[dims, f, law] for f in BIG]
        assert all(c["dropped"] == 0 and c["dropped_at_edge"] == 0 and c["pruned_multicell_off_grid"] == 0 for c in cs)
        assert all(c["multi_writer_cells"] == 0 for c in cs)
        for k in range(R.CHAIN + 1):
            assert any(c["chain_codes"][k] > 0 for c in cs), (law, k)
        assert any(c["cuts_above_D_that_differ"] for c in cs) and any(c["cuts_in_branch_that_differ"] for c in cs), law
