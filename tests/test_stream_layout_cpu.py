"""tests/streamlayout.py against the stream generator's own block census, and the census of the contents that
tests/test_gpu_concat_edges.py builds: every path class of k_concat12 must occur in them, read off the oracle's streams.

No GPU here: the streams are refstream's and the CPU oracle's."""
import numpy as np
import pytest

import refstream as RS
import streamlayout as SL
import test_gpu_concat_edges as CE

DIMS = {12: (16, 16, 16), 14: (32, 32, 16), 18: (64, 64, 64)}       # (x, y, z)
FAMILIES = ("dense7", "blockprune", "shallow", "root3", "root_children3", "mixed")


def _spine_model(lv):
    """tokens of depth < D-12 per leftmost block, straight from the levels"""
    db = lv.D - 12
    nsp = np.zeros(1 << db, np.int64)
    for d in range(db):
        here = np.flatnonzero(lv.tok[d] != 255)
        np.add.at(nsp, here << (db - d), 1)
    return nsp


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("D", sorted(DIMS))
def test_layout_of_generated_streams(D, family):
    """The parse finds the generator's blocks again: string lengths, spines, offsets that are the running sums."""
    lv = RS.make(DIMS[D], family)
    assert lv.D == D
    tokens = lv.tokens
    lay = SL.layout(RS.pack(tokens), tokens.size, D)
    assert np.array_equal(lay["cnt"], RS.census(lv)["block_tokens"])
    assert np.array_equal(lay["nsp"], _spine_model(lv))
    assert np.array_equal(lay["tot"], lay["nsp"] + lay["cnt"])
    assert int(lay["tot"].sum()) == tokens.size
    assert np.array_equal(lay["g0"], np.cumsum(lay["tot"]) - lay["tot"])
    assert np.array_equal(lay["w0"], lay["g0"] >> 4) and np.array_equal(lay["wl"], (lay["g0"] + lay["tot"] - 1) >> 4)
    assert int(lay["cnt"].max()) <= SL.MAX_CNT
    if family == "dense7":
        assert (lay["cnt"] == SL.MAX_CNT).all()


def test_layout_rejects_what_the_grammar_does_not_produce():
    tokens = RS.make(DIMS[14], "mixed").tokens
    SL.layout(RS.pack(tokens), tokens.size, 14)
    with pytest.raises(ValueError):
        SL.layout(RS.pack(tokens), tokens.size - 1, 14)          # ends early
    with pytest.raises(ValueError):
        SL.layout(RS.pack(np.append(tokens, 3)), tokens.size + 1, 14)     # a token left over


def test_classes_of_hand_made_layouts():
    """the class boundaries on layouts written down by hand"""
    def lay(nsp, cnt):
        nsp, cnt = np.array(nsp, np.int64), np.array(cnt, np.int64)
        tot = nsp + cnt
        g0 = np.cumsum(tot) - tot
        return dict(g0=g0, nsp=nsp, cnt=cnt, tot=tot, w0=g0 >> 4, wl=(g0 + tot - 1) >> 4)

    a = lay([2, 0, 1, 0], [14, 32, 0, 33])       # g0 0, 16, 48, 49
    assert SL.block_classes(a, 0) == ["S1", "S4", "S7"]
    assert SL.block_classes(a, 1) == ["S2", "S5", "S8"]
    assert SL.block_classes(a, 2) == ["S1", "S6"]
    assert SL.block_classes(a, 3) == ["L1", "L2", "L3_w0_3", "L3_wl_1", "L7"]
    b = lay([0, 1], [15, 31])                     # g0 15: 15 + 32 > 32, three words
    assert SL.block_classes(b, 1) == ["S3", "S5", "S7", "S8"]
    c = lay([0, 3], [14, SL.MAX_CNT])             # a spine across a word, 2304 words of string
    assert SL.block_classes(c, 1) == ["L3_w0_0", "L3_wl_%d" % (((14 + 3 + SL.MAX_CNT - 1) >> 4) & 3), "L4", "L5", "L7", "L8"]
    d = lay([1] + [0] * 15 + [1] + [0] * 15 + [0] * 16 + [0] * 15 + [1], [45] + [1, 1] + [0] * 13 + [0] * 16 + [0] * 16 + [0] * 15 + [40])
    cd = SL.classes(d)
    assert cd["W7"] == 1 and cd["W2"] == 1 and cd["W1"] == 0 and cd["W3"] == 1 and cd["W4_first"] == 1 and cd["W4_last"] == 1
    assert SL.classes(lay([0], [5]))["W8_nblk1"] == 1 and SL.classes(lay([1, 0, 1, 0], [5, 5, 5, 5]))["W8_nblk4"] == 1
    full = lay([4] + [0] * 15, [SL.MAX_CNT] * 16)
    cf = SL.classes(full)
    assert cf["W6"] == 1 and cf["W5"] == 1 and cf["L8"] == 16


def test_oracle_streams_parse(oracle):
    """every stream the GPU module compares against follows the grammar, with no token left over, and its blocks lie
    back to back"""
    for name in CE.CASES:
        for ref, lay in zip(CE.case(oracle, name)[1], CE.layouts(oracle, name)):
            assert int(lay["tot"].sum()) == ref.numActiveNodes, name
            assert np.array_equal(lay["g0"], np.cumsum(lay["tot"]) - lay["tot"]), name


def test_content_classes(oracle):
    """Every class of blocks, workgroups and words that k_concat12 tells apart occurs in the contents of
    tests/test_gpu_concat_edges.py (constant bricks aside: the kernels leave them to the closed form).

    W4_last: a workgroup's root token belongs to its first block and a node's sibling always has a token, so a full
    workgroup in which only the last block owns tokens does not exist; the class is the nearest thing there is, a
    workgroup whose only block on the chunk list is its last."""
    total = dict.fromkeys(SL.MANDATORY + SL.OPTIONAL, 0)
    for name in CE.CASES:
        vols, refs, tol, midrange = CE.case(oracle, name)
        per = dict.fromkeys(total, 0)
        for vol, lay in zip(vols, CE.layouts(oracle, name)):
            if not CE.is_constant(vol, tol):
                per = SL.add(per, SL.classes(lay))
        print("%-20s %s" % (name, " ".join("%s=%d" % (k, v) for k, v in per.items())))
        total = SL.add(total, per)
    missing = [k for k in SL.MANDATORY + SL.OPTIONAL if not total[k]]
    assert not missing, missing
    # each shape on its own reaches what its block count allows
    for shape, need in (("16x16x16", ("W8_nblk1",)), ("32x32x16", ("W8_nblk4", "S1", "S6", "W7")),
                        ("64x32x32", ("S1", "S2", "S3", "S4", "S5", "S6", "S7", "L2", "L5", "W7", "W4_last")),
                        ("64x64x64", ("S1", "S2", "S3", "S4", "S5", "S6", "S7", "L2", "L4", "L5", "W1", "W3", "W4_first", "W4_last", "W7"))):
        per = dict.fromkeys(total, 0)
        for tol in (1, 4):
            name = "%s tol %d" % (shape, tol)
            for vol, lay in zip(CE.case(oracle, name)[0], CE.layouts(oracle, name)):
                if not CE.is_constant(vol, tol):
                    per = SL.add(per, SL.classes(lay))
        assert all(per[k] for k in need), (shape, [k for k in need if not per[k]])
    full = dict.fromkeys(total, 0)
    for lay in CE.layouts(oracle, "full"):
        full = SL.add(full, SL.classes(lay))
    assert full["W5"] and full["W6"] and full["L8"], full


def test_handle_reuse_shrinks_strings(oracle):
    """the blocks test_one_handle_long_short_long is about exist: strings that shrink from long to short and from long
    to a shorter long one, ending inside a word (L7)"""
    to_short, to_long = CE.shrinking_blocks(oracle)
    print("long -> short: %d blocks, long -> shorter long: %d blocks" % (len(to_short), len(to_long)))
    assert to_short and to_long
