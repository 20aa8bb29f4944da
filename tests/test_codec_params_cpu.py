"""The codec's two parameters outside the box every other module stays in (tolerance 0 .. 12, max_epochs 0 .. 5), on
the CPU: (a) the oracle against the reference codec itself on the extended ladders, (b) a census on the oracle alone
showing that the ladders' values really behave differently from one another, (c) known answers recorded from the
reference (tests/golden/codec_param_known_answers.json, written by oracle/gen_codec_param_answers.py), and the
interface's ceiling on max_epochs.  tests/test_gpu_codec_params.py runs the HIP codec over the same ladders."""
import ctypes as C

import numpy as np
import pytest

import codec_params as P
from test_ref_parity import compare


@pytest.fixture(scope="module")
def ref(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref/libvkref.so is not built: no reference sources at %s" % oracle.ref_dir())
    return oracle


# ---- (a) oracle == reference ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", P.VOLUMES)
@pytest.mark.parametrize("midrange", [False, True], ids=["kd", "mid"])
@pytest.mark.parametrize("shape", P.CPU_SHAPES, ids=P.sid)
def test_oracle_matches_ref_on_the_extended_ladders(ref, shape, midrange, name, tmp_path):
    """Everything test_ref_parity.compare checks: depths, token count, both distance maps, both streams, the 4-bit
    packing, levelCut and the saved file -- TOL_X x epochs {0, 2} and EP_X x tolerance {0, 1, 13}."""
    vol = P.volume(name, shape)
    for tol, ep in P.TOL_SETTINGS + P.EP_SETTINGS:
        compare(ref, vol, tol, ep, midrange, tmp_path, (P.sid(shape), name, tol, ep, midrange))


# ---- (b) census on the oracle alone ---------------------------------------------------------------------------------
def _stream(t):
    return (int(t.numActiveNodes), t.tree.tobytes(), t.distanceMap.tobytes())


def _pairwise_different(streams):
    return len(set(streams)) == len(streams)


def test_census_tolerance_with_a_level_loop(oracle):
    """noise 32^3, two epochs: 12, 13, 16, 31, 32 and 64 give six streams; the leaf errors after the level loop stop at
    61, so every tolerance from 64 up gives the tolerance-64 stream."""
    s = {t: _stream(P.oracle_tree(oracle, "noise", P.S15, t, 2, 0)) for t in (12,) + P.TOL_X}
    assert _pairwise_different([s[t] for t in (12, 13, 16, 31, 32, 64)])
    assert P.oracle_tree(oracle, "noise", P.S15, 64, 2, 0).leaf_stats()["max_after"] == 61
    for t in P.TOL_X:
        if t >= 64:
            assert s[t] == s[64], t


def test_census_tolerance_without_a_level_loop(oracle):
    """noise 16^3, no epochs: the leaf errors reach 255, so the tolerance matters all the way to 256, where the stream
    becomes one token."""
    trees = {t: P.oracle_tree(oracle, "noise", P.S12, t, 0, 0) for t in P.TOL_X}
    nodes = [int(trees[t].numActiveNodes) for t in (64, 100, 255, 256)]
    print("nodes at tolerance 64, 100, 255, 256: %r" % nodes)
    assert len(set(nodes)) == 4 and nodes == sorted(nodes, reverse=True)
    assert nodes[3] == 1
    for t in P.TOL_X:
        if t >= 256:
            assert _stream(trees[t]) == _stream(trees[256]), t


def _last_epochs(tree):
    last = {}
    for r in tree.trace():
        last[r["depth"]] = max(last.get(r["depth"], -1), r["epoch"])
    return last


def test_census_epochs(oracle):
    """rm_like 128 x 64 x 64, tolerance 1: more than five epochs change the stream, levels stop at different epochs
    before the limit, and the long runs revert."""
    trees = {e: P.oracle_tree(oracle, "rm_like", P.S19, 1, e, 0) for e in (5,) + P.EP_X}
    assert _pairwise_different([_stream(trees[e]) for e in (5, 6, 8, 13)])
    assert _stream(trees[13]) == _stream(trees[40]) == _stream(trees[200])
    for e in P.EP_X:
        last = _last_epochs(trees[e])
        print("max_epochs %d: last epoch per level %r, reverts %d" % (e, sorted(last.items()), trees[e].numReverts))
        assert min(last.values()) < e - 1, e
        assert trees[e].numReverts >= 1, e
    assert max(_last_epochs(trees[13]).values()) >= 6


def _settings(cases):
    out = {}
    for name, shape, tol, ep in cases:
        out.setdefault((shape, tol, ep), []).append(name)
    return sorted(out.items())


_HIGH = _settings(P.high_tolerance_fused_cases())


@pytest.mark.parametrize("setting,names", _HIGH, ids=["%s-tol%d-ep%d" % (P.sid(s[0]), s[1], s[2]) for s, _ in _HIGH])
def test_census_high_tolerance_fused_cases_mix_dead_and_live_blocks(oracle, setting, names):
    """What the GPU module's high-tolerance settings at D >= 14 show the fused kernels: 4096-leaf blocks pruned whole
    next to live blocks that hold pruned leaves and live leaves with a non-zero code.  Asserted for every case of the
    setting that can hold both (codec_params.mixes_dead_and_live_blocks: the constant-block mix of every shape, and the
    smooth and mixed fields at 128 x 64 x 64); noise never has a block pruned whole (measured: 0 of 4, 8, 16 and 128),
    the smooth fields of 32 x 32 x 16 .. 128 x 32 x 16 neither, and they are only printed."""
    shape, tol, ep = setting
    asserted = 0
    for name in names:
        boxes = P.box_leaf_census(P.oracle_tree(oracle, name, shape, tol, ep, 0))
        dead = sum(b is None for b in boxes)
        both = sum(b is not None and b[0] > 0 and b[1] > 0 for b in boxes)
        print("%s: %d boxes, %d pruned whole, %d live with pruned and coded leaves" % (name, len(boxes), dead, both))
        if P.mixes_dead_and_live_blocks(name, shape):
            assert dead >= 1 and both >= 1, name
            asserted += 1
    assert asserted >= 1


# ---- (c) known answers ------------------------------------------------------------------------------------------------
def _case_args(c):
    return c["volume"], c["seed"], tuple(c["shape"]), c["tolerance"], c["max_epochs"], c["variant"]


def _case_id(c):
    return "%s-%s-tol%d-ep%d-%s" % (c["volume"], P.sid(tuple(c["shape"])), c["tolerance"], c["max_epochs"], c["variant"])


def test_known_answers_are_the_listed_cases():
    assert [_case_args(c) for c in P.known_answers()] == [tuple(k) for k in P.KNOWN_CASES]


@pytest.mark.parametrize("case", P.known_answers(), ids=_case_id)
def test_oracle_reproduces_known_answers(oracle, case):
    name, seed, shape, tol, ep, vname = _case_args(case)
    t = P.oracle_tree(oracle, name, shape, tol, ep, P.VARIANTS[vname], seed)
    assert P.known_record(oracle, t, name, seed, shape, tol, ep, vname) == case


@pytest.mark.parametrize("case", P.known_answers(), ids=_case_id)
def test_ref_reproduces_known_answers(ref, case):
    name, seed, shape, tol, ep, vname = _case_args(case)
    r = ref.RefTree(P.volume(name, shape, seed), tolerance=tol, max_epochs=ep, midrange=vname == "mid").build()
    assert P.known_record(ref, r, name, seed, shape, tol, ep, vname) == case


# ---- the ceiling on max_epochs ----------------------------------------------------------------------------------------
def test_create_refuses_more_than_vr_max_epochs_before_the_device():
    """vr_brickset_create answers VR_ERR_UNSUPPORTED above VR_MAX_EPOCHS whatever the device: the level loop's launches
    grow with max_epochs, so INT32_MAX would never return.  Nothing is ever built with such a value."""
    import os
    import re
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "vrhip.h")).read()
    assert int(re.search(r"#define\s+VR_MAX_EPOCHS\s+(\d+)", hdr).group(1)) == 1024
    h = C.c_void_p()
    dims = (C.c_int64 * 3)(16, 16, 16)
    for e in (1025, 40000, 2 ** 31 - 1):
        assert L.vr_brickset_create(C.byref(h), 1, dims, 1, e, 0) == -7 and not h, e     # VR_ERR_UNSUPPORTED
    assert L.vr_brickset_create(C.byref(h), 1, dims, 1, -1, 0) == -1                     # (negative: invalid, as before)
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    if n.value == 0:       # the ceiling itself, and any tolerance, pass the argument checks and reach the device check
        assert L.vr_brickset_create(C.byref(h), 1, dims, 2 ** 31 - 1, 1024, 0) == -2
