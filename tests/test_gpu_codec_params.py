"""The HIP codec over the whole range of its two parameters, bit-exact against the CPU oracle.

Every other module stays inside tolerance 0 .. 12 and max_epochs 0 .. 5; the C ABI takes any non-negative int32 for
the tolerance and 0 .. VR_MAX_EPOCHS epochs.  Here the ladders of tests/codec_params.py (tolerance up to 2^31 - 1
around every power of two, 255 / 256 and the 16-bit limits; 6 .. 200 epochs) run on the smallest shape of every encode
path.  test_codec_params_cpu.py pins the oracle to the reference codec on the same ladders and shows on the oracle
alone that the values behave differently from one another.

Per case: everything test_gpu_codec.check_case compares, the progressive decode at cuts M, D, D-3, D/2 and 0, the saved
file reopened and decoded, and error_table() against its NumPy restatement; for MidRangeTree both streams, both
distance maps, the 4-bit packing and decode_range.

The fused prune kernels carry the tolerance in two signed 16-bit lanes; handed the caller's value they built wrong
streams from 32769 up (every D >= 12 case here at 32769, 40000, 65535, 65536 and 65537).  The kernels now get
min(tolerance, 256): a leaf error never exceeds 255."""
import json
import os

import numpy as np
import pytest

import codec_params as P
from test_error_table_cpu import table_py
from test_gpu_codec import check_case
from test_gpu_codec import vr  # noqa: F401  (the module's fixture)
from test_gpu_const_boxes import _census

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------- one case ----
def _build_checked(vr, O, vol, ref, tol, ep, variant):
    """A fresh handle built and compared with the oracle's tree `ref` (made with the variant's own switches)."""
    z, y, x = vol.shape
    what = (P.sid(vol.shape), tol, ep, variant)
    if variant != 2:
        # (check_case builds the unguarded oracle: the guard changes the work, not the result)
        _, bs = check_case(vr, O, vol, tol, ep, variant)
    else:
        bs = vr.BrickSet(1, (x, y, z), tol, ep, 2)
        bs.build(vol.copy())
    info, st = bs.info(0), ref.leaf_stats()
    assert info["tolerance"] == tol and info["max_epochs"] == ep, what          # the caller's values, not the kernels'
    assert info["orig_tree_depth"] == ref.origTreeDepth and info["max_tree_depth"] == ref.maxTreeDepth, what
    assert info["num_active_nodes"] == ref.numActiveNodes and info["num_reverts"] == ref.numReverts, what
    assert info["zero_run_rewrites"] == 0 and ref.zeroRunRewrites == 0, what
    assert info["max_error_before"] == st["max_before"] and info["max_error_after"] == st["max_after"], what
    assert abs(info["mean_l1_after"] - st["l1_after"]) < 1e-12, what
    assert list(bs.distance_map(0)) == list(ref.distanceMap), what
    assert np.array_equal(bs.tree(0), ref.tree), what
    if variant == 2:
        assert list(bs.distance_map_range(0)) == list(ref.distanceMap_range), what
        assert np.array_equal(bs.tree_range(0), ref.tree_range), what
        assert np.array_equal(bs.packed4(0), ref.convertToByteArray()), what
    return bs


def _cuts(ref):
    D, M = ref.origTreeDepth, ref.maxTreeDepth
    return sorted({M, D, max(D - 3, 0), D // 2, 0})


def _full_check(vr, O, vol, ref, tol, ep, variant, tmp_path):
    shape = vol.shape
    what = (P.sid(shape), tol, ep, variant)
    bs = _build_checked(vr, O, vol, ref, tol, ep, variant)
    D, M = ref.origTreeDepth, ref.maxTreeDepth
    full = ref.levelCut()
    assert np.array_equal(bs.decode().cpu().numpy().reshape(shape), full), what
    want = {c: ref.levelCutProgressive(c) for c in _cuts(ref)}
    assert np.array_equal(want[M], full), what
    for c in _cuts(ref):
        assert np.array_equal(bs.decode(cut_depth=c).cpu().numpy().reshape(shape), want[c]), (what, c)
    if variant == 2:
        for c in (-1, D, max(D - 6, 0)):
            got = bs.decode_range(cut_depth=c).cpu().numpy().reshape(shape)
            assert np.array_equal(got, ref.levelCutRange(None if c < 0 else c)), (what, "range", c)
    # the table of errors per cut against the set's own full decode, restated in NumPy
    decs = [bs.decode(cut_depth=c).cpu().numpy().reshape(1, -1).copy() for c in range(M + 1)]
    table = bs.error_table()
    assert table.shape == (M + 1, 1) and np.array_equal(table, table_py(decs, decs[M])), what
    # the file: written, reopened (side-cars rebuilt from the bytes alone), decoded
    p = str(tmp_path / "t.bin")
    bs.save(p)
    fs = vr.BrickSet.open(p, variant=2 if variant == 2 else 0)
    assert fs.info(0)["num_active_nodes"] == ref.numActiveNodes, what
    assert np.array_equal(fs.decode().cpu().numpy().reshape(shape), full), (what, "reopened")
    c = max(D - 3, 0)
    assert np.array_equal(fs.decode(cut_depth=c).cpu().numpy().reshape(shape), want[c]), (what, "reopened", c)
    return bs


def _outputs(bs, shape):
    info = bs.info(0)
    return (bs.tree(0).tobytes(), bs.distance_map(0).tobytes(), tuple(sorted(info.items())),
            bs.decode().cpu().numpy().tobytes(), bs.decode(cut_depth=max(info["orig_tree_depth"] - 3, 0)).cpu().numpy().tobytes())


def _switched_handles_agree(vr, O, vol, ref, tol, ep, bs):
    """constant-block mixes: the closed-form kernel, the path without it and the path that writes every level agree"""
    z, y, x = vol.shape
    first = _outputs(bs, vol.shape)
    for name in ("no_uniform_blocks", "no_skip_blocks"):
        other = vr.BrickSet(1, (x, y, z), tol, ep)
        other.set_switch(name, 1)
        other.build(vol.copy())
        assert _outputs(other, vol.shape) == first, (name, tol, ep)
    assert np.array_equal(bs.tree(0), ref.tree)


# ---------------------------------------------------------------- the paths ----
def test_shapes_reach_the_paths_they_are_named_for(vr, oracle, monkeypatch):
    """Each shape of the ladders is the smallest on its encode path: read off the depths the builds report, the stored
    decode plans and the oracle's own census of constant boxes -- not off the shape."""
    plans = json.load(open(os.path.join(P.GOLD, "decode_plans.json")))["plans"]
    region = {tuple(p[:3]) for p in plans if p[3][0] and p[4][0]}
    depth = {}
    for shape in (P.S9, P.S12, P.S14, P.S15, P.S19, P.G840, P.G15360, P.IDX64):
        z, y, x = shape
        bs = vr.BrickSet(1, (x, y, z), 1, 2).build(P.volume("rm_like", shape))
        depth[shape] = bs.info(0)["orig_tree_depth"]
    assert depth[P.S9] == 9                                     # below 12: k_prune_leaf and the k_emit_* kernels
    assert depth[P.S12] == 12                                   # the smallest fused brick: one 4096-leaf block, no skip blocks
    assert (depth[P.S14], depth[P.S15]) == (14, 15)             # skip blocks need D >= 14 (kd_encode.hip skipOn)
    assert depth[P.S19] == 19 and (128, 64, 64) in region and min(region, key=lambda d: d[0] * d[1] * d[2]) == (128, 64, 64)
    for shape in (P.G840, P.G15360):
        assert any(v & (v - 1) for v in shape)                  # general extents: the table-driven kernels
    assert depth[P.IDX64] == 16                                 # >= 12: VRHIP_FORCE_IDX64 applies
    for shape, name in P.CONST_MIX.items():                     # skipped and filled constant boxes beside a busy one
        vol = P.volume(name, shape)
        c = _census(oracle, vol, P.oracle_tree(oracle, name, shape, 256, 2, 0))
        assert c["busy"] == 1 and c["skipped"] + c["filled"] == (1 << (depth[shape] - 12)) - 1 and c["filled"] >= 1, (shape, c)


# ---------------------------------------------------------------- tolerance ----
_TOL = P.tolerance_cases()


@pytest.mark.parametrize("shape,tol,cases", _TOL, ids=["%s-tol%d%s" % (P.sid(s), t, "-ep%d-v%d" % c[0][:2] if s == P.S19 else "")
                                                       for s, t, c in _TOL])
def test_tolerance_ladder(vr, oracle, monkeypatch, tmp_path, shape, tol, cases):
    if shape == P.IDX64:
        monkeypatch.setenv("VRHIP_FORCE_IDX64", "1")            # 64-bit token offsets (read when a set is created)
    for ep, variant, name in cases:
        vol = P.volume(name, shape)
        ref = P.oracle_tree(oracle, name, shape, tol, ep, variant)
        bs = _full_check(vr, oracle, vol, ref, tol, ep, variant, tmp_path)
        if name.startswith("const") and variant == 0:
            _switched_handles_agree(vr, oracle, vol, ref, tol, ep, bs)


# ---------------------------------------------------------------- epochs ----
_EP = P.epoch_cases()


@pytest.mark.parametrize("shape,ep,cases", _EP, ids=["%s-ep%d%s" % (P.sid(s), e, "-tol%d-v%d" % c[0][:2] if s == P.S19 else "")
                                                     for s, e, c in _EP])
def test_epoch_ladder(vr, oracle, tmp_path, shape, ep, cases):
    """Levels that stop at different epochs long before the limit, the leafless build's last-epoch logic and a host
    loop that keeps launching on levels gone inactive: the streams, num_reverts and the statistics are the oracle's."""
    for tol, variant, name in cases:
        ref = P.oracle_tree(oracle, name, shape, tol, ep, variant)
        _full_check(vr, oracle, P.volume(name, shape), ref, tol, ep, variant, tmp_path)


def test_set_max_epochs_refuses_more_than_the_ceiling(vr, oracle):
    """VR_ERR_UNSUPPORTED above VR_MAX_EPOCHS, and the set keeps its setting (nothing is built with such a value)."""
    vol = P.volume("rm_like", P.S12)
    bs = vr.BrickSet(1, (16, 16, 16), 1, 2)
    for e in (1025, 2 ** 31 - 1):
        with pytest.raises(vr.VrError) as ei:
            bs.set_max_epochs(e)
        assert ei.value.status == -7
    with pytest.raises(vr.VrError) as ei:
        vr.BrickSet(1, (16, 16, 16), 1, 2 ** 31 - 1)
    assert ei.value.status == -7
    bs.build(vol.copy())
    assert bs.info(0)["max_epochs"] == 2
    assert np.array_equal(bs.tree(0), P.oracle_tree(oracle, "rm_like", P.S12, 1, 2, 0).tree)
    bs.set_max_epochs(1024)                                    # the ceiling itself is a setting like any other


# ---------------------------------------------------------------- a root-only stream from the encoder ----
def _every_switch_every_cut(bs, shape, n, want):
    """want[c]: the oracle's voxels of all n bricks at cut c, for every cut 0 .. M"""
    for name in (None, "decode_quad", "decode_fine_v1", "decode_walk"):
        if name:
            bs.set_switch(name, 1)
        for c, w in enumerate(want):
            got = bs.decode(cut_depth=c).cpu().numpy().reshape((n,) + shape)
            assert np.array_equal(got, w), (name, c)
        assert np.array_equal(bs.decode().cpu().numpy().reshape((n,) + shape), want[-1]), name
        if name:
            bs.set_switch(name, 0)


@pytest.mark.parametrize("tol", [256, 40000])
@pytest.mark.parametrize("shape", [P.S12, P.S15, P.S19], ids=P.sid)
def test_root_only_stream_from_the_encoder(vr, oracle, shape, tol):
    """No level loop and a tolerance no leaf error reaches: a brick that is not constant becomes a one-token stream.
    In a fused build every 4096-leaf block is then dead without the brick being a constant one, so k_block_alive,
    k_index12, k_concat12, the compaction and the decode index serve a root-only tree that only foreign streams had
    shown the decoders before.  One brick alone, and five such bricks of different data -- noise, smooth, constant --
    in one set (with no level loop and this tolerance every brick of a set is root-only)."""
    z, y, x = shape
    vol = P.volume("noise", shape)
    ref = P.oracle_tree(oracle, "noise", shape, tol, 0, 0)
    assert ref.numActiveNodes == 1 and int(vol.min()) != int(vol.max())
    M = ref.maxTreeDepth
    for compaction in (0, 1):
        bs = vr.BrickSet(1, (x, y, z), tol, 0)
        bs.set_compaction(compaction)
        bs.build(vol.copy())
        assert bs.info(0)["num_active_nodes"] == 1
        assert np.array_equal(bs.tree(0), ref.tree) and list(bs.distance_map(0)) == list(ref.distanceMap), compaction
    want = [ref.levelCutProgressive(c)[None] for c in range(M + 1)]
    assert np.array_equal(want[M][0], ref.levelCut())
    _every_switch_every_cut(bs, shape, 1, want)
    # five bricks: ordinary data, constants, the noise brick in the middle
    names = [("rm_like", 0), None, ("noise", 0), ("mixed", 1), None]
    vols = [np.full(shape, 77 if i == 1 else 255, np.uint8) if n is None else P.volume(n[0], shape, n[1]) for i, n in enumerate(names)]
    refs = [oracle.OracleTree(v.copy(), tolerance=tol, max_epochs=0).build() for v in vols]
    five = vr.BrickSet(5, (x, y, z), tol, 0).build(np.stack(vols))
    for b, r in enumerate(refs):
        assert five.info(b)["num_active_nodes"] == r.numActiveNodes == 1, b
        assert np.array_equal(five.tree(b), r.tree) and list(five.distance_map(b)) == list(r.distanceMap), b
    assert np.array_equal(five.tree(2), ref.tree)
    want5 = [np.stack([r.levelCutProgressive(c) for r in refs]) for c in range(M + 1)]
    _every_switch_every_cut(five, shape, 5, want5)
    D = ref.origTreeDepth
    cuts = [M, 0, D - 3, -1, D]
    base = five.decode(cut_depth=0).clone()
    lod = five.decode_lod(np.array(cuts, np.int32), out=base.clone()).cpu().numpy().reshape((5,) + shape)
    for b, c in enumerate(cuts):
        assert np.array_equal(lod[b], want5[0][b] if c < 0 else want5[c][b]), (b, c)


# ---------------------------------------------------------------- one handle across the extremes ----
@pytest.mark.parametrize("variant", [0, 2], ids=["kd", "mid"])
@pytest.mark.parametrize("shape", [P.S15, P.S19], ids=P.sid)
def test_one_handle_across_the_extremes(vr, oracle, shape, variant):
    """set_error_tolerance / set_max_epochs move one handle through (1, 2) -> (40000, 0) -> (13, 40) -> (256, 1) ->
    (1, 2): across the leafless / storing switch of the encoder's buffers at max_epochs 0 <-> >= 1, with a stream that
    shrinks to one token and grows back.  Every build equals a fresh handle's and the oracle's."""
    z, y, x = shape
    vol = P.volume("rm_like", shape)
    bs = vr.BrickSet(1, (x, y, z), 1, 2, variant)
    for tol, ep in ((1, 2), (40000, 0), (13, 40), (256, 1), (1, 2)):
        bs.set_error_tolerance(tol)
        bs.set_max_epochs(ep)
        bs.build(vol.copy())
        ref = P.oracle_tree(oracle, "rm_like", shape, tol, ep, variant)
        fresh = _build_checked(vr, oracle, vol, ref, tol, ep, variant)
        assert _outputs(bs, shape) == _outputs(fresh, shape), (tol, ep)
        if variant == 2:
            assert np.array_equal(bs.tree_range(0), ref.tree_range), (tol, ep)
            assert list(bs.distance_map_range(0)) == list(ref.distanceMap_range), (tol, ep)
            assert np.array_equal(bs.decode_range().cpu().numpy().reshape(shape), ref.levelCutRange(None)), (tol, ep)
        assert np.array_equal(bs.decode().cpu().numpy().reshape(shape), ref.levelCut()), (tol, ep)
    assert P.oracle_tree(oracle, "rm_like", shape, 40000, 0, variant).numActiveNodes == 1


# ---------------------------------------------------------------- known answers ----
class _Built:
    """a built set with the accessors codec_params.known_record reads"""

    def __init__(self, bs, shape, midrange):
        self.numActiveNodes = bs.info(0)["num_active_nodes"]
        self.tree = bs.tree(0)
        self.tree_range = bs.tree_range(0) if midrange else None
        self._dec = bs.decode().cpu().numpy().reshape(shape)

    def levelCut(self):
        return self._dec


@pytest.mark.parametrize("case", P.known_answers(),
                         ids=lambda c: "%s-%s-tol%d-ep%d-%s" % (c["volume"], P.sid(tuple(c["shape"])), c["tolerance"], c["max_epochs"], c["variant"]))
def test_gpu_reproduces_known_answers(vr, oracle, case):
    """The answers recorded from the reference codec itself (oracle/gen_codec_param_answers.py)."""
    name, seed, shape = case["volume"], case["seed"], tuple(case["shape"])
    tol, ep, vname = case["tolerance"], case["max_epochs"], case["variant"]
    z, y, x = shape
    bs = vr.BrickSet(1, (x, y, z), tol, ep, P.VARIANTS[vname]).build(P.volume(name, shape, seed))
    assert P.known_record(oracle, _Built(bs, shape, vname == "mid"), name, seed, shape, tol, ep, vname) == case
