"""k_prune_emit12's upper levels (depths D-12 .. D-5 by one wave in registers), its top-down spine, block scan and code
write-back, on the cases of tests/prunecases.py -- planted subtrees that the bottom-up rule prunes at
every in-block level beside noisy siblings; test_prune_chain_cpu.py asserts on the oracle that the cases hold every class
of node and thread the kernel distinguishes.

Every case is compared bit for bit with the CPU oracle and with a fresh handle: the stream bytes, info(b)
(num_active_nodes, tree_bytes, max_tree_depth), the distance map, and the decoded voxels at the full cut and at cut
D-6 (the decode index k_prune_emit12 writes: idxOff, fineIdx).  The same cases go through
  * a MidRangeTree set (variant 2): the RANGE instantiations, both streams against the oracle's MidRangeTree;
  * a handle with `no_uniform_blocks` on: constant boxes take the full path through the same code;
  * max_epochs 0, which builds with a leaf level: the non-leafless instantiations (k_prune_emit12<., false>).

Shapes are the smallest with the path: 16x16x16 (D = 12, one box, every in-block level), 32x32x16 (D = 14, four boxes),
32x32x32 (D = 15)."""
import numpy as np
import pytest

import prunecases as pc

pytestmark = pytest.mark.gpu

IDS = ["16x16x16", "32x32x16", "32x32x32"]


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


_REFS = {}


def _refs(O, shape, tol, ep, midrange):
    key = (shape, tol, ep, midrange)
    if key not in _REFS:
        vols, _ = pc.case(O, shape, tol, ep)
        _REFS[key] = [O.OracleTree(v.copy(), tolerance=tol, max_epochs=ep, midrange=midrange).build() for v in vols]
    return _REFS[key]


def _make(vr, n, shape, tol, ep, midrange=False, switches=()):
    bs = vr.BrickSet(n, shape[::-1], tol, ep, variant=2) if midrange else vr.BrickSet(n, shape[::-1], tol, ep)
    for name in switches:
        bs.set_switch(name, 1)
    return bs


def _outputs(bs, n, shape, midrange):
    D = pc.depth_of(shape)
    out = dict(dec=bs.decode().cpu().numpy().reshape(n, *shape), cut=bs.decode(cut_depth=D - 6).cpu().numpy().reshape(n, *shape))
    if midrange:
        out["dec_range"] = bs.decode_range().cpu().numpy().reshape(n, *shape)
    for b in range(n):
        out["tree%d" % b] = bs.tree(b)
        out["dmap%d" % b] = bs.distance_map(b)
        info = bs.info(b)
        out["info%d" % b] = np.array([info[k] for k in sorted(info)], np.float64)
        if midrange:
            out["treeR%d" % b] = bs.tree_range(b)
            out["dmapR%d" % b] = bs.distance_map_range(b)
    return out


def _same(a, b, what):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), (k, what)


def _against_oracle(bs, refs, shape, midrange, what):
    n, D = len(refs), pc.depth_of(shape)
    out = _outputs(bs, n, shape, midrange)
    for b, ref in enumerate(refs):
        info = bs.info(b)
        assert info["num_active_nodes"] == ref.numActiveNodes, (b, what)
        assert info["tree_bytes"] == len(ref.tree), (b, what)
        assert info["max_tree_depth"] == ref.maxTreeDepth, (b, what)
        assert list(out["dmap%d" % b]) == list(ref.distanceMap), (b, what)
        assert np.array_equal(out["tree%d" % b], ref.tree), (b, what)
        assert np.array_equal(out["dec"][b], ref.levelCut()), (b, what)
        assert np.array_equal(out["cut"][b], ref.levelCutProgressive(D - 6)), (b, what)
        if midrange:
            assert list(out["dmapR%d" % b]) == list(ref.distanceMap_range), (b, what)
            assert np.array_equal(out["treeR%d" % b], ref.tree_range), (b, what)
            assert np.array_equal(out["dec_range"][b], ref.levelCutRange()), (b, what)
    return out


def _run(vr, O, shape, tol, ep, midrange=False, switches=()):
    vols, _ = pc.case(O, shape, tol, ep)
    refs = _refs(O, shape, tol, ep, midrange)
    what = (shape, tol, ep, midrange, switches)
    data = np.stack(vols)
    bs = _make(vr, len(vols), shape, tol, ep, midrange, switches).build(data)
    out = _against_oracle(bs, refs, shape, midrange, what)
    # a second build on the same handle and a fresh handle give the same bytes
    _same(out, _outputs(bs.build(data), len(vols), shape, midrange), ("rebuilt",) + what)
    _same(out, _outputs(_make(vr, len(vols), shape, tol, ep, midrange, switches).build(data), len(vols), shape, midrange),
          ("fresh",) + what)
    return out


@pytest.mark.parametrize("tol,ep", pc.PARAMS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_default_handle(vr, oracle, shape, tol, ep):
    """k_prune_emit12<false, true> (max_epochs >= 1) and <false, false> (max_epochs 0: the API's way to a build with a
    leaf level); constant boxes go to k_prune_emit12_const, everything else through the upper levels under test."""
    _run(vr, oracle, shape, tol, ep)


@pytest.mark.parametrize("tol,ep", pc.PARAMS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_constant_boxes_on_the_full_path(vr, oracle, shape, tol, ep):
    """`no_uniform_blocks`: planted boxes and sub-boxes that are constant run through the upper levels too, and the
    result equals the default handle's."""
    out = _run(vr, oracle, shape, tol, ep, switches=("no_uniform_blocks",))
    vols, _ = pc.case(oracle, shape, tol, ep)
    _same(out, _outputs(_make(vr, len(vols), shape, tol, ep).build(np.stack(vols)), len(vols), shape, False), "default handle")
    _run(vr, oracle, shape, tol, ep, switches=("no_skip_blocks",))


@pytest.mark.parametrize("tol,ep", pc.PARAMS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=IDS)
def test_midrange_tree(vr, oracle, shape, tol, ep):
    """Variant 2: k_prune_emit12<true, .> meets the codes the first launch has pruned (code 3 on entry); both streams
    against the oracle's MidRangeTree, and against the build with `no_uniform_blocks`."""
    out = _run(vr, oracle, shape, tol, ep, midrange=True)
    _same(out, _run(vr, oracle, shape, tol, ep, midrange=True, switches=("no_uniform_blocks",)), "no_uniform_blocks")
