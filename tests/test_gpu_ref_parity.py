"""GPU parity with no oracle in the loop: the HIP codec against the reference codec itself (oracle/_ref/libvkref.so,
built by oracle/Makefile's `ref` target; see tests/test_ref_parity.py for the oracle's side).

Bit-exact, at the shapes where the kernels branch: the fused brick kernels, the bench's brick, the table-driven
single-tree path, constant-brick closed forms sharing launches with dense bricks, the MidRange streams and the 4-bit
packing, files crossing between the two implementations, and one handle rebuilt with and without lazy compaction.
Only the built library is loaded here, never the reference's sources; without it these tests skip."""
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def O(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref/libvkref.so is not built (build() makes it where the reference sources exist)")
    return oracle


def field(shape, seed=3):
    """A smooth surface with a little noise (long grown branches next to pruned slabs)."""
    rng = np.random.default_rng(seed)
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    h = shape[0] / 2 + 3 * np.sin(x * 0.4) + 2 * np.cos(y * 0.23)
    v = 128 + 120 * np.tanh((z - h) / 3.0) + rng.integers(0, 3, shape)
    return np.clip(v, 0, 255).astype(np.uint8)


def ball(shape, noise_mask=7, seed=5):
    rng = np.random.default_rng(seed)
    g = np.meshgrid(*[(np.arange(s) + 0.5) / s - 0.5 for s in shape], indexing="ij")
    v = np.clip(255.0 * (1.0 - 2.0 * np.sqrt(sum(a * a for a in g))), 0, 255).astype(np.int64)
    return np.clip(v + (rng.integers(0, 256, shape) & noise_mask), 0, 255).astype(np.uint8)


def noise(shape, seed=7, hi=256):
    return np.random.default_rng(seed).integers(0, hi, shape, dtype=np.uint8)


def check_brick(bs, b, ref, dec, what):
    """What check_case (test_gpu_codec.py) asserts that the reference exposes, for brick b of a set."""
    info = bs.info(b)
    assert (info["orig_tree_depth"], info["max_tree_depth"]) == (ref.origTreeDepth, ref.maxTreeDepth), what
    assert list(bs.distance_map(b)) == list(ref.distanceMap), what
    assert info["num_active_nodes"] == ref.numActiveNodes, what
    assert np.array_equal(bs.tree(b), ref.tree), what
    assert np.array_equal(dec, ref.levelCut()), what


def check_set(vr, O, vols, tol, ep, what, midrange=False):
    """All vols (same shape) built as one BrickSet; each brick against its own reference tree."""
    z, y, x = vols[0].shape
    bs = vr.BrickSet(len(vols), (x, y, z), tol, ep, 2 if midrange else 0)
    bs.build(np.stack(vols))
    dec = bs.decode().cpu().numpy().reshape((len(vols), z, y, x))
    refs = []
    for b, v in enumerate(vols):
        ref = O.RefTree(v.copy(), tolerance=tol, max_epochs=ep, midrange=midrange).build()
        w = (what, tol, ep, b)
        check_brick(bs, b, ref, dec[b], w)
        if midrange:
            assert list(bs.distance_map_range(b)) == list(ref.distanceMap_range), w
            assert np.array_equal(bs.tree_range(b), ref.tree_range), w
            assert np.array_equal(bs.packed4(b), ref.convertToByteArray()), w
        refs.append(ref)
    return bs, refs


@pytest.mark.parametrize("shape", [(8, 16, 16), (16, 16, 16), (16, 32, 32), (32, 32, 32), (64, 64, 64),
                                   (256, 16, 16), (16, 16, 256)], ids=lambda s: "%dx%dx%d" % s[::-1])
def test_fused_bricks_match_ref(vr, O, shape):
    for tol, ep in ((1, 2), (0, 5), (6, 1), (2, 0)):
        check_set(vr, O, [field(shape), noise(shape), ball(shape)], tol, ep, shape)


def test_bench_bricks_match_ref(vr, O):
    """Two bricks of the bench's 256 x 256 x 128 shape and field, tolerance 1, epochs 2."""
    import sys
    import torch
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    vox = bench.make_volume_gpu(torch, (256, 256, 256), (256, 256, 128), seed=12345, kind="rm_volume")
    host = vox.cpu().numpy()
    assert host.shape == (2, 128, 256, 256) and host[0].tobytes() != host[1].tobytes()
    check_set(vr, O, [host[0], host[1]], 1, 2, "bench")


@pytest.mark.parametrize("shape", [(12, 6, 5), (2048, 2, 2), (48, 64, 96), (96, 256, 256)],
                         ids=lambda s: "%dx%dx%d" % s[::-1])
def test_single_tree_path_matches_ref(vr, O, shape):
    """Extents off the fused kernels' grid: the table-driven single-tree path."""
    cases = [(field(shape), 1, 2), (ball(shape, 3), 2, 5)]
    if np.prod(shape) <= (1 << 20):
        cases.append((noise(shape, 11), 0, 1))
    for vol, tol, ep in cases:
        check_set(vr, O, [vol], tol, ep, shape)


@pytest.mark.parametrize("shape", [(16, 16, 16), (32, 64, 64)], ids=lambda s: "%dx%dx%d" % s[::-1])
def test_mixed_brick_set_matches_ref(vr, O, shape):
    """Constant bricks (closed forms) sharing launches with noise and sphere bricks."""
    vols = [np.zeros(shape, np.uint8), noise(shape, 1), np.full(shape, 77, np.uint8), ball(shape),
            np.full(shape, 255, np.uint8), noise(shape, 2, hi=4), ball(shape, 0)]
    for tol, ep in ((1, 2), (0, 2), (4, 5), (3, 0)):
        check_set(vr, O, vols, tol, ep, shape)


@pytest.mark.parametrize("shape", [(16, 16, 16), (32, 32, 32), (12, 6, 5), (16, 32, 64)], ids=lambda s: "%dx%dx%d" % s[::-1])
def test_midrange_matches_ref(vr, O, shape):
    vols = [ball(shape), noise(shape, 3), np.full(shape, 9, np.uint8), field(shape)]
    pow2 = all(s & (s - 1) == 0 for s in shape)
    for tol, ep in ((1, 1), (1, 2), (0, 5), (6, 0)):
        if pow2:
            check_set(vr, O, vols, tol, ep, shape, midrange=True)
        else:                        # general extents: one brick per set, as test_general_extents_match_oracle
            for v in vols:
                check_set(vr, O, [v], tol, ep, shape, midrange=True)


@pytest.mark.parametrize("shape", [(16, 32, 128), (64, 128, 128), (128, 16, 16)], ids=lambda s: "%dx%dx%d" % s[::-1])
def test_files_cross_between_hip_and_ref(vr, O, shape, tmp_path):
    """A HIP-saved file read by the reference's open() + levelCut; a reference-saved file read by the HIP open() and
    decoded by the default kernel and by each debugging switch's kernel."""
    z, y, x = shape
    for vol, tol, ep in ((field(shape), 1, 2), (ball(shape, 3), 2, 5)):
        ref = O.RefTree(vol.copy(), tolerance=tol, max_epochs=ep).build()
        want = ref.levelCut()
        bs = vr.BrickSet(1, (x, y, z), tol, ep).build(vol.copy())
        got = bs.decode().cpu().numpy().reshape(shape)
        assert np.array_equal(got, want), shape
        hp, rp = str(tmp_path / "hip.bin"), str(tmp_path / "ref.bin")
        bs.save(hp)
        ref.save(rp)
        assert open(hp, "rb").read() == open(rp, "rb").read(), shape
        back = O.RefTree.open(hp)
        assert np.array_equal(back.levelCut(), got), shape
        fs = vr.BrickSet.open(rp)
        assert fs.info(0)["num_active_nodes"] == ref.numActiveNodes
        assert np.array_equal(fs.decode().cpu().numpy().reshape(shape), want), (shape, "default")
        for sw in ("decode_walk", "decode_fine_v1", "decode_quad"):
            fs.set_switch(sw, 1)
            dec = fs.decode().cpu().numpy().reshape(shape)
            fs.set_switch(sw, 0)
            assert np.array_equal(dec, want), (shape, sw)


@pytest.mark.parametrize("compact", [True, False], ids=["compact_on_build", "compact_lazily"])
def test_one_handle_rebuilt_matches_ref(vr, O, compact, tmp_path):
    """Sphere, uniform noise, sphere again through one handle: the contiguous stream regrows for the noise and the
    lazy compaction runs on the first tree read after each build."""
    shape = (32, 64, 64)
    z, y, x = shape
    bs = vr.BrickSet(1, (x, y, z), 1, 2)
    bs.set_compaction(compact)
    for i, vol in enumerate((ball(shape), noise(shape, 21), ball(shape, 7, seed=6))):
        bs.build(vol.copy())
        ref = O.RefTree(vol.copy(), tolerance=1, max_epochs=2).build()
        p, q = str(tmp_path / "h.bin"), str(tmp_path / "r.bin")
        ref.save(q)
        if i == 1:                   # the first read of the stream after this build is save(), else the tree bytes
            bs.save(p)
        assert np.array_equal(bs.tree(0), ref.tree), (compact, i)
        bs.save(p)
        assert open(p, "rb").read() == open(q, "rb").read(), (compact, i)
        check_brick(bs, 0, ref, bs.decode().cpu().numpy().reshape(shape), (compact, i))
