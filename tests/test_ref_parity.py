"""The oracle against the reference codec itself (oracle/_ref/libvkref.so, built in place from the upstream sources by
oracle/Makefile's `ref` target): CPU only, bit-exact.

The oracle (oracle/kdtree_oracle.c) and the HIP kernels were written from the same reading of the reference; these
tests take that reading out of the loop.  They also regenerate every known answer of tests/golden/ from the reference,
so the golden data has a committed generator."""
import json
import os

import numpy as np
import pytest

GOLD = os.path.join(os.path.dirname(__file__), "golden")
KA = json.load(open(os.path.join(GOLD, "survey_known_answers.json")))


@pytest.fixture(scope="module")
def O(oracle):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref/libvkref.so is not built: no reference sources at %s" % oracle.ref_dir())
    return oracle


# -- known answers: the reference regenerates the golden data

def _ka_param(c):
    return pytest.param(c, id="n%d" % c["n"], marks=[pytest.mark.slow] if c.get("slow") else [])


@pytest.mark.parametrize("case", [_ka_param(c) for c in KA["volume_kdtree"]])
def test_ref_reproduces_volume_kdtree_known_answers(O, case, tmp_path):
    vol = O.gen_sphere(case["n"], case["noise_mask"])
    r = O.RefTree(vol.copy(), tolerance=case["tolerance"], max_epochs=case["max_epochs"]).build()
    if "origTreeDepth" in case:
        assert r.origTreeDepth == case["origTreeDepth"] and r.maxTreeDepth == case["maxTreeDepth"]
    if "numActiveNodes" in case:
        assert r.numActiveNodes == case["numActiveNodes"] and len(r.tree) == case["tree_bytes"]
    if "distanceMap" in case:
        assert list(map(int, r.distanceMap)) == case["distanceMap"]
    assert "%016x" % O.fnv1a64(r.tree) == case["tree_fnv"]
    out = r.levelCut()
    if "voxels_fnv" in case:
        assert "%016x" % O.fnv1a64(out) == case["voxels_fnv"]
    if "decoded_max_error" in case:
        assert int(np.abs(out.astype(np.int32) - vol).max()) == case["decoded_max_error"]
    if "saved_file" in case:
        p = str(tmp_path / "r.bin")
        r.save(p)
        gold = open(os.path.join(GOLD, case["saved_file"]), "rb").read()
        assert len(gold) == case["saved_file_bytes"] and open(p, "rb").read() == gold
        u = O.RefTree.open(os.path.join(GOLD, case["saved_file"]))
        assert len(u.tree) == case["tree_bytes"] + 8           # open() over-allocates by 8 bytes (C-6)
        assert np.array_equal(u.levelCut(), out)


@pytest.mark.parametrize("case", KA["mid_range_tree"], ids=lambda c: "n%d" % c["n"])
def test_ref_reproduces_mid_range_tree_known_answers(O, case):
    vol = O.gen_sphere(case["n"], case["noise_mask"])
    r = O.RefTree(vol.copy(), tolerance=case["tolerance"], max_epochs=case["max_epochs"], midrange=True).build()
    assert r.numActiveNodes == case["numActiveNodes"]
    assert "%016x" % O.fnv1a64(r.tree) == case["tree_fnv"]
    assert "%016x" % O.fnv1a64(r.tree_range) == case["tree_range_fnv"]
    packed = r.convertToByteArray()
    assert len(packed) == case["packed_bytes"] and "%016x" % O.fnv1a64(packed) == case["packed_fnv"]
    assert int(np.abs(r.levelCut().astype(np.int32) - vol).max()) == case["decoded_max_error"]


@pytest.mark.slow
def test_ref_reproduces_sphere_n0_256(O):
    """The survey's 256^3 sphere_n0 entry, at the tolerance / epochs test_gpu_codec.py checks it with (1, 2)."""
    case = KA["survey_256_sphere_n0"]
    vol = O.gen_sphere(256, 0)
    r = O.RefTree(vol.copy(), tolerance=1, max_epochs=2).build()
    assert r.numActiveNodes == case["numActiveNodes"] and len(r.tree) == case["tree_bytes"]
    assert int(np.abs(r.levelCut().astype(np.int32) - vol).max()) == case["decoded_max_error"]


# -- the seeded matrix: oracle against reference

TOL_EP = [(t, e) for t in (0, 1, 2, 4, 6, 12) for e in (0, 1, 2, 5)]

CUBES = [(n, n, n) for n in (1, 2, 4, 8, 16, 32, 64)]
ANISOTROPIC = [(8, 16, 32), (32, 16, 8), (16, 4, 64), (4, 64, 16), (2, 8, 128)]
# test_gpu_codec.py::test_general_extents_match_oracle's extents, and the odd ones of the first scratch sweep
GENERAL = [(12, 6, 5), (40, 16, 24), (48, 64, 96), (3, 1, 1), (7, 9, 2), (2, 2, 2048), (5, 6, 12), (1, 1, 3),
           (2, 9, 7)]


def sphere(shape, noise_mask, rng):
    """A sphere field on any extents ([z][y][x]); for cubes, the survey's LCG generator."""
    z, y, x = shape
    if x == y == z:
        from oracle import oracle
        return oracle.gen_sphere(x, noise_mask, seed=int(rng.integers(1, 1 << 31)))
    g = np.meshgrid(*[(np.arange(s) + 0.5) / s - 0.5 for s in shape], indexing="ij")
    r = np.sqrt(sum(a * a for a in g)) * 2.0
    v = np.clip(255.0 * (1.0 - r), 0, 255).astype(np.int64)
    if noise_mask:
        v = v + (rng.integers(0, 256, shape) & noise_mask)
    return np.clip(v, 0, 255).astype(np.uint8)


def gradient(shape, rng):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    a, b, c = (int(k) for k in rng.integers(1, 41, 3))
    return ((a * x + b * y + c * z + int(rng.integers(0, 256))) % 256).astype(np.uint8)


def step(shape, rng):
    axis = int(rng.integers(0, 3))
    idx = np.arange(shape[axis]).reshape([-1 if i == axis else 1 for i in range(3)])
    at = int(rng.integers(0, shape[axis] + 1))
    return np.broadcast_to(np.where(idx < at, 0, 255), shape).astype(np.uint8)


def checker(shape, rng):
    z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    k = int(rng.integers(1, 4))
    lo, hi = sorted(int(v) for v in rng.integers(0, 256, 2))
    return np.where(((x // k + y // k + z // k) & 1) == 1, hi, lo).astype(np.uint8)


GENERATORS = {
    "sphere_n3": lambda s, r: sphere(s, 7, r),
    "sphere_n0": lambda s, r: sphere(s, 0, r),
    "noise": lambda s, r: r.integers(0, 256, s, dtype=np.uint8),
    "noise4": lambda s, r: r.integers(0, 4, s, dtype=np.uint8),
    "gradient": gradient,
    "step": step,
    "checker": checker,
    "zeros": lambda s, r: np.zeros(s, np.uint8),
    "full255": lambda s, r: np.full(s, 255, np.uint8),
    "const": lambda s, r: np.full(s, int(r.integers(1, 255)), np.uint8),
}


def compare(O, vol, tol, ep, midrange, tmp_path, what):
    """Everything the two implementations expose, bit-exact; returns (oracle tree, reference tree)."""
    o = O.OracleTree(vol.copy(), tolerance=tol, max_epochs=ep, midrange=midrange, guarded=midrange).build()
    r = O.RefTree(vol.copy(), tolerance=tol, max_epochs=ep, midrange=midrange).build()
    assert (o.origTreeDepth, o.maxTreeDepth) == (r.origTreeDepth, r.maxTreeDepth), what
    assert o.numActiveNodes == r.numActiveNodes, what
    assert np.array_equal(o.distanceMap, r.distanceMap), what
    assert np.array_equal(o.tree, r.tree), what
    if midrange:
        assert np.array_equal(o.distanceMap_range, r.distanceMap_range), what
        assert np.array_equal(o.tree_range, r.tree_range), what
        assert np.array_equal(o.convertToByteArray(), r.convertToByteArray()), what
    assert np.array_equal(o.levelCut(), r.levelCut()), what
    po, pr = str(tmp_path / "o.bin"), str(tmp_path / "r.bin")
    o.save(po)
    r.save(pr)
    assert open(po, "rb").read() == open(pr, "rb").read(), what
    return o, r


def run_matrix(O, shapes, midrange, seed, tmp_path, generators=None):
    rng = np.random.default_rng(seed)
    k = int(rng.integers(0, len(TOL_EP)))
    for shape in shapes:
        for name in generators or GENERATORS:
            tol, ep = TOL_EP[k % len(TOL_EP)]
            k += 5                     # coprime with 24: every pair comes round for every generator
            vol = GENERATORS[name](shape, rng)
            compare(O, vol, tol, ep, midrange, tmp_path, (shape, name, tol, ep, "mid" if midrange else "kd"))


@pytest.mark.parametrize("midrange", [False, True], ids=["kd", "mid"])
@pytest.mark.parametrize("shape", CUBES + ANISOTROPIC + GENERAL, ids=lambda s: "%dx%dx%d" % s)
def test_oracle_matches_ref(O, shape, midrange, tmp_path):
    run_matrix(O, [shape], midrange, 1000 + 7 * sum(shape) + shape[0], tmp_path)


@pytest.mark.parametrize("midrange", [False, True], ids=["kd", "mid"])
def test_oracle_matches_ref_128(O, midrange, tmp_path):
    run_matrix(O, [(128, 128, 128)], midrange, 128, tmp_path, ["sphere_n3", "gradient", "step", "const"])


@pytest.mark.parametrize("midrange", [False, True], ids=["kd", "mid"])
def test_every_tolerance_epoch_pair(O, midrange, tmp_path):
    """Each (tolerance, epochs) pair on a noisy and a smooth volume, so no pair rests on the matrix's rotation."""
    rng = np.random.default_rng(24)
    noisy = rng.integers(0, 256, (8, 16, 16), dtype=np.uint8)
    smooth = sphere((16, 16, 16), 3, rng)
    for tol, ep in TOL_EP:
        for vol in (noisy, smooth):
            compare(O, vol, tol, ep, midrange, tmp_path, (vol.shape, tol, ep))


# -- files written by one side, opened by the other

@pytest.mark.parametrize("shape", [(16, 16, 16), (12, 6, 5), (8, 16, 32), (2, 2, 2048)], ids=lambda s: "%dx%dx%d" % s)
def test_cross_open(O, shape, tmp_path):
    rng = np.random.default_rng(sum(shape))
    for name, tol, ep in (("sphere_n3", 1, 2), ("noise", 2, 5), ("step", 0, 1), ("const", 1, 0)):
        vol = GENERATORS[name](shape, rng)
        o, r = compare(O, vol, tol, ep, False, tmp_path, (shape, name))
        want = r.levelCut()
        po, pr = str(tmp_path / "o.bin"), str(tmp_path / "r.bin")
        ro = O.RefTree.open(po)                          # the reference reads the oracle's file
        assert ro.numActiveNodes == o.numActiveNodes and ro.maxTreeDepth == o.maxTreeDepth
        assert np.array_equal(ro.levelCut(), want), (shape, name)
        orr = O.OracleTree.open(pr)                      # the oracle reads the reference's file
        assert np.array_equal(orr.tree, ro.tree), (shape, name)   # both over-allocate alike (C-6)
        assert np.array_equal(orr.levelCut(), want), (shape, name)


def test_cross_open_midrange(O, tmp_path):
    """MidRangeTree::open reads its own files back shifted (M.cpp:815); the oracle's open_midrange restates that
    reading, so both sides must come back with the same (shifted) streams."""
    vol = O.gen_sphere(16, 7)
    o, r = compare(O, vol, 1, 1, True, tmp_path, "mid")
    u = O.OracleTree.open_midrange(str(tmp_path / "r.bin"))
    v = O.RefTree.open(str(tmp_path / "o.bin"), midrange=True)
    assert (u.numActiveNodes, u.maxTreeDepth) == (v.numActiveNodes, v.maxTreeDepth)
    assert np.array_equal(u.distanceMap, v.distanceMap) and np.array_equal(u.distanceMap_range, v.distanceMap_range)
    assert np.array_equal(u.tree, v.tree) and np.array_equal(u.tree_range, v.tree_range)
