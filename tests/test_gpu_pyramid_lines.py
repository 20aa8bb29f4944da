"""k_pyramid12_lines -- the pyramid's bottom twelve levels by eight x-adjacent 16-voxel-wide boxes per workgroup --
against the CPU oracle and against the same data built under the `pyramid_boxes` switch (k_pyramid12, one box per
workgroup).  Stream bytes, distance maps, info() and the decoded volume are compared bit for bit.

Which kernel a shape gets is not assumed: tests/pyr12_plan_main.cpp, a stand-alone program linked against
volumerenderer_amd/csrc/host_plan.cpp and built under the address and undefined-behaviour sanitizers, checks the rule
over every power-of-two shape and reports the plan of each shape used here (`plans`).  The line kernel needs boxes 16
voxels wide (four x splits among the twelve deepest levels) in a brick at least 128 wide.  By the split rule (depth d
splits axis d % 3 while that axis is longer than one voxel) the smallest such bricks are 128x64x64 (boxes 16x16x16,
one group per row of boxes), 128x32x128 (16x8x32: ay != az), 128x32x256 (16x4x64) and, with two groups per row,
256x128x128.  The bricks 128x16x16, 256x16x16, 128x32x16 and 128x16x32 are 128 wide and more but split x six or five
times down there (boxes 64x8x8, 32x16x8, 32x8x16): they keep k_pyramid12, as 64x64x64 and 32x32x32 do, and are built
here all the same -- the switch must make no difference to them either.

A group's contents (`_grouped`): 0, 1, 7 or 8 of its eight boxes constant, the number changing from group to group
and the constant boxes' places rotating, so neighbours of different values stand side by side; the others are noise
of two kinds.  The corner cases put one deviating byte into a constant box at the first or last byte of its first or
last row: the first and last of the eight lanes (of waves 0 and 3) that hold the box."""
import os
import subprocess

import numpy as np
import pytest

from test_gpu_const_boxes import MIX_VALUES, _refs, _outputs, _same, _against_oracle, _make, _noise_box, _census, _add
from test_gpu_const_boxes import vr  # noqa: F401  (the module's fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")

# (z, y, x)
OLD_PATH = [(16, 16, 128), (16, 16, 256), (16, 32, 128), (32, 16, 128), (64, 64, 64), (32, 32, 32)]
L444 = (64, 64, 128)            # D = 19, boxes 16x16x16, 16 groups, one per row of boxes: the smallest brick with the kernel
L435 = (128, 32, 128)           # D = 19, boxes 16x8x32
L426 = (256, 32, 128)           # D = 20, boxes 16x4x64
L2ROW = (128, 128, 256)         # D = 22, two groups per row of boxes
BENCH = (128, 256, 256)         # the bench's brick, D = 23
LINES = {L444: (4, 4), L435: (3, 5), L426: (2, 6), L2ROW: (4, 4), BENCH: (4, 4)}     # shape -> (ay, az)


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(z, y, x): dict(use12, ax, ay, az, lines, groups)} from the stand-alone plan program, built under sanitizers"""
    exe = str(tmp_path_factory.mktemp("pyr12") / "pyr12_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "pyr12_plan_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    shapes = OLD_PATH + list(LINES)
    args = [str(s[k]) for s in shapes for k in (2, 1, 0)]
    r = subprocess.run([exe] + args, capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0].startswith("rule: ok")
    out = {}
    for s, ln in zip(shapes, lines[1:]):
        f = [int(v) for v in ln.split()]
        assert tuple(f[:3]) == (s[2], s[1], s[0])
        out[s] = dict(zip(("use12", "ax", "ay", "az", "lines", "groups"), f[3:]))
    return out


def test_shapes_take_the_paths_meant(plans):
    """No device: the plan of every shape of this file."""
    for s in OLD_PATH:
        assert plans[s]["use12"] == 1 and plans[s]["lines"] == 0, (s, plans[s])
    assert [plans[s]["ax"] for s in OLD_PATH] == [6, 6, 5, 5, 4, 4]      # wide boxes, or a brick narrower than a line
    for s, (ay, az) in LINES.items():
        p = plans[s]
        assert p["lines"] == 1 and (p["ax"], p["ay"], p["az"]) == (4, ay, az), (s, p)
        assert p["groups"] == s[0] * s[1] * s[2] // 32768, (s, p)
    assert plans[L444]["groups"] == 16 and plans[L2ROW]["groups"] == 128 and plans[BENCH]["groups"] == 256


# ---------------------------------------------------------------- volumes ----
def _groups(shape):
    """origins (z, y, x) of the groups of a line-kernel shape, and a box's extents (ez, ey)"""
    ay, az = LINES[shape]
    ey, ez = 1 << ay, 1 << az
    return [(z, y, x) for z in range(0, shape[0], ez) for y in range(0, shape[1], ey) for x in range(0, shape[2], 128)], (ez, ey)


def _grouped(shape, seed, counts=(0, 1, 7, 8), values=MIX_VALUES):
    """Group i holds counts[i % len] constant boxes, at places that rotate with i; neighbouring constant boxes get
    different values.  The busy boxes alternate between plain noise and noise with structure at every scale."""
    rng = np.random.default_rng(seed)
    vol = np.empty(shape, np.uint8)
    origins, (ez, ey) = _groups(shape)
    for i, (z, y, x) in enumerate(origins):
        n = counts[i % len(counts)]
        const = {(i + k) % 8 for k in range(n)}
        for c in range(8):
            if c in const:
                box = values[(i + c) % len(values)]
            elif (i + c) % 2:
                box = rng.integers(0, 256, (ez, ey, 16), dtype=np.uint8)
            else:
                box = _noise_box(rng).astype(np.uint8).reshape(ez, ey, 16)
            vol[z:z + ez, y:y + ey, x + 16 * c:x + 16 * c + 16] = box
    return vol


def _rm_like(shape, n, seed=12345):
    import bench
    return list(bench.make_bricks("rm_like", n, shape[::-1], seed))


def _content_set(shape):
    """<= 4 bricks: grouped boxes, noise, a constant brick, the bench's kind of brick"""
    return [_grouped(shape, 1), np.random.default_rng(2).integers(0, 256, shape, dtype=np.uint8), np.full(shape, 131, np.uint8),
            _rm_like(shape, 1)[0]]


_CACHE = {}


def _case(O, key, make, tol, ep, midrange=False):
    """(volumes, oracle builds) made once per module"""
    k = (key, tol, ep, midrange)
    if k not in _CACHE:
        vols = [np.ascontiguousarray(v) for v in make()]
        _CACHE[k] = (vols, _refs(O, vols, tol, ep, midrange))
    return _CACHE[k]


def _check(vr, O, vols, refs, tol, ep, midrange=False):
    """A fresh handle against the oracle and against a handle with pyramid_boxes on"""
    what = (vols[0].shape, tol, ep, midrange)
    new = _make(vr, len(vols), vols[0].shape, tol, ep, midrange).build(np.stack(vols))
    out = _against_oracle(new, vols, refs, midrange, what)
    old = _make(vr, len(vols), vols[0].shape, tol, ep, midrange, switches=("pyramid_boxes",)).build(np.stack(vols))
    _same(out, _outputs(old, len(vols), vols[0].shape, midrange), what)
    return out


def _box_census(O, vols, refs):
    census = dict(constant_brick=0, skipped=0, filled=0, busy=0)
    for v, r in zip(vols, refs):
        census = _add(census, _census(O, v, r))
    return census


# ---------------------------------------------------------------- the cases ----
@pytest.mark.gpu
@pytest.mark.parametrize("shape", OLD_PATH[:4], ids=["128x16x16", "256x16x16", "128x32x16", "128x16x32"])
def test_wide_box_bricks_keep_the_box_kernel(vr, oracle, plans, shape):
    """Bricks a line wide whose boxes are wider than 16 voxels: k_pyramid12 with and without the switch."""
    assert plans[shape]["lines"] == 0
    rng = np.random.default_rng(7)
    half = np.full(shape, 90, np.uint8)
    half[:, :, :shape[2] // 2] = rng.integers(0, 256, (shape[0], shape[1], shape[2] // 2), dtype=np.uint8)
    vols = [rng.integers(0, 256, shape, dtype=np.uint8), half, np.full(shape, 3, np.uint8), _rm_like(shape, 1)[0]]
    _check(vr, oracle, vols, _refs(oracle, vols, 1, 2), 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [L444, L435, L426], ids=["128x64x64", "128x32x128", "128x32x256"])
def test_group_contents(vr, oracle, plans, shape):
    """Groups of 0, 1, 7 and 8 constant boxes, noise, a constant brick and an rm_like brick; tolerance 1, 2 epochs."""
    assert plans[shape]["lines"] == 1
    vols, refs = _case(oracle, ("content", shape), lambda: _content_set(shape), 1, 2)
    _check(vr, oracle, vols, refs, 1, 2)
    census = _box_census(oracle, vols[:1], refs[:1])
    print("grouped brick %r: %r" % (shape, census))
    nb = shape[0] * shape[1] * shape[2] // 4096
    assert census["busy"] == nb // 2 and census["skipped"] + census["filled"] == nb // 2, census


@pytest.mark.gpu
def test_two_groups_per_row(vr, oracle, plans):
    """256x128x128: the group's x origin is not 0.  The two groups of a row get different numbers of constant boxes."""
    assert plans[L2ROW]["lines"] == 1 and plans[L2ROW]["groups"] == 128
    vols, refs = _case(oracle, "tworow", lambda: [_grouped(L2ROW, 3, counts=(7, 1, 8, 0, 1, 7, 0, 8))], 1, 2)
    _check(vr, oracle, vols, refs, 1, 2)


@pytest.mark.gpu
@pytest.mark.parametrize("box", [0, 3, 7])
def test_corner_bytes_of_a_constant_box(vr, oracle, plans, box):
    """A constant box of a group with one byte off by one, at the first or last byte of its first or last row: the
    box must take the full path.  On the oracle, each such volume's result differs from the all-constant one's, so a
    box taken for constant would show.  The seven boxes beside it are constant (another value): only this box of the
    group is busy."""
    shape = L444
    assert plans[shape]["lines"] == 1
    origins, (ez, ey) = _groups(shape)
    z, y, x = origins[5]
    base = np.full(shape, 140, np.uint8)
    base[:shape[0] // 2] = np.random.default_rng(9).integers(0, 256, (shape[0] // 2,) + shape[1:], dtype=np.uint8)   # (a busy brick)
    base[z:z + ez, y:y + ey, x:x + 128] = 101
    base[z:z + ez, y:y + ey, x + 16 * box:x + 16 * box + 16] = 100
    const_ref = _refs(oracle, [base], 1, 2)[0]
    vols = []
    for k, (dz, dy, dx) in enumerate(((0, 0, 0), (0, 0, 15), (ez - 1, ey - 1, 0), (ez - 1, ey - 1, 15))):
        vol = base.copy()
        vol[z + dz, y + dy, x + 16 * box + dx] = 100 + (1 if k % 2 else -1)
        vols.append(vol)
    refs = _refs(oracle, vols, 1, 2)
    for r in refs:
        assert not (np.array_equal(r.tree, const_ref.tree) and np.array_equal(r.levelCut(), const_ref.levelCut()))
    _check(vr, oracle, vols, refs, 1, 2)
    assert _census(oracle, vols[0], refs[0])["busy"] == _census(oracle, base, const_ref)["busy"] + 1


@pytest.mark.gpu
def test_tolerance_zero(vr, oracle, plans):
    """No flags: every box takes the full path, the constant ones too."""
    vols, refs = _case(oracle, ("content", L444), lambda: _content_set(L444), 0, 2)
    _check(vr, oracle, vols, refs, 0, 2)


@pytest.mark.gpu
def test_midrange_tree(vr, oracle, plans):
    """variant = 2: the half-range heap beside the midrange heap, zeros below the constant boxes."""
    vols, refs = _case(oracle, ("content", L444), lambda: _content_set(L444), 1, 2, midrange=True)
    _check(vr, oracle, vols, refs, 1, 2, midrange=True)


@pytest.mark.gpu
def test_one_handle_alternating_kernels(vr, oracle, plans):
    """One handle, rebuilt over A and B with the switch off, on, on, off, off: boxes change between constant and busy
    from build to build and the levels D-1 and D that a constant box leaves unwritten hold the other build's bytes.
    Every rebuild equals the oracle and a fresh handle."""
    shape = L444
    A, RA = _case(oracle, ("content", shape), lambda: _content_set(shape), 1, 2)
    B, RB = _case(oracle, ("content-b", shape),
                  lambda: [np.full(shape, 8, np.uint8), _grouped(shape, 4, counts=(8, 7, 1, 0)), _grouped(shape, 5, counts=(1, 8, 0, 7), values=[128, 129]),
                           np.random.default_rng(6).integers(0, 256, shape, dtype=np.uint8)], 1, 2)
    bs = _make(vr, len(A), shape, 1, 2)
    for name, boxes in (("A", 0), ("B", 1), ("A", 1), ("B", 0), ("A", 0)):
        V, R = (A, RA) if name == "A" else (B, RB)
        bs.set_switch("pyramid_boxes", boxes)
        bs.build(np.stack(V))
        what = "rebuild %s, pyramid_boxes %d" % (name, boxes)
        out = _against_oracle(bs, V, R, False, what)
        fresh = _make(vr, len(V), shape, 1, 2).build(np.stack(V))
        _same(out, _outputs(fresh, len(V), shape, False), what + ", against a fresh handle")


@pytest.mark.gpu
def test_bench_brick_against_the_box_kernel(vr, plans):
    """One 256x256x128 brick of the bench's kind (256 groups, two per row), against the switch only: the oracle at
    this size is too slow for a unit test."""
    assert plans[BENCH]["lines"] == 1 and plans[BENCH]["groups"] == 256
    vols = _rm_like(BENCH, 1)
    new = _make(vr, 1, BENCH, 1, 2).build(np.stack(vols))
    old = _make(vr, 1, BENCH, 1, 2, switches=("pyramid_boxes",)).build(np.stack(vols))
    _same(_outputs(new, 1, BENCH, False), _outputs(old, 1, BENCH, False), "bench brick")
    assert int(vols[0].min()) != int(vols[0].max())
