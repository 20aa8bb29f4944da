"""The case table of tests/marchcases.py through the float64 references alone, no GPU: every case and marcher keeps the
masked-fraction caps that test_gpu_marcher_edges.py enforces, every case meant to show something has an unmasked pixel
whose ray took samples, and the exact-count comparison of that module reports a reference that is off by one sample."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marchcases as MC  # noqa: E402
import refproject as RP  # noqa: E402
from refmarch import rays  # noqa: E402


def test_the_case_table_is_the_edges_modules():
    cs = MC.cases()
    assert [len(MC.family(f)) for f in ("size", "dims", "side", "cam", "ns", "slab")] == [5, 11, 6, 11, 10, 9]
    assert len(cs) == 52 and [c["k"] for c in cs] == list(range(52))
    assert [(c["W"], c["H"]) for c in cs[:5]] == [(1, 1), (1, 9), (9, 1), (7, 5), (65, 63)]
    assert sorted({c["ns"] for c in cs if c["family"] == "ns"}) == [0, 1, 2, 300, 2000]
    assert [c["name"] for c in cs if c["fine"]] == ["brick step 256x256x128", "ns 2000 nee 0"]
    assert [c["name"] for c in cs if not c["shows"]] == ["on face plane x=0.5, looking in", "inside the cube",
                                                         "z_near cuts the cube", "z_far before the cube", "ns 0 nee 0",
                                                         "ns 0 nee 1"]
    near = {c["name"]: (c["near"], c["far"]) for c in cs if c["family"] == "cam"}
    assert near["z_near cuts a corner"] == MC.f32((0.9, 100.0)) and near["z_far through the cube"] == MC.f32((0.1, 1.2))
    slab = cs[MC.family("slab")[4]]                   # axis 1, rank 1: 19 voxels, owned [6, 12), halo 1 and 2
    assert slab["box_min"] == MC.f32((0.0, 6 / 19, 0.0)) and slab["box_max"] == MC.f32((1.0, 12 / 19, 1.0))
    assert slab["sub"][1][1] == (0, 5, 0) and slab["sub"][1][0].shape == (25, 8, 22)
    assert slab["sub"][2][1] == (0, 4, 0) and slab["sub"][2][0].shape == (25, 10, 22)
    assert all(max(MC.count_step_dims(c)) <= 64 for c in cs)
    lut, lut2 = MC.smooth_table(1), MC.smooth_table2d(1)
    assert lut.dtype == np.float32 and lut[:, 3].max() <= 0.5 and lut2.shape == (3, 256, 4)
    assert np.abs(np.diff(lut.astype(np.float64), axis=0)).max() <= 1 / 51 + 1e-6


@pytest.mark.parametrize("k", range(52))
def test_masked_fractions_and_something_shows(k):
    c = MC.cases()[k]
    refs = MC.references(k)
    n, nslack = refs["n"]
    line = []
    for m in MC.MARCHERS:
        img, slack = refs[m]
        assert img.shape == (c["H"], c["W"], 4) and slack.shape == (c["H"], c["W"]) and np.isfinite(img).all()
        line.append("%s %d" % (m, MC.check_masked(c, m, slack)))
        took = img[..., 3] > 0
        if m in MC.COLOUR:                              # a colour pixel is (background, 0) exactly where no sample is owned
            assert not (took & (n == 0)).any()
        else:
            assert np.array_equal(took, n > 0)
        assert not c["shows"] or (took & (slack > 1)).any(), (c["name"], m)
        assert c["shows"] or not took.any(), (c["name"], m)
    cn, cslack = refs["count"]
    line.append("count %d" % MC.check_masked(c, "count", cslack))
    assert cn.max() <= 126                                # T = 2^-n stays a normal float32
    assert not c["shows"] or ((cn > 0) & (cslack > 1)).any()
    assert MC.count_mismatches(n, n, nslack) == 0
    print("BUDGET %-34s %3dx%-3d masked: %s" % (c["name"], c["W"], c["H"], ", ".join(line)))


def test_full_hd_rows_keep_the_cap_and_show_something():
    """The eight compared rows of the 1920 x 1080 frame, marched through rows=: the same rays as the whole frame's."""
    c = MC.special("hd")
    for m in ("tf", "shaded", "max"):
        img, slack = MC.reference(c, m, MC.HD_ROWS)
        assert img.shape == (8, 1920, 4) and slack.shape == (8, 1920)
        masked = MC.check_masked(c, m, slack)
        assert ((img[..., 3] > 0) & (slack > 1)).any() and ((img[..., 3] == 0) & (slack > 1)).any()     # cube and background
        print("BUDGET 1080p rows %s: masked %d of %d" % (m, masked, slack.size))
    small = dict(c, W=48, H=27)
    whole, _ = MC.reference(small, "tf")
    rows, _ = MC.reference(small, "tf", [0, 13, 26])
    assert np.array_equal(rows, whole[[0, 13, 26]])


def test_the_skip_tables_are_transparent_below_90_and_the_sparse_volume_is_mostly_empty():
    lut, lut2 = MC.skip_tables()
    assert (lut[:90, 3] == 0).all() and (lut2[:, :90, 3] == 0).all() and (lut[90:, 3] > 0).all() and (lut2[:, 90:, 3] > 0).all()
    vol = MC.sparse_volume()
    assert vol.shape == (23, 29, 37) and (vol < 89).mean() > 0.8 and (vol == 180).any()
    n, _ = MC.owned(MC.special("skip"))
    assert (n == 0).any() and (n > 0).any()               # the frame has rays past the cube


# ---- the exact-count comparison bites ---------------------------------------------------------------------------------
def _perturbed(c, extra_steps=0, late=0):
    """The owned-sample count of a marcher that is off by one: `extra_steps` more iterations than max_samples, or a march
    that starts `late` steps into the cube (its first samples are never taken)."""
    step = np.asarray(MC.step_of(MC.count_step_dims(c)))
    covered, vuv, g = rays(c["pos"], c["front"], c["up"], c["fov"], c["W"], c["H"], None, c["near"], c["far"])
    _, n = RP.project(c["vol"], covered, vuv + late * g * step, g, step, RP.MAX, c["ns"] + extra_steps, c["box_min"], c["box_max"])
    return n


def _by_name(name):
    return [c for c in MC.cases() if c["name"] == name][0]


def test_the_count_comparison_reports_one_sample_too_many_or_too_few():
    """Without a GPU: a count that is one sample off is a mismatch on an unmasked pixel.  One iteration too many shows
    where max_samples binds (1 and 2); a first sample never taken shows wherever a ray enters the box through a cube face:
    "z_far through the cube", and for every slab axis the rank that holds the entry face."""
    for name in ("ns 1 nee 0", "ns 1 nee 1", "ns 2 nee 1"):
        c = _by_name(name)
        n, slack = MC.references(c["k"])["count"]
        assert MC.count_mismatches(_perturbed(c), n, slack) == 0, name            # the comparison itself is exact
        assert MC.count_mismatches(_perturbed(c, extra_steps=1), n, slack) > 0.5 * slack.size, name
    c = _by_name("z_far through the cube")
    n, slack = MC.references(c["k"])["count"]
    assert MC.count_mismatches(_perturbed(c), n, slack) == 0
    assert MC.count_mismatches(_perturbed(c, late=1), n, slack) > 0.5 * slack.size
    assert MC.count_mismatches(np.zeros_like(n), n, slack) > 0.5 * slack.size     # th > z_far taken for t1 > z_far: no ray
    for axis in (0, 1, 2):
        bitten = []
        for r in range(3):
            c = _by_name("slab axis %d rank %d" % (axis, r))
            n, slack = MC.references(c["k"])["count"]
            assert MC.count_mismatches(_perturbed(c), n, slack) == 0
            bitten.append(MC.count_mismatches(_perturbed(c, late=1), n, slack))
            # a box test that owns the neighbour's samples too (the whole cube) is seen in every rank
            whole = dict(c, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0))
            assert MC.count_mismatches(_perturbed(whole), n, slack) > 0.3 * slack.size
        assert max(bitten) > 0, axis
