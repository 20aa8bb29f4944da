"""The case table of tests/slicecases.py without a GPU: the float32 restatement (refslice.py) held to the independent
float64 reference (slicecases.ref64) for every case, op and filter; the masked counts held to the cap; every family held
to the edge it exists for, so that a case which silently stops reaching it fails here."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
pytest.importorskip("torch")        # render.SlicePlane
import slicecases as SC  # noqa: E402

CASES = SC.cases()
WORST = {}


def _run(vol, geo, flt, op):
    return SC.ref32(vol, SC.plane_of(geo, flt), op)


def test_the_case_table():
    count = {f: len(SC.family(f)) for f in ("lattice", "turned", "sheared", "faces", "rim", "still", "overflow", "deep", "slabs",
                                            "general")}
    assert count == dict(lattice=5, turned=5, sheared=1, faces=24, rim=12, still=3, overflow=1, deep=2, slabs=22, general=16)
    assert [c["exact"] for c in CASES] == [c["family"] != "general" for c in CASES]
    assert SC.TOL == 2e-3 and SC.CAP == 0.05
    for c in CASES:
        g = c["geo"]
        assert g["width"] * g["height"] * g["layers"] <= 65 * 63 * 7, c["name"]          # the largest single call
        for k in ("origin", "du", "dv", "dw", "box_min", "box_max"):
            assert g[k] == SC.f32(g[k]), (c["name"], k)                                   # the kernel's inputs, as float32
    lat = CASES[SC.family("lattice")[2]]["geo"]
    assert (lat["origin"], lat["du"], lat["dv"], lat["dw"], lat["layers"]) == \
        ((-0.125, -0.125, 0.5), (1 / 32, 0, 0), (0, 1 / 32, 0), (0, 0, 1 / 64), 5)
    assert (lat["box_min"], lat["box_max"]) == ((0.25, 0, 0), (0.75, 1, 17 / 32))
    worlds = sorted((c["name"].split()[1], c["geo"]["layers"]) for c in CASES if c["family"] == "slabs")
    assert [w for w, l in worlds if l == 5] == ["x2", "x3", "x4", "x5", "x8", "y2", "y3", "y4", "y8", "z2", "z4"]
    thick = {len(c["slabs"]) and min(s.shape[2 - "xyz".index(c["name"].split()[1][0])] for _, s in c["slabs"])
             for c in CASES if c["family"] == "slabs"}
    assert {2, 3} <= thick                          # slabs one voxel thick hold 2 layers with the halo, at the volume's end


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"].replace(" ", "-") for c in CASES])
def test_float32_restatement_against_ref64(k):
    c = CASES[k]
    worst, most = 0.0, 0
    for flt in (SC.NEAREST, SC.LINEAR):
        for op in SC.OPS:
            part = _run(c["vol"], c["geo"], flt, op)
            err, masked = SC.compare(c, c["vol"], c["geo"], flt, op, part)
            assert masked == 0 or not c["exact"]
            SC.check_known(c, flt, op, part, _run)
            if c["exact"] and c["family"] != "deep":
                SC.check_reversed(c, flt, op, part, _run)
            if not c["slabs"]:
                SC.check_rotated(c, flt, op, part, _run)
            worst, most = max(worst, err), max(most, masked)
            if c["slabs"]:
                total = np.zeros_like(part[..., 1])
                for geo, sub in c["slabs"]:
                    sp = _run(sub, geo, flt, op)
                    SC.compare(c, sub, geo, flt, op, sp)
                    total = total + sp[..., 1]
                assert np.array_equal(total, part[..., 1]), (c["name"], flt, op)          # every sample has one owner
    WORST[c["family"]] = max(WORST.get(c["family"], 0.0), worst)
    print("SLICE-REF %-28s largest difference %.3g, most masked %d of %d" % (c["name"], worst, most, part[..., 0].size))


@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"].replace(" ", "-") for c in CASES])
def test_every_case_hits_its_edge(k):
    c = CASES[k]
    for what in c["hits"]:
        assert SC.hit(c, what), (c["name"], what)


def test_every_family_hits_what_it_is_for():
    """Per family, so that dropping a hit from a case's list does not go unnoticed either."""
    def some(fam, what):
        return any(SC.hit(CASES[k], what) for k in SC.family(fam))
    for what in SC.BOUNDARIES:
        assert some("lattice", what) and some("sheared", what), what
    for what in ("zero", "one", "voxel_boundary"):
        assert some("turned", what), what
    assert some("sheared", "every_n") and not some("lattice", "every_n")
    assert some("faces", "all_empty") and some("faces", "zero") and some("faces", "one")
    assert some("overflow", "nan") and some("slabs", "box_min") and some("slabs", "box_max")
    # the general planes: the third and the fourth stick out of the cube, and with 7 layers n takes every value
    for which in (2, 3):
        c = CASES[[k for k in SC.family("general") if CASES[k]["name"] == "plane %d 28x20x24 x7" % which][0]]
        n = SC.ref64(c["vol"], SC.plane(c, SC.LINEAR), SC.MAX).n
        assert set(range(8)) <= set(n.ravel().tolist()), which


def test_largest_differences_per_family():
    """Of the families test_float32_restatement_against_ref64 has run in this process (all of them in a whole run)."""
    for fam, worst in sorted(WORST.items()):
        print("SLICE-REF family %-8s largest difference %.3g" % (fam, worst))
        assert worst <= SC.TOL
