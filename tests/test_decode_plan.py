"""The plan of a decode call, without a device.

tests/decode_plan_main.cpp, a stand-alone program linked against volumerenderer_amd/csrc/host_plan.cpp and built under the
address and undefined-behaviour sanitizers, restates the rules of the uniform, range, per-brick and pool decodes in its
own words and compares every field of make_decode_plan / make_lod_plan over the class boundaries of D, the cut, the
geometry, the side-cars, the stream and the switches (its header lists them), then checks pool_layout.  Nothing is
loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("decodeplan") / "decode_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "decode_plan_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().split("\n")


def _count(line, what):
    m = re.fullmatch(what + r": (\d+) ok", line)
    assert m, line
    return int(m.group(1))


def test_uniform_plans_at_every_class_boundary(report):
    assert _count(report[0], "decode plans") > 1000000


def test_lod_plans_classes_offsets_and_descriptors(report):
    assert _count(report[1], "lod plans") > 2000


def test_pool_layout_slots_cells_and_totals(report):
    assert _count(report[2], "pool layouts") == 28


def test_decode_decisions_live_in_the_plan_only():
    """the decode driver of kd_decode.hip executes: no switch, geometry class, side-car or stream-origin condition is
    left in it, and it neither allocates nor creates events"""
    src = open(os.path.join(CSRC, "kd_decode.hip")).read()
    drv = src[src.index("// ---- decode driver: executes a DecodePlan / LodPlan"):]
    for word in ("hipMalloc", "hipHostMalloc", "hipEventCreate", "->sw.", "->generalGeom", "->foreign", "->fineAll"):
        assert word not in drv, word
    # and the kernel is chosen in one place
    assert "decode_stores_vectors" not in src and "DecodeKernel::" not in open(os.path.join(CSRC, "capi.hip")).read()
