"""The plan of an install, without a device.

tests/install_plan_main.cpp, a stand-alone program linked against volumerenderer_amd/csrc/host_plan.cpp and built under
the address and undefined-behaviour sanitizers, restates the rules of vr_brickset_set_tree / vr_brickset_set_trees in its
own words -- the precedence of their refusals as it was before there was a plan is written down in its header -- and
compares every field of make_install_plan and check_stream over the depths, engines, states and violations its header
lists.  Nothing is loaded into Python."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")
UNITS = ("capi.hip", "kd_index.hip", "host_plan.h", "host_plan.cpp", "brickset.h")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("installplan") / "install_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "install_plan_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().split("\n")


def _count(line, what):
    m = re.fullmatch(what + r": (\d+) ok", line)
    assert m, line
    return int(m.group(1))


def test_install_plans_over_engines_states_and_violations(report):
    assert _count(report[0], "install plans") > 900000


def test_stream_checks_one_and_two_violations(report):
    assert _count(report[1], "stream checks") == 7 * 2 * 2 * 12 * 12


def _body(src, name):
    """the text of the function definition `name(` from its opening brace to the closing brace in column 0"""
    start = src.index("\nvr_status " + name + "(")
    return src[src.index("\n{", start):src.index("\n}", start)]


def test_install_decisions_and_allocations_live_in_one_place_each():
    """the two entry points neither allocate nor restate a rule: the buffers come from ensure_install_buffers, the
    refusals and sizes from the plan, the grown-branch rule from std_chain_distances, written once"""
    capi = open(os.path.join(CSRC, "capi.hip")).read()
    for name in ("vr_brickset_set_tree", "vr_brickset_set_trees"):
        body = _body(capi, name)
        assert "make_install_plan" in body and "begin_install" in body, name
        for word in ("hipMalloc", "ensure_dev", "treeCap -", "+ 3) / 4", "VR_ERR_STATE", "VR_ERR_UNSUPPORTED"):
            assert word not in body, (name, word)
    units = {u: open(os.path.join(CSRC, u)).read() for u in UNITS}
    assert sum(s.count("64 >> ") for s in units.values()) == 1
    assert units["host_plan.h"].count("64 >> ") == 1 and "std_chain_distances" in units["kd_index.hip"]
    # the member that nothing read is gone
    for dirpath, _, files in os.walk(os.path.join(ROOT, "volumerenderer_amd")):
        for f in files:
            if f.endswith((".hip", ".h", ".cpp", ".py")):
                assert "openTreeBytes" not in open(os.path.join(dirpath, f), errors="replace").read(), os.path.join(dirpath, f)
