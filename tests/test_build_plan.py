"""The plan of a build and the one table of debugging switches, without a device.

tests/build_plan_main.cpp, a stand-alone program linked against volumerenderer_amd/csrc/host_plan.cpp and built under the
address and undefined-behaviour sanitizers, restates the rules of vr_brickset_build in its own words and compares every
field of make_build_plan / build_level over the class boundaries of D, B, variant, epochs, tolerance, streams and
switches (its header lists them), then checks the switch table's lookup.  Nothing is loaded into Python.

The names include/vrhip.h documents for vr_brickset_set_switch and for the environment are compared with the table's
rows here: a switch that is documented and not in the table, or the other way round, fails."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")


@pytest.fixture(scope="module")
def report(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("buildplan") / "build_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "build_plan_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    return r.stdout.strip().split("\n")


def test_plan_rules_at_every_class_boundary(report):
    m = re.fullmatch(r"plans: (\d+) ok", report[0])
    assert m and int(m.group(1)) > 1000000, report[0]


def _documented():
    """(names, environment variables) of the "debugging switches" comment of vrhip.h"""
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    doc = hdr[hdr.index("---- debugging switches"):hdr.index("vr_status vr_brickset_set_switch(")]
    env = doc[doc.index("initialised from the environment ("):]
    env = set(re.findall(r"VRHIP_[A-Z0-9_]+", env[:env.index(")")]))
    names = doc[doc.index("Names:"):doc.index("any other name is VR_ERR_INVALID")]
    names = set(re.findall(r'"([a-z0-9_]+)"', names))
    return names, env


def test_switch_table_matches_the_header(report):
    rows = [ln.split()[1:] for ln in report if ln.startswith("switch ")]
    assert report[-1] == "switches: %d ok" % len(rows)
    table = {name: env for name, env in rows}
    assert len(table) == len(rows) >= 10
    names, env = _documented()
    assert names == set(table), (names ^ set(table))
    # every variable the header lists is a row's; a row's variable may go unlisted there, never the other way round
    assert env <= set(table.values()), env - set(table.values())
    assert all(table[n] == "VRHIP_" + n.upper() for n in table)


def test_build_decisions_live_in_the_plan_only():
    """the host driver of kd_encode.hip executes: no geometry, variant, tolerance, epoch or switch condition is left
    in it, and it neither allocates nor creates streams or events"""
    src = open(os.path.join(CSRC, "kd_encode.hip")).read()
    drv = src[src.index("// ------------------------------------------------------------ host driver ----"):]
    for word in ("hipMalloc", "hipStreamCreate", "hipEventCreate", "->sw.", "->variant", "->tolerance <", "->tolerance >",
                 "->maxEpochs", "->levelLoopStreams", "->compactOnBuild", "D >= 1", "D > 1", "->leafless"):
        assert word not in drv, word
