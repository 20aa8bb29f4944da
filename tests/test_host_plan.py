"""The GPU-free host unit (volumerenderer_amd/csrc/host_plan.*): split rule, launch plans, the walker of foreign streams
and the file header, checked by tests/host_plan_main.cpp -- a stand-alone program built with plain g++ under the
address and undefined-behaviour sanitizers and run as a child process.  No device, nothing loaded into Python."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")
GOLD = os.path.join(ROOT, "tests", "golden")


def test_host_plan_unit_under_sanitizers(tmp_path):
    src = open(os.path.join(CSRC, "host_plan.h")).read() + open(os.path.join(CSRC, "host_plan.cpp")).read()
    assert "hip/" not in src and "hip_runtime" not in src           # the unit includes no HIP header
    exe = str(tmp_path / "host_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "host_plan_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    r = subprocess.run([exe, os.path.join(GOLD, "ref_sphere_n3_16_tol1_ep2.tree.bin"), os.path.join(GOLD, "decode_plans.json")],
                       capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "geometry and plans: 1331 extent triples ok" in r.stdout
