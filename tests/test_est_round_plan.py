"""The start-distance estimator's round plan, without a device.

tests/est_plan_main.cpp, a stand-alone program linked against volumerenderer_amd/csrc/host_plan.cpp and built under the
address and undefined-behaviour sanitizers, checks est_round_plan for every level of 2^13 .. 2^31 nodes and both
schedules (its header lists what) and prints the plans of the levels the GPU cases run at; tests/est_rounds_cases.py's
restatement of the limits is pinned to that output.

The GPU cases (tests/test_gpu_est_rounds.py) claim where their volumes change the threshold.  That is asserted here, on
the oracle's side: every level above the leaves of such a volume is 128 and reproduced exactly (the oracle's heaps), and
the leaf level's trajectory, restated from the running-mean rule, has its changes where the case says."""
import os
import subprocess

import numpy as np
import pytest

import est_rounds_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")
LEVELS = [13, 15, 18, 19, 23, 31]


@pytest.fixture(scope="module")
def plans(tmp_path_factory):
    """{(level, schedule): (nseg, [(segEnd, nc, kernel)])} from the stand-alone program"""
    exe = str(tmp_path_factory.mktemp("estplan") / "est_plan_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "est_plan_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    r = subprocess.run([exe] + [str(v) for v in LEVELS], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[0] == "rule: ok"
    out = {}
    for ln in lines[1:]:
        f = ln.split()
        out[(int(f[0]), f[1])] = (int(f[2]), [(int(a), int(b), c) for a, b, c in (x.split(":") for x in f[3:])])
    return out


def test_plan_rule_and_levels(plans):
    for level in LEVELS:
        nseg, old = plans[(level, "old")]
        assert nseg == (1 << level) // 1024
        assert old == [(nseg, 4, "q"), (nseg, 4, "x")] + [(nseg, 8, "x")] * 3
        nseg, new = plans[(level, "new")]
        lim, n2 = EC.limits(level)
        assert n2 == nseg
        assert [r[0] for r in new if r[0] < nseg] == lim, (level, new)
        assert [r[2] for r in new][-3:] == ["x"] * 3 and all(r[2] == "q" for r in new[:-3])
    # D = 13: four segments behind the head, every prefix limit collapses; level 19: limits inside a walk step of 256
    assert EC.limits(13) == ([], 8) and EC.limits(19) == ([35, 131], 512) and EC.limits(18) == ([19, 67], 256)
    assert EC.limits(31)[0] == [4 + ((1 << 21) - 4) // 16, 4 + ((1 << 21) - 4) // 4]


def _pinned(oracle, shape, a):
    """The leaf level's thresholds of the volume of amplitudes `a` -- after checking on the oracle's heaps that the
    construction is what est_rounds_cases says (parents 128, reproduced exactly, leaves 128 -+ a) and that the restated
    running-mean rule ends the leaf level with the sum and count the oracle's own estimate ends with (its trace)."""
    order = EC.leaf_order(oracle, shape)
    vol = EC.paired_volume(shape, order, a)
    t = oracle.OracleTree(vol.copy(), tolerance=1, max_epochs=2).build()
    D = t.origTreeDepth
    leaves = np.array(t.temp, np.int64)
    assert np.array_equal(np.abs(leaves - 128), np.repeat(a, 2))
    rec = np.array(t.recon_all, np.int64)
    assert rec.size == (2 << D) - 1 and np.all(rec[:(1 << D) - 1] == 128)      # every node above the leaves
    S, C = EC.leaf_state(a)
    est = [r for r in t.trace() if r["kind"] == 0 and r["depth"] == D]           # the start estimate: error = sum, df = count
    assert len(est) == 1 and (est[0]["error"], est[0]["df"]) == (float(S[-1]), float(C[-1])), (est, S[-1], C[-1])
    assert est[0]["distance"] == (round(float(S[-1]) / float(C[-1])) if C[-1] else 0.0)
    return EC.leaf_thresholds(a)


@pytest.mark.parametrize("shape", [(64, 64, 64), (128, 64, 64)])
def test_constructed_trajectories(oracle, shape):
    n = shape[0] * shape[1] * shape[2]
    level = int(np.log2(n))
    (l0, l1), nseg = EC.limits(level)
    T = _pinned(oracle, shape, EC.constant(n // 2))
    assert EC.changes(T) == [] and T[4] == 4
    # one change: inside the first prefix round; in the last segment of a round, the first of the next, and one further
    for seg in (10, l0 - 1, l0, l0 + 1, l1 - 1, l1, l1 + 1, nseg - 2):
        T = _pinned(oracle, shape, EC.one_change(n // 2, seg))
        assert EC.changes(T) == [(seg, 4, 5)], seg
    for first, then, sign in ((9, 40, 1), (40, 22, -1)):
        T = _pinned(oracle, shape, EC.drift(n // 2, first, then))
        ch = EC.changes(T)
        assert len(ch) >= 6 and all((new - old) * sign > 0 for _, old, new in ch), ch      # monotone, more changes than rounds
        assert abs(int(T[-1]) - int(T[4])) >= 6
        assert any(s >= l1 for s, _, _ in ch)                                             # some of them in the bulk
    # the boundary case: the threshold is 3 or 4 at every segment start (it alternates inside the segments)
    T = _pinned(oracle, shape, EC.boundary(n // 2))
    assert set(int(v) for v in T[4:]) <= {3, 4}
    # the false-alarm case: the threshold is 4 at every NODE behind the head (no exact record can fail), the mean never
    # more than 4 units above the boundary (S - 8 C in [4, 8]: inside the quad bound's slack of 9 at Th = 4)
    a = EC.near_boundary(n // 2)
    T = _pinned(oracle, shape, a)
    S, C = EC.leaf_state(a)
    d = (S - 8 * C)[4096:]
    assert d.min() >= 4 and d.max() <= 8 and np.all(S[4096:] // (2 * C[4096:] + 1) == 4) and np.all(np.diff(C) == 1)
