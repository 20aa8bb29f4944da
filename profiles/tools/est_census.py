#!/usr/bin/env python3
"""est_census.py -- replay the start-distance estimator's threshold trajectories against round plans.

Input: the event log of a VR_EST_CENSUS build of the library (kd_encode.hip: k_est_walk logs, per brick, level and
round, where the walk starts, every segment it walks node by node with the threshold behind it, and where and why the
round ends), read with vr_debug_est_census after one build of the bench volume under est_exact_bounds and
est_old_schedule (profiles/tools/est_census_capture.py: the build line and the capture), as an (N, 4) uint32 .npy: brick | level << 16 | round << 24, segment, threshold, kind | up << 8.
With exact records a segment is walked exactly where its hypothesis fails, and the threshold floor(S / (2C + 1)) is
constant between two walked segments, so the log IS the trajectory, whatever plan it was taken under.

  python profiles/tools/est_census.py profiles/r12_est_census.txt            # the table of plans
  python profiles/tools/est_census.py profiles/r12_est_census.txt --where    # and where in a level the threshold changes
  python profiles/tools/est_census.py LOG.npy --write-text OUT.txt           # a raw log as trajectories, one walk per line

profiles/r12_est_census.txt is the bench volume's log in that text form: brick, level, the threshold and half behind the
head, then segment:threshold:half of every walked segment.

A plan is a list of rounds (limit as a fraction of the level's segments behind the head, window width, kernel).  Per
brick and level the replay charges a round (limit - start) segments, under its width, and ends it where the threshold
leaves the window (window_base below = est_window_base of host_plan.h).  Cost model, static VALU instructions per wave
and sweep of two segments: 182 + 118 nc for the quad kernel; 170 + 200 nc for the exact kernel (16 node pairs of 9
instructions and the same epilogue per candidate: an estimate from the source, not a count).  Not modelled: lane-uniform
and skipped sweeps (cheap under every plan), the quad rounds' false failures and budget (654 of 11 965 walked segments
on the bench volume), and the orientation bit at a round that starts at a limit, where the log has no state: the last
logged one is used.
"""
import sys

import numpy as np

EC_WALKED, EC_START = 1, 7
HEAD_SEGS = 4


def window_base(T, up, nc):
    b = T - (2 if nc >= 8 else (1 if nc >= 3 else (1 if nc == 2 and not up else 0)))
    return max(0, min(b, 256 - nc))


def trajectories(log):
    """{(brick, level): (T0, up0, [(seg, T, up), ...])}"""
    out = {}
    key = log[:, 0] & 0xFFFFFF
    kind, up = log[:, 3] & 0xFF, (log[:, 3] >> 8) & 1
    rnd = log[:, 0] >> 24
    for i in np.flatnonzero(((kind == EC_START) & (rnd == 0)) | (kind == EC_WALKED)):
        k = (int(key[i] & 0xFFFF), int(key[i] >> 16))
        if kind[i] == EC_START:
            out[k] = (int(log[i, 2]), int(up[i]), [])
        else:
            out[k][2].append((int(log[i, 1]), int(log[i, 2]), int(up[i])))
    for v in out.values():
        v[2].sort()
    return out


def write_text(traj, path):
    """One line per walk: brick level T0 up0, then seg:T:up per walked segment (the committed form of a log)."""
    with open(path, "w") as f:
        f.write("# brick level T0 up0 [segment:threshold:up of every segment walked node by node]\n")
        for (brick, level), (T, up, ev) in sorted(traj.items()):
            f.write(" ".join(["%d %d %d %d" % (brick, level, T, up)] + ["%d:%d:%d" % e for e in ev]) + "\n")


def read_text(path):
    out = {}
    for ln in open(path):
        if ln.startswith("#"):
            continue
        f = ln.split()
        out[(int(f[0]), int(f[1]))] = (int(f[2]), int(f[3]), [tuple(int(v) for v in e.split(":")) for e in f[4:]])
    return out


def plan_rounds(plan, nseg):
    """[(segEnd, nc, quads)]: prefix rounds shorter than 8 segments dropped, as est_round_plan does"""
    rounds, at = [], HEAD_SEGS
    for frac, nc, quads in plan:
        if frac >= 1.0:
            rounds.append((nseg, nc, quads))
            at = nseg
        else:
            pre = int((nseg - HEAD_SEGS) * frac)
            if pre >= 8 and HEAD_SEGS + pre > at:
                at = HEAD_SEGS + pre
                rounds.append((at, nc, quads))
    return rounds


def replay(traj, plan):
    cand_seg = valu = 0.0
    last_resort = ends = 0
    per_round = [0] * 8
    for (brick, level), (T, up, ev) in traj.items():
        nseg = (1 << level) // 1024
        rounds = plan_rounds(plan, nseg)
        seg, i = HEAD_SEGS, 0
        for r, (end, nc, quads) in enumerate(rounds):
            if seg >= nseg:
                break
            if seg >= end:
                continue
            base = window_base(T, up, nc)
            if not base <= T < base + nc:
                raise AssertionError("a window misses its own threshold")
            cand_seg += (end - seg) * nc
            valu += (end - seg) / 2.0 * ((182 + 118 * nc) if quads else (170 + 200 * nc))
            per_round[r] += 1
            left = False
            while i < len(ev) and ev[i][0] < end:
                s, T, up = ev[i]
                i += 1
                if not base <= T < base + nc:
                    seg, left = s + 1, True
                    break
            if not left:
                seg = end
            elif r == len(rounds) - 1:
                last_resort += nseg - seg
                seg = nseg
            else:
                ends += 1
    return cand_seg, valu, ends, last_resort, per_round


Q, X = True, False
TAIL = [(1.0, 8, X)] * 3
PLANS = [
    ("old: 4Q, 4X, 8X 8X 8X, whole level", [(1.0, 4, Q), (1.0, 4, X)] + TAIL),
    ("2Q, 4Q", [(1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1Q, 4Q", [(1.0, 1, Q), (1.0, 4, Q)] + TAIL),
    ("1Q, 2Q, 4Q", [(1.0, 1, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 2Q, 4Q", [(1 / 16, 4, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/8 4Q, 1Q, 2Q, 4Q", [(1 / 8, 4, Q), (1.0, 1, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 4Q, 2Q, 4Q", [(1 / 16, 4, Q), (1 / 4, 4, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 2Q, 2Q, 4Q", [(1 / 16, 4, Q), (1 / 4, 2, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 2Q, 1/4 2Q, 2Q, 4Q", [(1 / 16, 2, Q), (1 / 4, 2, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 4Q, 1Q, 4Q", [(1 / 16, 4, Q), (1 / 4, 4, Q), (1.0, 1, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 2Q, 1Q, 4Q  (chosen)", [(1 / 16, 4, Q), (1 / 4, 2, Q), (1.0, 1, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 2Q, 1Q, 2Q, 4Q", [(1 / 16, 4, Q), (1 / 4, 2, Q), (1.0, 1, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 2Q, 1/2 2Q, 2Q, 4Q", [(1 / 16, 4, Q), (1 / 4, 2, Q), (1 / 2, 2, Q), (1.0, 2, Q), (1.0, 4, Q)] + TAIL),
    ("1/16 4Q, 1/4 2Q, 1/2 1Q, 1Q, 4Q", [(1 / 16, 4, Q), (1 / 4, 2, Q), (1 / 2, 1, Q), (1.0, 1, Q), (1.0, 4, Q)] + TAIL),
]


def main():
    traj = trajectories(np.load(sys.argv[1])) if sys.argv[1].endswith(".npy") else read_text(sys.argv[1])
    if "--write-text" in sys.argv:
        write_text(traj, sys.argv[sys.argv.index("--write-text") + 1])
    busy = sum(1 for v in traj.values() if v[2])
    print("%d (brick, level) walks, %d with a walked segment, %d walked segments" %
          (len(traj), busy, sum(len(v[2]) for v in traj.values())))
    base = None
    print("%-36s %14s %7s %12s %7s %8s %11s  %s" % ("plan", "cand-segments", "vs old", "VALU/1e6", "vs old", "re-runs",
                                                   "last-resort", "walks per round"))
    for name, plan in PLANS:
        cs, valu, ends, lr, per = replay(traj, plan)
        base = base or (cs, valu)
        print("%-36s %14d %6.1f%% %12.1f %6.1f%% %8d %11d  %s" % (name, cs, 100 * cs / base[0], valu / 1e6, 100 * valu / base[1],
                                                                ends, lr, per[:len(plan)]))
    if "--where" in sys.argv:
        # where the threshold changes: position of a change as a fraction of the level's segments behind the head
        pos, nchg = [], []
        for (brick, level), (T, up, ev) in traj.items():
            nseg, n = (1 << level) // 1024, 0
            for s, T2, _ in ev:
                if T2 != T:
                    pos.append((s - HEAD_SEGS) / float(nseg - HEAD_SEGS))
                    T, n = T2, n + 1
            nchg.append(n)
        pos, nchg = np.array(pos), np.array(nchg)
        print("threshold changes: %d in all; walks with 0 / 1 / 2 / 3+ changes: %d / %d / %d / %d" %
              (pos.size, (nchg == 0).sum(), (nchg == 1).sum(), (nchg == 2).sum(), (nchg >= 3).sum()))
        for a, b in ((0, 1 / 64), (1 / 64, 1 / 16), (1 / 16, 1 / 4), (1 / 4, 1 / 2), (1 / 2, 1.0001)):
            print("  changes in [%.3f, %.3f) of a level: %d" % (a, b, ((pos >= a) & (pos < b)).sum()))


if __name__ == "__main__":
    main()
