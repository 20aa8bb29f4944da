"""The per-brick error kernel and the error table on the bench volume:
python profiles/tools/error_bench.py [--out FILE] [--reps N]

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once, decodes it at
full depth and times, with HIP events around the calls on the two buffers (decode, original voxels; 2 x 7.5 GiB read):
  k_brick_error     vr_measure_error_bricks, 960 entries
  k_measure_error   vr_measure_error, the one max and one mean this library had before
as five alternating runs of each, a run being the median of --reps calls after two warm-up calls.  Both calls allocate
their few result bytes, clear them, launch one kernel, copy back and synchronise, so the intervals compare like with
like.  Also: the same kernel on 100 000 bricks of 64 bytes, the whole table (every cut 0 .. max_tree_depth: a uniform
decode plus the kernel per cut, one synchronisation), and, from a child process once this one's buffers are freed,
profiles/tools/bw_ref.py, whose "read (sum)" line is the streaming-read rate of the same device in the same session.
Writes the report to profiles/error_table_bench.txt (or --out)."""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import volumerenderer_amd as vr  # noqa: E402


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "error_table_bench.txt"))
    ap.add_argument("--reps", type=int, default=9)
    args = ap.parse_args()
    bd, gd = (256, 256, 128), (2048, 2048, 1920)
    vox = bench.make_volume_gpu(torch, gd, bd, seed=12345).reshape(-1)
    V = bd[0] * bd[1] * bd[2]
    B = vox.numel() // V
    bs = vr.BrickSet(B, bd, 1, 2)
    bs.build(vox)
    dec = bs.decode()
    torch.cuda.synchronize()
    M = bs.info(0)["max_tree_depth"]
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    gib = 2.0 * B * V / 2**30
    say("bench volume %s, %d bricks of %s, max_tree_depth %d; two buffers of %.2f GiB; %d reps per run (median)"
        % (gd, B, bd, M, gib / 2, args.reps))
    per = vr.measure_error_bricks(dec, vox, B)
    mx, mean = vr.measure_error(dec, vox)
    assert int(per["max_abs"].max()) == mx, "the two kernels disagree on the maximum"
    assert abs(float(sum(int(v) for v in per["sum_abs"])) / (B * V) - mean) < 1e-9, "the two kernels disagree on the mean"
    new, old = [], []
    for _ in range(5):
        new.append(timed(lambda: vr.measure_error_bricks(dec, vox, B), args.reps))
        old.append(timed(lambda: vr.measure_error(dec, vox), args.reps))
    tb = lambda ms: 2.0 * B * V / ms / 1e9      # noqa: E731
    say("k_brick_error    runs (ms) %s   slowest %.3f ms = %.2f TB/s   fastest %.3f ms = %.2f TB/s"
        % (" ".join("%.3f" % m for m in new), max(new), tb(max(new)), min(new), tb(min(new))))
    say("k_measure_error  runs (ms) %s   slowest %.3f ms = %.2f TB/s   fastest %.3f ms = %.2f TB/s"
        % (" ".join("%.3f" % m for m in old), max(old), tb(max(old)), min(old), tb(min(old))))
    say("ratio of medians (old / new) %.2f x;  slowest new %s fastest old (%.3f vs %.3f ms)"
        % (float(np.median(old)) / float(np.median(new)), "<" if max(new) < min(old) else ">=", max(new), min(old)))
    res.update(brick_error_ms=new, measure_error_ms=old)
    # many tiny bricks: the same bytes of the two buffers read as 100 000 bricks of 64
    nb, v = 100000, 64
    tiny = timed(lambda: vr.measure_error_bricks(dec[:nb * v], vox[:nb * v], nb), args.reps)
    say("k_brick_error    %d bricks of %d bytes: %.3f ms" % (nb, v, tiny))
    res["tiny_ms"] = tiny
    # the whole table
    scratch = torch.empty(B * V, dtype=torch.uint8, device="cuda")
    t_dec = timed(lambda: bs.decode(out=scratch), args.reps)
    t_tab = timed(lambda: bs.error_table(reference=vox, scratch=scratch), 3)
    t0 = time.perf_counter()
    table = bs.error_table(reference=vox, scratch=scratch)
    wall = (time.perf_counter() - t0) * 1e3
    say("full table, cuts 0 .. %d against the original voxels: %.1f ms by events, %.1f ms wall (%d x (decode + kernel); "
        "a full-depth decode alone %.3f ms)" % (M, t_tab, wall, M + 1, t_dec))
    cuts0 = vr.select_lod_error(bs.error_table(scratch=scratch), 0, V)
    hist = {int(k): int(c) for k, c in zip(*np.unique(cuts0, return_counts=True))}
    say("cuts that lose nothing against the full decode (bound 0): %s" % hist)
    psnr = [10.0 * np.log10(255.0 * 255.0 * B * V / max(1, sum(int(s) for s in table[c]["sum_sq"]))) for c in range(M + 1)]
    say("PSNR against the original by cut: %s" % " ".join("%.1f" % p for p in psnr))
    res.update(table_ms=t_tab, table_wall_ms=wall, decode_ms=t_dec, lossless_cuts=hist)
    del vox, dec, scratch, bs
    torch.cuda.empty_cache()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "profiles", "tools", "bw_ref.py")], capture_output=True, text=True)
    for ln in r.stdout.strip().splitlines():
        say("bw_ref.py: " + ln)
    if r.returncode != 0:
        say("bw_ref.py failed: " + r.stderr.strip()[-300:])
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
