"""The histogram kernels on the bench volume:
python profiles/tools/hist_bench.py [--out FILE] [--reps N]

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once, decodes it at
full depth and times, with HIP events around the calls (a run = the median of --reps calls after two warm-up calls):
  k_hist_bricks     vr_histogram_bricks of the decode, 960 x 256 counts and the total      (7.5 GiB read)
  k_brick_error     vr_measure_error_bricks of the decode against the original voxels     (2 x 7.5 GiB read): the
                    project's yardstick for a streaming read; its rate in this run sets the histogram's floor
  torch.bincount    of the same bytes in chunks of 256 MiB: what a user does without the library
as five alternating runs of each, then the histogram again without its data-aware paths (vr_debug_set "hist_plain").
Both library calls allocate their result tables, clear them, launch one kernel, copy back and synchronise, so the
intervals compare like with like.  Then, on buffers of the same size: a constant volume and a uniform-random one, with
and without the data-aware paths; a ladder of 1 GiB buffers that all cost the same bytes but 0, 1, 4 and 16 LDS adds per
16-byte vector and lane (what the kernel's time follows when the bytes are held fixed); and vr_histogram2d of the decode
assembled densely, against one read of the volume at the yardstick's rate.
Writes the report to profiles/hist_bench.txt (or --out)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import volumerenderer_amd as vr  # noqa: E402
from volumerenderer_amd import _lib  # noqa: E402


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


def plain(on):
    assert _lib.lib().vr_debug_set(b"hist_plain", int(on)) == 0


def bincount_chunked(buf, chunk=1 << 28):
    total = torch.zeros(256, dtype=torch.int64, device=buf.device)
    for lo in range(0, buf.numel(), chunk):
        total += torch.bincount(buf[lo:lo + chunk].to(torch.int64), minlength=256)
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hist_bench.txt"))
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
    del bs
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    nbytes = B * V
    say("bench volume %s, %d bricks of %s, decoded: %.2f GiB; %d reps per run (median)" % (gd, B, bd, nbytes / 2**30, args.reps))
    bricks, total = vr.histogram_bricks(dec, B)
    want = bincount_chunked(dec).cpu().numpy().astype(np.uint64)
    assert np.array_equal(total, want) and np.array_equal(bricks.astype(np.uint64).sum(0), want), "the histogram disagrees with torch.bincount"
    blocks = dec.reshape(-1, 4096)
    const_blocks = float((blocks == blocks[:, :1]).all(1).float().mean())
    say("histogram equals torch.bincount; bin 0 holds %.1f %% of the voxels, %d bins are populated, %.1f %% of the 4096-byte runs are constant"
        % (100.0 * float(total[0]) / nbytes, int((total != 0).sum()), 100.0 * const_blocks))
    new, err, tbc = [], [], []
    for _ in range(5):
        new.append(timed(lambda: vr.histogram_bricks(dec, B), args.reps))
        err.append(timed(lambda: vr.measure_error_bricks(dec, vox, B), args.reps))
        tbc.append(timed(lambda: bincount_chunked(dec), 3))
    tb = lambda n, ms: n / ms / 1e9      # noqa: E731
    say("k_hist_bricks    runs (ms) %s   slowest %.3f ms = %.2f TB/s   fastest %.3f ms = %.2f TB/s"
        % (" ".join("%.3f" % m for m in new), max(new), tb(nbytes, max(new)), min(new), tb(nbytes, min(new))))
    say("k_brick_error    runs (ms) %s   slowest %.3f ms = %.2f TB/s   fastest %.3f ms = %.2f TB/s  (twice the bytes)"
        % (" ".join("%.3f" % m for m in err), max(err), tb(2 * nbytes, max(err)), min(err), tb(2 * nbytes, min(err))))
    say("torch.bincount   runs (ms) %s   (256 MiB chunks through int64)" % " ".join("%.1f" % m for m in tbc))
    rate = tb(2 * nbytes, float(np.median(err)))
    floor = nbytes / rate / 1e9
    say("streaming floor: %.2f GiB at k_brick_error's %.2f TB/s = %.3f ms; k_hist_bricks' median %.3f ms is %.2f x the floor"
        % (nbytes / 2**30, rate, floor, float(np.median(new)), float(np.median(new)) / floor))
    say("ratio of medians: k_brick_error / k_hist_bricks %.2f x; torch.bincount / k_hist_bricks %.0f x; slowest new %s fastest "
        "torch.bincount (%.3f vs %.1f ms)" % (float(np.median(err)) / float(np.median(new)), float(np.median(tbc)) / float(np.median(new)),
                                              "<" if max(new) < min(tbc) else ">=", max(new), min(tbc)))
    res.update(hist_ms=new, brick_error_ms=err, bincount_ms=tbc, floor_ms=floor)
    plain(1)
    try:
        slow = [timed(lambda: vr.histogram_bricks(dec, B), args.reps) for _ in range(3)]
    finally:
        plain(0)
    say("k_hist_bricks without the data-aware paths: runs (ms) %s = %.2f x the kernel as built" %
        (" ".join("%.3f" % m for m in slow), float(np.median(slow)) / float(np.median(new))))
    res["hist_plain_ms"] = slow
    del vox
    # the two ends of the data: one value everywhere, and no two bytes alike
    for name, buf in (("constant", torch.full((nbytes,), 37, dtype=torch.uint8, device="cuda")),
                      ("uniform random", torch.randint(0, 256, (nbytes,), dtype=torch.uint8, device="cuda"))):
        fast = [timed(lambda: vr.histogram_bricks(buf, B), args.reps) for _ in range(3)]
        plain(1)
        try:
            slow = [timed(lambda: vr.histogram_bricks(buf, B), 3) for _ in range(3)]
        finally:
            plain(0)
        say("%-15s volume: runs (ms) %s = %.2f TB/s, %.2f x the floor; without the data-aware paths %s"
            % (name, " ".join("%.3f" % m for m in fast), tb(nbytes, float(np.median(fast))), float(np.median(fast)) / floor,
               " ".join("%.3f" % m for m in slow)))
        res[name.replace(" ", "_") + "_ms"] = fast
        res[name.replace(" ", "_") + "_plain_ms"] = slow
        del buf
    # a ladder of LDS adds at fixed bytes: 1 GiB each, as 256 bricks
    n = 1 << 30
    r16 = torch.randint(0, 256, (n,), dtype=torch.uint8, device="cuda")
    ladder = [("0 adds (wave-uniform vectors)", torch.full((n,), 200, dtype=torch.uint8, device="cuda")),
              ("1 add  (16 equal bytes, lanes differ)", r16[::16].repeat_interleave(16)),
              ("4 adds (words of 4 equal bytes)", r16[::4].repeat_interleave(4)),
              ("16 adds (random bytes)", r16)]
    for name, buf in ladder:
        ms = timed(lambda: vr.histogram_bricks(buf, 256), args.reps)
        say("ladder, 1 GiB, %-38s %.3f ms = %.2f TB/s" % (name + ":", ms, tb(n, ms)))
        res["ladder " + name.split("(")[0].strip()] = ms
    del ladder, r16, buf
    # two dimensions: the decode assembled densely
    ijk = np.array([vr.fill_volume_brick_map(8, 8, 15)[b] for b in range(B)], np.int64)
    dense = vr.assemble_bricks(dec, bd, ijk, (8, 8, 15))
    del dec
    torch.cuda.empty_cache()
    h2 = vr.histogram2d(dense, gd)
    assert np.array_equal(h2.sum(0), want), "the 2-D table's column sums disagree with the 1-D histogram"
    rows = h2.sum(1)
    say("vr_histogram2d of the dense volume: row 0 holds %.1f %% of the voxels, rows 0..3 %.1f %%, %d of 111 rows and %d of 28416 cells populated"
        % (100.0 * float(rows[0]) / nbytes, 100.0 * float(rows[:4].sum()) / nbytes, int((rows != 0).sum()), int((h2 != 0).sum())))
    two = [timed(lambda: vr.histogram2d(dense, gd), 3) for _ in range(5)]
    plain(1)
    try:
        two_plain = [timed(lambda: vr.histogram2d(dense, gd), 3) for _ in range(3)]
    finally:
        plain(0)
    say("k_hist2d         runs (ms) %s   median %.3f ms = %.2f TB/s of voxels = %.1f x the floor of one read (%.3f ms); "
        "without the wave-uniform path %s" % (" ".join("%.3f" % m for m in two), float(np.median(two)), tb(nbytes, float(np.median(two))),
                                               float(np.median(two)) / floor, floor, " ".join("%.3f" % m for m in two_plain)))
    res.update(hist2d_ms=two, hist2d_plain_ms=two_plain)
    say(json.dumps(res))
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
