"""Per-brick (view-dependent) decode on the bench volume: python profiles/tools/lod_bench.py [--out FILE] [--reps N]

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once and times
BrickSet.decode_lod against BrickSet.decode with HIP events (median of --reps, after two warm-up calls):
  full      every brick at max_tree_depth (the same kernels as decode: expected equal within noise)
  default   the start camera (0, 0, -0.75), fov 50, 1920 x 1080, cuts from select_lod at pixel tolerance 1
  inside    a camera at the cube's centre looking along +z: the bricks behind it and outside its fov are culled
and reports decoded voxels per ms for each.

--host-bricks B instead: the host time of one decode_lod call (planning, staging and enqueueing; the stream is idle when
the call starts and is not waited for) on B bricks of 32^3 with cuts of every class, median and minimum in microseconds."""
import argparse
import json
import time
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
    return float(np.median(ms)), ms


def host_time(B, reps):
    bd = (32, 32, 32)
    V = bd[0] * bd[1] * bd[2]
    g = torch.Generator(device="cuda").manual_seed(5)
    ramp = (torch.arange(B * V, device="cuda") // 97 % 200).to(torch.uint8)
    vox = ramp + torch.randint(0, 3, (B * V,), generator=g, device="cuda", dtype=torch.uint8)
    bs = vr.BrickSet(B, bd, 1, 2)
    bs.build(vox)
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    choices = [-1, 0, 3, D - 7, D - 6, D - 3, D - 1, D, M]
    cuts = np.array([choices[b % len(choices)] for b in range(B)], np.int32)
    out = torch.empty(B * V, dtype=torch.uint8, device="cuda")
    us = []
    for _ in range(reps + 5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        bs.decode_lod(cuts, out=out)
        us.append((time.perf_counter() - t0) * 1e6)
    torch.cuda.synchronize()
    us = us[5:]
    print("decode_lod host time, %d bricks of %s, %d calls: median %.1f us, min %.1f us" % (B, bd, reps, float(np.median(us)), min(us)), flush=True)
    print(json.dumps({"host_bricks": B, "median_us": float(np.median(us)), "min_us": min(us)}))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the report (text + one JSON line) here")
    ap.add_argument("--reps", type=int, default=15)
    ap.add_argument("--host-bricks", type=int, default=0, help="only the host time of one decode_lod call on this many 32^3 bricks")
    args = ap.parse_args()
    if args.host_bricks:
        return host_time(args.host_bricks, args.reps)
    bd, gd, grid = (256, 256, 128), (2048, 2048, 1920), (8, 8, 15)
    vox4 = bench.make_volume_gpu(torch, gd, bd, seed=12345)
    B = vox4.shape[0]
    V = bd[0] * bd[1] * bd[2]
    ijk = np.array([(b % grid[0], (b // grid[0]) % grid[1], b // (grid[0] * grid[1])) for b in range(B)], np.int64)
    bs = vr.BrickSet(B, bd, 1, 2)
    bs.build(vox4.reshape(-1))
    del vox4
    torch.cuda.synchronize()
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    out = torch.empty(B * V, dtype=torch.uint8, device="cuda")
    lod_out = torch.empty(B * V, dtype=torch.uint8, device="cuda")
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("bench volume %s, %d bricks of %s, orig_tree_depth %d, max_tree_depth %d, %d reps (median)" % (gd, B, bd, D, M, args.reps))
    dec_ms, dec_all = timed(lambda: bs.decode(out), args.reps)
    say("decode            %8.3f ms   %4d bricks  %9.0f voxels/ms" % (dec_ms, B, B * V / dec_ms))
    res["decode_ms"] = dec_ms
    P = vr.default_params(1920, 1080, bd)
    cams = {}
    cams["default"] = vr.default_camera()
    c = vr.default_camera()
    c.pos[:] = (0.0, 0.0, 0.0)
    cams["inside"] = c
    cases = [("full", np.full(B, M, np.int32))]
    for name, cam in cams.items():
        cases.append((name, vr.select_lod(cam, P, bd, ijk, grid, D, M, 1.0)))
    for name, cuts in cases:
        n = int(np.sum(cuts >= 0))
        ms, _ = timed(lambda: bs.decode_lod(cuts, out=lod_out), args.reps)
        hist = {int(k): int(v) for k, v in zip(*np.unique(cuts, return_counts=True))}
        say("decode_lod %-7s%8.3f ms   %4d bricks  %9.0f voxels/ms   (%.2f x decode)   cuts %s"
            % (name, ms, n, n * V / ms if ms > 0 else 0.0, ms / dec_ms, hist))
        res[name] = {"ms": ms, "bricks": n, "voxels_per_ms": n * V / ms if ms > 0 else 0.0, "cuts": hist}
        if name == "full":
            torch.cuda.synchronize()
            assert torch.equal(lod_out, out), "decode_lod at full depth differs from decode"
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
