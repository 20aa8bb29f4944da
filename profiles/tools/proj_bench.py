"""The intensity projections (vr_raycast_projection / vr_raycast_pool_projection) on the bench volume:
python profiles/tools/proj_bench.py [--out FILE] [--reps N]   (writes profiles/proj_bench.txt unless --out says otherwise)

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once, decodes the
start camera's level-of-detail cut (select_lod at pixel tolerance 1, VR_RENDER_PROJECTION: the one-voxel grow) both as a
dense volume (decode_lod + assemble) and as a pool (decode_lod_pool), and times at 1920 x 1080, start camera, with HIP
events (median of --reps after two warm-up calls):
  partial  vr_raycast in VR_RENDER_PARTIAL mode on the dense volume: the same walk and the same fetches, with a dependent
           accumulation -- the yardstick of the same run;
  MAX, MIN, MEAN, dense and pool, each without and with an 8^3 skip grid.
Each op asserts that the frames with and without the grid and the pool and dense frames are equal.  The one bar: MAX,
dense, no grid <= 1.05 x partial, reported as met or MISSED in the text and as "bar_met" in the JSON line (recorded, not
gated: the run still writes its report)."""
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

OPS = ("max", "min", "mean")
KEYS = ("dense", "dense_skip", "pool", "pool_skip")


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "proj_bench.txt"),
                    help="where the report (text + one JSON line) is written")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
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
    cam = vr.default_camera()
    W, H = 1920, 1080
    MODE = vr._lib.RENDER_PROJECTION
    cuts = vr.select_lod(cam, vr.default_params(W, H, bd, MODE), bd, ijk, grid, D, M, 1.0)
    bricks = torch.zeros(B * V, dtype=torch.uint8, device="cuda")
    bs.decode_lod(cuts, out=bricks)
    vol = vr.assemble_bricks(bricks, bd, ijk, grid)
    del bricks
    pool, table = bs.decode_lod_pool(cuts, ijk, grid)
    sg, sgp = vr.build_skip_grid(vol, gd, 8), vr.build_skip_grid_pool(pool, table, bd, grid, 8)
    assert torch.equal(sg, sgp), "skip grids differ"
    cells = sg.reshape(-1, 2)
    const_cells = float((cells[:, 0] == cells[:, 1]).float().mean())
    zero_cells = float((cells[:, 1] == 0).float().mean())
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    lines, res = [], {"const_cells": const_cells, "zero_cells": zero_cells}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("bench volume %s, %d bricks of %s, start camera, cuts %s, %d x %d, %d reps (median)"
        % (gd, B, bd, {int(k): int(v) for k, v in zip(*np.unique(cuts, return_counts=True))}, W, H, args.reps))
    say("8^3 skip grid: %.1f %% of the cells have equal bounds, %.1f %% are all zero" % (100 * const_cells, 100 * zero_cells))
    Pp = vr.default_params(W, H, bd, vr._lib.RENDER_PARTIAL)
    res["partial_ms"] = timed(lambda: vr.raycast(vol, gd, cam, Pp, out=frame), args.reps)
    say("  vr_raycast VR_RENDER_PARTIAL, dense  %7.3f ms" % res["partial_ms"])
    r, covered = {}, {}
    for op in OPS:
        proj = vr.Projection(op)
        want = None
        for kind in ("dense", "pool"):
            for skip in (False, True):
                Pk = vr.default_params(W, H, bd, MODE)
                if skip:
                    vr.use_skip_grid(Pk, sg if kind == "dense" else sgp, 8)
                if kind == "dense":
                    fn = lambda: vr.raycast_projection(vol, gd, cam, Pk, proj, out=frame)        # noqa: E731
                else:
                    fn = lambda: vr.raycast_pool_projection(pool, table, bd, grid, cam, Pk, proj, out=frame)  # noqa: E731
                key = "%s_%s%s" % (op, kind, "_skip" if skip else "")
                r[key + "_ms"] = timed(fn, args.reps)
                if want is None:
                    want = frame.clone()
                assert torch.equal(frame, want), ("frames differ", key)
        covered[op] = float((want[..., 3] > 0).float().mean())
    for key in KEYS:
        say("  %-11s" % key + "".join("  %s %7.3f ms" % (op.upper().ljust(4), r["%s_%s_ms" % (op, key)]) for op in OPS))
    res.update(r)
    res["covered"] = covered
    say("grid speed-up: " + ", ".join(
        "%s dense %.2f x, pool %.2f x" % (op.upper(), r[op + "_dense_ms"] / r[op + "_dense_skip_ms"],
                                          r[op + "_pool_ms"] / r[op + "_pool_skip_ms"]) for op in OPS))
    ratio = r["max_dense_ms"] / res["partial_ms"]
    res["max_dense_over_partial"] = ratio
    res["bar_met"] = bool(ratio <= 1.05)
    say("MAX dense, no grid / VR_RENDER_PARTIAL = %.3f (bar: <= 1.05): %s; %.1f %% of the pixels are covered"
        % (ratio, "met" if ratio <= 1.05 else "MISSED", 100 * covered["max"]))
    say(json.dumps(res))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
