"""The level-of-detail pool against the dense LOD frame path on the bench volume:
python profiles/tools/lod_pool_bench.py [--out FILE] [--reps N]

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once and, for the
start camera (cuts from select_lod at pixel tolerance 1), a camera at the cube's centre and every brick at full depth,
1920 x 1080, times with HIP events (median of --reps after two warm-up calls):
  dense  decode_lod into a B*V brick buffer, assemble_bricks into a B*V volume, raycast
  pool   decode_lod_pool, raycast_pool
raycast and raycast_pool in composite and iso-surface mode, each without and with an 8^3 skip grid (the grid's build
is timed on its own).  Memory: pool bytes against 2*B*V.  Each case also checks that the two frames are equal."""
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
    ap.add_argument("--out", default=None, help="also write the report (text + one JSON line) here")
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
    bricks = torch.zeros(B * V, dtype=torch.uint8, device="cuda")
    vol = torch.zeros(B * V, dtype=torch.uint8, device="cuda")
    pool = torch.empty(B * V, dtype=torch.uint8, device="cuda")         # the largest pool (all full depth)
    table = torch.empty(B * 16, dtype=torch.uint8, device="cuda")
    frame = torch.empty((1080, 1920, 4), dtype=torch.float32, device="cuda")
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("bench volume %s, %d bricks of %s, orig_tree_depth %d, max_tree_depth %d, 1920 x 1080, %d reps (median), "
        "2*B*V = %d MiB" % (gd, B, bd, D, M, args.reps, 2 * B * V >> 20))
    cams = {"start": vr.default_camera()}
    c = vr.default_camera()
    c.pos[:] = (0.0, 0.0, 0.0)
    cams["centre"] = c
    for name in ("start", "centre", "full"):
        cam = cams.get(name, vr.default_camera())
        P0 = vr.default_params(1920, 1080, bd)
        cuts = np.full(B, M, np.int32) if name == "full" else vr.select_lod(cam, P0, bd, ijk, grid, D, M, 1.0)
        hist = {int(k): int(v) for k, v in zip(*np.unique(cuts, return_counts=True))}
        _, nbytes = vr.lod_pool_layout(bd, ijk, grid, cuts, D, M)
        r = {"cuts": hist, "pool_MiB": nbytes / 2**20, "dense_MiB": 2 * B * V / 2**20}
        bricks.zero_()
        vol.zero_()
        r["decode_lod_ms"] = timed(lambda: bs.decode_lod(cuts, out=bricks), args.reps)
        r["assemble_ms"] = timed(lambda: vr.assemble_bricks(bricks, bd, ijk, grid, out=vol), args.reps)
        r["decode_lod_pool_ms"] = timed(lambda: bs.decode_lod_pool(cuts, ijk, grid, pool=pool, table=table), args.reps)
        r["skip_grid_ms"] = timed(lambda: vr.build_skip_grid(vol, gd, 8), args.reps)
        r["skip_grid_pool_ms"] = timed(lambda: vr.build_skip_grid_pool(pool, table, bd, grid, 8), args.reps)
        sg, sgp = vr.build_skip_grid(vol, gd, 8), vr.build_skip_grid_pool(pool, table, bd, grid, 8)
        assert torch.equal(sg, sgp), "skip grids differ"
        for mode, mname in ((0, "composite"), (1, "iso")):
            for skip in (False, True):
                P, Pp = vr.default_params(1920, 1080, bd, mode), vr.default_params(1920, 1080, bd, mode)
                if skip:
                    vr.use_skip_grid(P, sg, 8)
                    vr.use_skip_grid(Pp, sgp, 8)
                key = "%s%s" % (mname, "_skip" if skip else "")
                r["raycast_%s_ms" % key] = timed(lambda: vr.raycast(vol, gd, cam, P, out=frame), args.reps)
                want = frame.clone()
                r["raycast_pool_%s_ms" % key] = timed(lambda: vr.raycast_pool(pool, table, bd, grid, cam, Pp, out=frame), args.reps)
                assert torch.equal(frame, want), ("frames differ", name, key)
        r["frame_dense_ms"] = r["decode_lod_ms"] + r["assemble_ms"] + r["raycast_composite_ms"]
        r["frame_pool_ms"] = r["decode_lod_pool_ms"] + r["raycast_pool_composite_ms"]
        say("%-7s cuts %s" % (name, hist))
        say("  memory    pool %8.1f MiB   dense (bricks + volume) %8.1f MiB   (%.3f x)"
            % (r["pool_MiB"], r["dense_MiB"], r["pool_MiB"] / r["dense_MiB"]))
        say("  decode    decode_lod_pool %7.3f ms   decode_lod %7.3f + assemble %7.3f = %7.3f ms"
            % (r["decode_lod_pool_ms"], r["decode_lod_ms"], r["assemble_ms"], r["decode_lod_ms"] + r["assemble_ms"]))
        for key in ("composite", "composite_skip", "iso", "iso_skip"):
            say("  raycast   %-15s pool %7.3f ms   dense %7.3f ms   (%.2f x)"
                % (key, r["raycast_pool_%s_ms" % key], r["raycast_%s_ms" % key],
                   r["raycast_pool_%s_ms" % key] / r["raycast_%s_ms" % key]))
        say("  skip grid pool %7.3f ms   dense %7.3f ms" % (r["skip_grid_pool_ms"], r["skip_grid_ms"]))
        say("  frame (composite, no grid)   pool %7.3f ms   dense %7.3f ms   target %s"
            % (r["frame_pool_ms"], r["frame_dense_ms"], "met" if r["frame_pool_ms"] <= r["frame_dense_ms"] else "NOT met"))
        res[name] = r
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
