"""The two-dimensional transfer-function marcher (vr_raycast_tf2d / vr_raycast_pool_tf2d) against the one-dimensional
ones on the bench volume: python profiles/tools/tf2d_bench.py [--out FILE] [--reps N]

shade_bench.py's set-up: the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs),
the start camera's level-of-detail cut (select_lod at pixel tolerance 1, VR_RENDER_SHADED) as a dense volume and as a
pool, 1920 x 1080, HIP events (median of --reps after two warm-up calls), dense and pool, each without and with an 8^3
skip grid, for tf_bench.py's two tables.  Per table, in one run:
  1-D lit     raycast_tf_shaded / raycast_pool_tf_shaded with the default Shading (head light)
  2-D lit     raycast_tf2d / raycast_pool_tf2d with the same Shading, the table being the 1-D table in 111 equal rows
  1-D unlit   raycast_tf / raycast_pool_tf
  2-D unlit   raycast_tf2d / raycast_pool_tf2d without a Shading
Every case asserts the 2-D = 1-D, grid = no-grid and pool = dense equalities (torch.equal)."""
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

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from shade_bench import TABLES, timed  # noqa: E402

ROWS = 111


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
    cam = vr.default_camera()
    W, H = 1920, 1080
    SHADED, COMPOSITE = vr._lib.RENDER_SHADED, vr._lib.RENDER_COMPOSITE
    cuts = vr.select_lod(cam, vr.default_params(W, H, bd, SHADED), bd, ijk, grid, D, M, 1.0)
    bricks = torch.zeros(B * V, dtype=torch.uint8, device="cuda")
    bs.decode_lod(cuts, out=bricks)
    vol = vr.assemble_bricks(bricks, bd, ijk, grid)
    del bricks
    pool, table = bs.decode_lod_pool(cuts, ijk, grid)
    sg, sgp = vr.build_skip_grid(vol, gd, 8), vr.build_skip_grid_pool(pool, table, bd, grid, 8)
    assert torch.equal(sg, sgp), "skip grids differ"
    frame = torch.empty((H, W, 4), dtype=torch.float32, device="cuda")
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say("bench volume %s, %d bricks of %s, start camera, cuts %s, %d x %d, %d reps (median), 2-D table: %d equal rows"
        % (gd, B, bd, {int(k): int(v) for k, v in zip(*np.unique(cuts, return_counts=True))}, W, H, args.reps, ROWS))
    sh = vr.Shading()
    for name, pts in TABLES.items():
        lut = vr.transfer_function_table(pts)
        tf1 = vr.TransferFunction(lut)
        tf2 = vr.TransferFunction2D(np.ascontiguousarray(np.broadcast_to(lut, (ROWS, 256, 4))))
        r = {}
        for lit in (True, False):
            want = None
            for two in (False, True):
                for kind in ("dense", "pool"):
                    for skip in (False, True):
                        Pk = vr.default_params(W, H, bd, SHADED if (lit or two) else COMPOSITE)
                        if skip:
                            vr.use_skip_grid(Pk, sg if kind == "dense" else sgp, 8)
                        s = sh if lit else None
                        if two and kind == "dense":
                            fn = lambda: vr.raycast_tf2d(vol, gd, cam, Pk, tf2, s, out=frame)        # noqa: E731
                        elif two:
                            fn = lambda: vr.raycast_pool_tf2d(pool, table, bd, grid, cam, Pk, tf2, s, out=frame)  # noqa: E731
                        elif kind == "dense" and lit:
                            fn = lambda: vr.raycast_tf_shaded(vol, gd, cam, Pk, tf1, sh, out=frame)        # noqa: E731
                        elif kind == "dense":
                            fn = lambda: vr.raycast_tf(vol, gd, cam, Pk, tf1, out=frame)        # noqa: E731
                        elif lit:
                            fn = lambda: vr.raycast_pool_tf_shaded(pool, table, bd, grid, cam, Pk, tf1, sh, out=frame)  # noqa: E731
                        else:
                            fn = lambda: vr.raycast_pool_tf(pool, table, bd, grid, cam, Pk, tf1, out=frame)  # noqa: E731
                        key = "%s_%s_%s%s" % ("2d" if two else "1d", "lit" if lit else "unlit", kind, "_skip" if skip else "")
                        r[key + "_ms"] = timed(fn, args.reps)
                        if want is None:
                            want = frame.clone()
                        assert torch.equal(frame, want), ("frames differ", name, key)
        say("%s" % name)
        for style in ("lit", "unlit"):
            for key in ("dense", "dense_skip", "pool", "pool_skip"):
                a, b = r["1d_%s_%s_ms" % (style, key)], r["2d_%s_%s_ms" % (style, key)]
                say("  %-5s %-11s 1-D %7.3f ms   2-D %7.3f ms   2-D / 1-D %.2f x" % (style, key, a, b, b / a))
        res[name] = r
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
