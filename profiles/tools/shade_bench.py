"""The gradient-shaded ray marcher (vr_raycast_tf_shaded / vr_raycast_pool_tf_shaded) against the unlit one on the bench
volume: python profiles/tools/shade_bench.py [--out FILE] [--reps N]

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once, decodes the
start camera's level-of-detail cut (select_lod at pixel tolerance 1, VR_RENDER_SHADED: the two-voxel grow) both as a
dense volume (decode_lod + assemble) and as a pool (decode_lod_pool), and times at 1920 x 1080, start camera, with HIP
events (median of --reps after two warm-up calls), dense and pool, each without and with an 8^3 skip grid:
  unlit   raycast_tf / raycast_pool_tf
  lit     raycast_tf_shaded / raycast_pool_tf_shaded with the default Shading (head light)
for tf_bench.py's two tables, `opaque` and `light_clear`.  Each case asserts that the frames with and without the grid
and the pool and dense frames are equal."""
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

TABLES = {
    "opaque": [(0, 0.1, 0.2, 0.8, 0.25), (128, 0.9, 0.5, 0.1, 0.5), (255, 1.0, 1.0, 1.0, 0.9)],
    "light_clear": [(0, 0.0, 0.0, 0.0, 0.0), (20, 0.2, 0.3, 0.9, 0.0), (128, 0.9, 0.5, 0.1, 0.4), (255, 1.0, 1.0, 1.0, 0.9)],
}


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
    cam = vr.default_camera()
    W, H = 1920, 1080
    cuts = vr.select_lod(cam, vr.default_params(W, H, bd, vr._lib.RENDER_SHADED), bd, ijk, grid, D, M, 1.0)
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

    say("bench volume %s, %d bricks of %s, start camera, cuts %s, %d x %d, %d reps (median)"
        % (gd, B, bd, {int(k): int(v) for k, v in zip(*np.unique(cuts, return_counts=True))}, W, H, args.reps))
    P = vr.default_params(W, H, bd)
    res["raycast_composite_ms"] = timed(lambda: vr.raycast(vol, gd, cam, P, out=frame), args.reps)
    say("  raycast (greyscale compositor)   %7.3f ms  %7.1f fps" % (res["raycast_composite_ms"], 1e3 / res["raycast_composite_ms"]))
    sh = vr.Shading()
    for name, pts in TABLES.items():
        tf = vr.TransferFunction.from_points(pts)
        r = {}
        for lit in (False, True):
            want = None
            for kind in ("dense", "pool"):
                for skip in (False, True):
                    Pk = vr.default_params(W, H, bd, vr._lib.RENDER_SHADED if lit else vr._lib.RENDER_COMPOSITE)
                    if skip:
                        vr.use_skip_grid(Pk, sg if kind == "dense" else sgp, 8)
                    if kind == "dense" and lit:
                        fn = lambda: vr.raycast_tf_shaded(vol, gd, cam, Pk, tf, sh, out=frame)        # noqa: E731
                    elif kind == "dense":
                        fn = lambda: vr.raycast_tf(vol, gd, cam, Pk, tf, out=frame)        # noqa: E731
                    elif lit:
                        fn = lambda: vr.raycast_pool_tf_shaded(pool, table, bd, grid, cam, Pk, tf, sh, out=frame)  # noqa: E731
                    else:
                        fn = lambda: vr.raycast_pool_tf(pool, table, bd, grid, cam, Pk, tf, out=frame)  # noqa: E731
                    key = "%s_%s%s" % ("lit" if lit else "unlit", kind, "_skip" if skip else "")
                    r[key + "_ms"] = timed(fn, args.reps)
                    if want is None:
                        want = frame.clone()
                    assert torch.equal(frame, want), ("frames differ", name, key)
        say("%s" % name)
        for key in ("dense", "dense_skip", "pool", "pool_skip"):
            u, l = r["unlit_" + key + "_ms"], r["lit_" + key + "_ms"]
            say("  %-11s unlit %7.3f ms   lit %7.3f ms   lit / unlit %.2f x" % (key, u, l, l / u))
        res[name] = r
    say(json.dumps(res))
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
