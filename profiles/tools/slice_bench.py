"""The slice views (vr_reslice) on the bench volume:
python profiles/tools/slice_bench.py [--out FILE] [--reps N]   (writes profiles/slice_bench.txt unless --out says otherwise)

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once, decodes and
assembles it densely, and times 2048 x 2048 frames (median of --reps after two warm-up calls):
  (a) dense NEAREST and LINEAR thin slices -- axial, coronal, sagittal and one oblique plane -- under each candidate wave
      footprint of k_reslice (8 x 8, 16 x 4, 64 x 1 pixels; vr_debug_set("reslice_tile_w")), with HIP events.  The
      footprint with the lowest total over the four planes (both filters) is the one to keep; every candidate's figures
      are recorded, and the frames of the candidates are asserted equal.
  (b) a 64-layer MAX slab against vr_raycast_projection MAX of the same volume at the same frame size, as context.
One process, one GPU.  Every step runs under a time limit of its own: a step that overruns ends the process with
status 124 and a message naming the step; nothing is started after it."""
import argparse
import json
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import __graft_entry__ as g  # noqa: E402

g.build()
import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import volumerenderer_amd as vr  # noqa: E402

TILES = (8, 16, 64)
FILTERS = ("nearest", "linear")
N = 2048                                # the frame is N x N


class step:
    """A time limit for one step of the run: the process ends (status 124) when the step overruns."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def _overrun(self):
        sys.stderr.write("slice_bench: step '%s' ran past its %d s limit; stopping\n" % (self.name, self.seconds))
        sys.stderr.flush()
        os._exit(124)

    def __enter__(self):
        self.timer = threading.Timer(self.seconds, self._overrun)
        self.timer.daemon = True
        self.timer.start()
        print("[step] %s" % self.name, flush=True)

    def __exit__(self, *exc):
        self.timer.cancel()
        return False


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


def frame_plane(gd, axis, index, layers=1, filter="linear"):
    """The N x N frame over the whole cross-section through voxel layer `index` along `axis` (axis_aligned's image axes)."""
    p = vr.SlicePlane.axis_aligned(gd, axis, index, layers=layers, filter=filter)
    cu, cv = [k for k in range(3) if p.du[k] != 0.0][0], [k for k in range(3) if p.dv[k] != 0.0][0]
    du, dv, o = [0.0] * 3, [0.0] * 3, list(p.origin)
    du[cu], dv[cv], o[cu], o[cv] = 1.0 / N, 1.0 / N, 0.5 / N, 0.5 / N
    return vr.SlicePlane(N, N, o, du, dv, p.dw, layers, filter)


def planes(gd, filter):
    return {"axial": frame_plane(gd, 2, 1000, filter=filter), "coronal": frame_plane(gd, 1, 1000, filter=filter),
            "sagittal": frame_plane(gd, 0, 1000, filter=filter),
            "oblique": vr.SlicePlane.from_frame((0.5, 0.5, 0.5), (1.0, 0.3, 0.2), (-0.2, 1.0, 0.4), N, N, 0.9 / N, 1, None, filter)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "slice_bench.txt"),
                    help="where the report (text + one JSON line) is written")
    ap.add_argument("--reps", type=int, default=15)
    args = ap.parse_args()
    bd, gd, grid = (256, 256, 128), (2048, 2048, 1920), (8, 8, 15)
    L = vr._lib.lib()
    lines, res = [], {}

    def say(s):
        print(s, flush=True)
        lines.append(s)

    with step("build the bench volume", 240):
        vox4 = bench.make_volume_gpu(torch, gd, bd, seed=12345)
        B = vox4.shape[0]
        V = bd[0] * bd[1] * bd[2]
        ijk = np.array([(b % grid[0], (b // grid[0]) % grid[1], b // (grid[0] * grid[1])) for b in range(B)], np.int64)
        bs = vr.BrickSet(B, bd, 1, 2)
        bs.build(vox4.reshape(-1))
        del vox4
        torch.cuda.synchronize()
    with step("decode and assemble the dense volume", 120):
        bricks = torch.empty(B * V, dtype=torch.uint8, device="cuda")
        bs.decode(out=bricks)
        vol = vr.assemble_bricks(bricks, bd, ijk, grid)
        torch.cuda.synchronize()
    frame = torch.empty((N, N, 4), dtype=torch.float32, device="cuda")
    grey = vr.Projection("max")
    say("bench volume %s, %d bricks of %s, %d x %d frames, %d reps (median)" % (gd, B, bd, N, N, args.reps))

    # ---- (a) the wave footprint
    say("(a) dense thin slices, ms per frame by wave footprint (pixels across x down)")
    a = {}
    try:
        for flt in FILTERS:
            for name, plane in planes(gd, flt).items():
                want = None
                for tw in TILES:
                    with step("(a) %s %s %dx%d" % (flt, name, tw, 64 // tw), 60):
                        assert L.vr_debug_set(b"reslice_tile_w", tw) == 0
                        a["%s_%s_%d" % (flt, name, tw)] = timed(lambda: vr.reslice(vol, gd, plane, grey, out=frame), args.reps)
                        if want is None:
                            want = frame.clone()
                        assert torch.equal(frame, want), ("frames differ", flt, name, tw)
                say("  %-8s %-9s" % (flt, name)
                    + "".join("  %2dx%-2d %7.3f" % (tw, 64 // tw, a["%s_%s_%d" % (flt, name, tw)]) for tw in TILES))
    finally:
        L.vr_debug_set(b"reslice_tile_w", 16)       # the library's default
    totals = {tw: sum(v for k, v in a.items() if k.endswith("_%d" % tw)) for tw in TILES}
    best = min(TILES, key=lambda tw: totals[tw])
    say("  total over the four planes and both filters:" + "".join("  %2dx%-2d %7.3f" % (tw, 64 // tw, totals[tw]) for tw in TILES)
        + "  -> lowest: %dx%d" % (best, 64 // best))
    res["a"], res["a_totals"], res["a_best_tile_w"] = a, {str(k): v for k, v in totals.items()}, best

    # ---- (b) a thick slab against the perspective MIP
    with step("(b) 64-layer MAX slab and vr_raycast_projection MAX", 120):
        c = {}
        for flt in FILTERS:
            slab = frame_plane(gd, 2, 968, 64, flt)
            c["slab64_%s_ms" % flt] = timed(lambda: vr.reslice(vol, gd, slab, grey, out=frame), args.reps)
        P = vr.default_params(N, N, bd, vr._lib.RENDER_PROJECTION)
        cam = vr.default_camera()
        c["raycast_projection_max_ms"] = timed(lambda: vr.raycast_projection(vol, gd, cam, P, grey, out=frame), args.reps)
    say("(b) axial 64-layer MAX slab: nearest %.3f ms, linear %.3f ms; vr_raycast_projection MAX (start camera, no grid) %.3f ms"
        % (c["slab64_nearest_ms"], c["slab64_linear_ms"], c["raycast_projection_max_ms"]))
    res["b"] = c
    say(json.dumps(res))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
