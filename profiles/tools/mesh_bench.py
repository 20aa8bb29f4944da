"""The iso-surface mesh (vr_isomesh_count / vr_isomesh_emit) on the bench volume:
python profiles/tools/mesh_bench.py [--out FILE] [--reps N] [--small]   (writes profiles/mesh_bench.txt unless --out says otherwise)

Builds the bench volume (2048 x 2048 x 1920, 960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs) once, decodes and
assembles it densely, and extracts the iso-surface at the iso value of default_params, cap off, with and without
gradients.  HIP-event medians of --reps calls after two warm-up calls:
  count   vr_isomesh_count with vr_debug_set("mesh_count_only", 1): the per-point pass alone (and its synchronise);
  scan    the whole vr_isomesh_count minus that: the three scan kernels, the 16-byte download;
  emit    vr_isomesh_emit, with and without gradients.
Each is set against the bytes the pass must move -- the volume once per pass, the workspace written (count) or read
(emit), the outputs written -- and a vr_skip_grid_build pass over the same volume, which also reads it exactly once, runs
in the same process as context.  If the whole volume's mesh has more vertices or triangles than 32-bit indices address,
the own box is halved along z until it fits; the box used is reported.  --small: a 512 x 512 x 256 corner, for rehearsals.
One process, one GPU.  Every step runs under a time limit of its own: a step that overruns ends the process with status
124 and a message naming the step; nothing is started after it."""
import argparse
import ctypes as C
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
from volumerenderer_amd import render as R  # noqa: E402


class step:
    """A time limit for one step of the run: the process ends (status 124) when the step overruns."""

    def __init__(self, name, seconds):
        self.name, self.seconds = name, seconds

    def _overrun(self):
        sys.stderr.write("mesh_bench: step '%s' ran past its %d s limit; stopping\n" % (self.name, self.seconds))
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_bench.txt"),
                    help="where the report (text + one JSON line) is written")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--small", action="store_true", help="a 512 x 512 x 256 volume of 8 bricks (rehearsal)")
    args = ap.parse_args()
    bd = (256, 256, 128)
    gd, grid = ((512, 512, 256), (2, 2, 2)) if args.small else ((2048, 2048, 1920), (8, 8, 15))
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
        del bricks, bs
        torch.cuda.synchronize()
    iso = vr.default_params().iso_value
    I3 = C.c_int64 * 3
    dims = I3(*gd)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vbytes = gd[0] * gd[1] * gd[2]
    say("bench volume %s, %d bricks of %s, iso_value %.6f (level %.3f), cap off, %d reps (median)"
        % (gd, B, bd, iso, float(np.float32(iso) * np.float32(255)), args.reps))

    # ---- the box: the whole volume, halved along z while the counts do not fit 32-bit indices
    hi_z = gd[2] - 1
    with step("count", 120):
        while True:
            desc = R.isomesh_desc(gd, iso, own_hi=(gd[0] - 1, gd[1] - 1, hi_z))
            nbytes = C.c_int64()
            assert L.vr_isomesh_workspace_bytes(dims, C.byref(desc), C.byref(nbytes)) == 0
            ws = torch.empty(nbytes.value, dtype=torch.uint8, device="cuda")
            counts = (C.c_uint64 * 2)()
            rc = L.vr_isomesh_count(C.c_void_p(vol.data_ptr()), dims, C.byref(desc), C.c_void_p(ws.data_ptr()), counts, stream)
            say("own cells z < %d: %d vertices, %d triangles, workspace %d bytes%s"
                % (hi_z, counts[0], counts[1], nbytes.value, "" if rc == 0 else " -- beyond 32-bit indices, halving the box"))
            if rc == 0:
                break
            assert rc == -7 and hi_z > 1, rc
            del ws
            hi_z //= 2
    nv, nt = int(counts[0]), int(counts[1])
    points = gd[0] * gd[1] * (hi_z + 1)
    read_vol = points                                         # every voxel of the point box once per pass
    res.update(own_hi_z=hi_z, points=points, vertices=nv, triangles=nt, workspace_bytes=nbytes.value)

    def count():
        rc = L.vr_isomesh_count(C.c_void_p(vol.data_ptr()), dims, C.byref(desc), C.c_void_p(ws.data_ptr()), counts, stream)
        assert rc == 0, ("vr_isomesh_count", rc, counts[0], counts[1])

    with step("time count and scan", 120):
        assert L.vr_debug_set(b"mesh_count_only", 1) == 0
        try:
            res["count_ms"] = timed(count, args.reps)
        finally:
            L.vr_debug_set(b"mesh_count_only", 0)
        res["count_scan_ms"] = timed(count, args.reps)
        res["scan_ms"] = res["count_scan_ms"] - res["count_ms"]
        assert (int(counts[0]), int(counts[1])) == (nv, nt)
    runs = (points + 63) // 64
    count_bytes = read_vol + 2 * points + 8 * runs
    scan_bytes = 3 * 8 * runs                                 # read, written back, read and written again by the add
    say("count  %8.3f ms  %7.1f GB/s of %d bytes (volume read once, 2 bytes per point and 8 per run written)"
        % (res["count_ms"], count_bytes / res["count_ms"] / 1e6, count_bytes))
    say("scan   %8.3f ms  %7.1f GB/s of %d bytes (8 bytes per run: read, written, read and written again)"
        % (res["scan_ms"], scan_bytes / max(res["scan_ms"], 1e-6) / 1e6, scan_bytes))

    pos = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    grad = torch.empty((nv, 3), dtype=torch.float32, device="cuda")
    tri = torch.empty((nt, 3), dtype=torch.int32, device="cuda")
    for name, gptr in (("emit", None), ("emit_gradients", C.c_void_p(grad.data_ptr()))):
        def emit():
            rc = L.vr_isomesh_emit(C.c_void_p(vol.data_ptr()), dims, C.byref(desc), C.c_void_p(ws.data_ptr()), nv, nt,
                                   C.c_void_p(pos.data_ptr()), gptr, C.c_void_p(tri.data_ptr()), stream)
            assert rc == 0, ("vr_isomesh_emit", rc)
        with step("time %s" % name, 120):
            res[name + "_ms"] = timed(emit, args.reps)
        out_bytes = 12 * nv * (2 if gptr else 1) + 12 * nt
        emit_bytes = read_vol + 2 * points + 8 * runs + out_bytes
        say("%-15s %8.3f ms  %7.1f GB/s of %d bytes (volume and workspace read once, %d bytes of mesh written)"
            % (name, res[name + "_ms"], emit_bytes / res[name + "_ms"] / 1e6, emit_bytes, out_bytes))
        res[name + "_bytes"] = emit_bytes
    res.update(count_bytes=count_bytes, scan_bytes=scan_bytes)

    with step("vr_skip_grid_build of the same volume", 120):
        grid_t = torch.empty(R._skip_grid_bytes(gd, 8), dtype=torch.uint8, device="cuda")
        res["skip_grid_ms"] = timed(lambda: vr.build_skip_grid(vol, gd, 8, out=grid_t), args.reps)
    say("context: vr_skip_grid_build (cell 8), which reads the volume once: %8.3f ms  %7.1f GB/s of %d bytes"
        % (res["skip_grid_ms"], vbytes / res["skip_grid_ms"] / 1e6, vbytes))
    say(json.dumps(res))
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
