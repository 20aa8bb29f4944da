#!/usr/bin/env python3
"""est_census_capture.py -- take the estimator's census log on the bench volume (input of est_census.py).

The log comes from a build of the library with -DVR_EST_CENSUS, which is never the package's own libvrhip.so: k_est_walk
then appends one record per event to a 64 MB device array, and vr_debug_est_census(out, capacity) (kd_encode.hip; declared
in no header: it exists in that build only) copies the records out and empties the log.  Build it beside the package,
with the flags of volumerenderer_amd/_build.py plus the macro:

  cd volumerenderer_amd/csrc && hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -shared -ffp-contract=off \\
      -DVR_EST_CENSUS -ldl -o /tmp/libvrhip_census.so kd_encode.hip kd_decode.hip raymarch.hip capi.hip compositor.hip \\
      error_table.hip histogram.hip kd_index.hip host_plan.cpp

  python profiles/tools/est_census_capture.py /tmp/libvrhip_census.so OUTDIR

One build of the 960 bench bricks (tolerance 1, two epochs, one level-loop stream) per setting; OUTDIR/census_<setting>.npy
is the (N, 4) uint32 log.  census_exact_old.npy (est_exact_bounds + est_old_schedule) is the trajectory log that
  python profiles/tools/est_census.py OUTDIR/census_exact_old.npy --write-text profiles/r12_est_census.txt
turns into the committed text; the other three show how each schedule's rounds really end (record kinds: kd_encode.hip).
"""
import ctypes as C
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)


def main():
    lib_path, out_dir = os.path.abspath(sys.argv[1]), sys.argv[2]
    os.makedirs(out_dir, exist_ok=True)
    import volumerenderer_amd._lib as _lib
    _lib.LIB_PATH = lib_path                 # before anything loads the library
    import torch
    import volumerenderer_amd as vr
    import bench
    gdims, bdims = (2048, 2048, 1920), (256, 256, 128)
    vox4 = bench.make_volume_gpu(torch, gdims, bdims, seed=12345)
    B = vox4.shape[0]
    vox = vox4.reshape(-1)
    fn = _lib.lib().vr_debug_est_census
    fn.restype = C.c_int64
    fn.argtypes = [C.c_void_p, C.c_int64]
    cap = 1 << 22
    buf = np.zeros((cap, 4), np.uint32)
    bs = vr.BrickSet(B, bdims, 1, 2)
    bs.set_concurrency(1)                    # brick ranges on internal streams would log range-relative brick numbers
    for name, exact, old in (("exact_old", 1, 1), ("quads_old", 0, 1), ("quads_new", 0, 0), ("exact_new", 1, 0)):
        bs.set_switch("est_exact_bounds", exact)
        bs.set_switch("est_old_schedule", old)
        bs.build(vox)
        torch.cuda.synchronize()
        n = fn(buf.ctypes.data, cap)
        assert 0 <= n <= cap, n
        print(name, "events", n, "est_exact_segments", sum(bs.info(b)["est_exact_segments"] for b in range(B)), flush=True)
        np.save(os.path.join(out_dir, "census_%s.npy" % name), buf[:n].copy())


if __name__ == "__main__":
    main()
