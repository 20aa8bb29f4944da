"""The launches of a fixed set of decode calls, for comparing two commits:

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/decode_trace.py run > checksums.txt
  python profiles/tools/decode_trace.py lists DIR > launches.txt

`run` builds small sets and decodes them: uniform decodes at the cuts 0, Ds-1, Ds, D-4, D-3, D, D+1, D+7 of four 64^3
bricks, two 256 x 256 x 128 bricks (the tiled kernels) with each decode switch off and on, two 12 x 10 x 6 bricks
(general extents), a MidRangeTree set with its range stream and an opened golden file; then a per-brick decode and a
pool decode of 64 bricks of 32^3 with 33 coarse bricks.  It prints one CRC-32 per decoded buffer.  `lists` reduces the
trace to one line "kernel grid workgroup" per dispatch of the library's kernels, in the order the host dispatched them
(by start time the kernels of a build's side streams swap from run to run).  Both outputs of two commits are compared
with diff."""
import csv
import glob
import os
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def run():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import volumerenderer_amd as vr

    def field(shape, seed):
        rng = np.random.default_rng(seed)
        z, y, x = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
        h = shape[0] / 2 + 3 * np.sin(x * 0.4) + 2 * np.cos(y * 0.23)
        return np.clip(128 + 120 * np.tanh((z - h) / 3.0) + rng.integers(0, 3, shape), 0, 255).astype(np.uint8)

    def crc(what, t):
        torch.cuda.synchronize()
        print("%-40s %08x" % (what, zlib.crc32(t.cpu().numpy().tobytes())), flush=True)

    def uniform(name, bs, rng_stream=False):
        info = bs.info(0)
        D, M = info["orig_tree_depth"], info["max_tree_depth"]
        Ds = D - min(D, 6)
        for c in sorted({c for c in (0, Ds - 1, Ds, D - 4, D - 3, D, D + 1, M) if 0 <= c <= M}):
            crc("%s cut %d" % (name, c), bs.decode(cut_depth=c))
            if rng_stream:
                crc("%s range cut %d" % (name, c), bs.decode_range(cut_depth=c))

    def built(B, dims, variant=0, tol=1):
        X, Y, Z = dims
        bs = vr.BrickSet(B, dims, tol, 2, variant) if variant else vr.BrickSet(B, dims, tol, 2)
        bs.build(np.stack([field((Z, Y, X), 3 + b) for b in range(B)]))
        return bs

    uniform("64^3 x 4", built(4, (64, 64, 64)))
    tiled = built(2, (256, 256, 128))
    uniform("256x256x128 x 2", tiled)
    for sw in ("decode_walk", "decode_fine_v1", "decode_quad", "no_uniform_decode"):
        tiled.set_switch(sw, 1)
        uniform("256x256x128 x 2 " + sw, tiled)
        tiled.set_switch(sw, 0)
    uniform("12x10x6 x 2", built(2, (12, 10, 6)))
    uniform("midrange 128x32x16 x 3", built(3, (128, 32, 16), vr.VARIANT_MIDRANGE, 2), rng_stream=True)
    uniform("golden file", vr.BrickSet.open(os.path.join(ROOT, "tests", "golden", "ref_sphere_n3_16_tol1_ep2.tree.bin")))

    bs = built(64, (32, 32, 32))
    info = bs.info(0)
    D, M = info["orig_tree_depth"], info["max_tree_depth"]
    ijk = np.array([(i, j, k) for k in range(4) for j in range(4) for i in range(4)], np.int64)
    cuts = np.full(64, M, np.int32)
    cuts[:33] = [(0, 3, D - 7, D - 6, D - 3, D - 1)[b % 6] for b in range(33)]
    cuts[40::7] = -1
    out = torch.full((64 * bs.voxels_per_brick,), 0xA5, dtype=torch.uint8, device="cuda")
    bs.decode_lod(cuts, out=out)
    crc("lod 32^3 x 64", out)
    pool, table = bs.decode_lod_pool(cuts, ijk, (4, 4, 4))
    crc("pool 32^3 x 64, 33 coarse", pool)
    crc("pool table", table)


def lists(d):
    f = sorted(glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True))[0]
    rows = list(csv.DictReader(open(f)))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        name = r["Kernel_Name"]
        if "vr::" not in name:
            continue
        name = name.split("(")[0].replace("void ", "")
        print(name, "x".join(r["Grid_Size_" + a] for a in "XYZ"), "x".join(r["Workgroup_Size_" + a] for a in "XYZ"))


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 3 and sys.argv[1] == "lists":
        lists(sys.argv[2])
    else:
        sys.exit(__doc__)
