"""The launches and results of a fixed set of installs by both engines, for comparing two commits, and their host time:

  rocprofv3 --kernel-trace --output-format csv -d DIR -- python profiles/tools/install_trace.py run > checksums.txt
  python profiles/tools/decode_trace.py lists DIR > launches.txt
  python profiles/tools/install_trace.py time

`run` takes the streams of small built sets (four bricks each of 32 x 16 x 16, two blocks; 128 x 64 x 64, the tiled
kernels; 12 x 6 x 5, general extents; 4 x 2 x 2, no fine side-car; one brick's map gets a grown-branch distance that is
not the standard one) and installs them, in this order: vr_brickset_set_trees into a fresh set and again, rotated, into
the same set; vr_brickset_save_set, vr_brickset_open_set and vr_brickset_load_set of that file; then
vr_brickset_set_tree brick by brick into a fresh set and again, rotated; then one brick of each set by the other
engine.  After every step it prints one CRC-32 per brick of vr_brickset_info / _get_tree / _get_distance_map and one per
uniform decode at the cuts 0, Ds-1, Ds, D-3, D and D+7, which between them read every index array an install writes
(offsets, scalars, the fine side-cars, the heap above the index depth).  decode_trace.py's `lists` reduces the trace.
`time` prints host milliseconds of eight vr_brickset_set_tree calls into a fresh 8-brick set of 32 x 16 x 16 (the first
call's reset included), of eight more into the same set, and of one vr_brickset_set_trees call, nine runs each."""
import os
import sys
import tempfile
import time
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
EXTENTS = [(32, 16, 16), (128, 64, 64), (12, 6, 5), (4, 2, 2)]


def streams(vr, np, B, dims):
    """[(tree bytes, tokens, map)] of B built bricks; the last one's first grown-branch distance is off by one"""
    X, Y, Z = dims
    rng = np.random.default_rng(X * 31 + Y * 7 + Z)
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    vox = np.stack([np.clip(128 + 100 * np.sin(x * 0.5 + b) * np.cos(y * 0.3) + 8 * z + rng.integers(0, 4, (Z, Y, X)), 0, 255).astype(np.uint8)
                    for b in range(B)])
    bs = vr.BrickSet(B, dims, 1, 2).build(vox)
    out = [(bs.tree(b), bs.info(b)["num_active_nodes"], bs.distance_map(b)) for b in range(B)]
    D = bs.info(0)["orig_tree_depth"]
    out[-1][2][D + 1] += 1
    return out


def run():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import volumerenderer_amd as vr
    from volumerenderer_amd.codec import stream_block_table

    def report(what, bs):
        info = bs.info(0)
        D, M = info["orig_tree_depth"], info["max_tree_depth"]
        Ds = D - min(D, 6)
        c = 0
        for b in range(bs.num_bricks):
            c = zlib.crc32(repr(sorted(bs.info(b).items())).encode() + bs.tree(b).tobytes() + bs.distance_map(b).tobytes(), c)
        print("%-44s state %08x" % (what, c), flush=True)
        for cut in sorted({k for k in (0, Ds - 1, Ds, D - 3, D, M) if 0 <= k <= M}):
            out = bs.decode(cut_depth=cut)
            torch.cuda.synchronize()
            print("%-44s cut %2d %08x" % (what, cut, zlib.crc32(out.cpu().numpy().tobytes())), flush=True)

    B = 4
    with tempfile.TemporaryDirectory() as work:
        for dims in EXTENTS:
            tag = "%dx%dx%d" % dims
            s = streams(vr, np, B, dims)
            cols = lambda order: [list(range(B))] + [[s[i][k] for i in order] for k in range(3)]    # noqa: E731
            tabs = lambda order: [stream_block_table(dims, *s[i]) for i in order]                    # noqa: E731
            first, turned = list(range(B)), [(i + 1) % B for i in range(B)]
            a = vr.BrickSet(B, dims)
            a.set_trees(*cols(first), tables=tabs(first))
            report(tag + " set_trees fresh", a)
            a.set_trees(*cols(turned), tables=None)
            report(tag + " set_trees again, tables made", a)
            path = os.path.join(work, tag + ".vrbs")
            a.save_set(path)
            report(tag + " open_set", vr.BrickSet.open_set(path))
            a.set_trees(*cols(first), tables=tabs(first))
            report(tag + " load_set", a.load_set(path))
            h = vr.BrickSet(B, dims)
            for b in range(B):
                h.set_tree(b, *s[b])
            report(tag + " set_tree fresh", h)
            for b in range(B):
                h.set_tree(b, *s[turned[b]])
            report(tag + " set_tree again", h)
            h.set_trees([1], [s[0][0]], [s[0][1]], [s[0][2]], tables=[stream_block_table(dims, *s[0])])
            report(tag + " set_trees into the set_tree set", h)
            a.set_tree(2, *s[3])
            report(tag + " set_tree into the set_trees set", a)


def timing():
    sys.path.insert(0, ROOT)
    import numpy as np
    import torch
    import volumerenderer_amd as vr
    from volumerenderer_amd.codec import stream_block_table
    B, dims = 8, (32, 16, 16)
    s = streams(vr, np, B, dims)
    tabs = [stream_block_table(dims, *v) for v in s]
    cols = [list(range(B))] + [[v[k] for v in s] for k in range(3)]
    fresh, again, batch = [], [], []

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for _ in range(10):
        h = vr.BrickSet(B, dims)
        fresh.append(clock(lambda: [h.set_tree(b, *s[b]) for b in range(B)]))
        again.append(clock(lambda: [h.set_tree(b, *s[b]) for b in range(B)]))
        a = vr.BrickSet(B, dims)
        batch.append(clock(lambda: a.set_trees(*cols, tables=tabs)))
    for what, ms in (("8 x set_tree, fresh set", fresh), ("8 x set_tree, again", again), ("set_trees of 8, fresh set", batch)):
        print("%-28s runs (ms) %s" % (what, " ".join("%.3f" % m for m in ms[1:])), flush=True)      # (the first run warms up)


if __name__ == "__main__":
    if len(sys.argv) == 2 and sys.argv[1] == "run":
        run()
    elif len(sys.argv) == 2 and sys.argv[1] == "time":
        timing()
    else:
        sys.exit(__doc__)
