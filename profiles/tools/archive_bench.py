"""Compressed brick-set archives on the bench volume:
python profiles/tools/archive_bench.py [--out FILE] [--bricks N] [--work DIR] [--legs a,b,...]

The parent process never opens the GPU: every leg runs as a child process of its own under a time limit, and a leg that
fails or runs out of time is reported as "unmeasured" while the others go on.  Legs (bench volume: 2048 x 2048 x 1920 as
960 bricks of 256 x 256 x 128, tolerance 1, 2 epochs; --bricks takes the first N bricks of it):
  prepare    build the set once, time vr_brickset_save_set, write the archive and report its size against the raw
             voxels and the block tables' share of it
  install8   8 bricks, five runs each, alternating: one vr_brickset_set_trees call against a loop of
             vr_brickset_set_tree (the host path, unchanged)
  install    every brick: vr_brickset_load_set_memory from pinned memory (parse, checksums, copies, kernels), and
             vr_brickset_set_trees alone on the same sections, five runs each; then one full-depth decode for scale
  playback   ms per timestep, archive -> decoded volume (pipeline.ArchivePlayer over T copies of the file, read through
             the page cache: they were written moments before) against raw -> build -> decode
             (pipeline.TimestepStreamer over the same voxels from pinned memory, no disk stage)
k_index_from_stream is not timed alone here (that takes a kernel trace of the install leg).
Writes the report to profiles/archive_bench.txt (or --out)."""
import argparse
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
LIMITS = {"prepare": 420, "install8": 300, "install": 420, "playback": 480}
BD, GD = (256, 256, 128), (2048, 2048, 1920)


def parse_archive(buf):
    """numpy view of a file's bytes -> (bricks, trees, num_active, dmaps, tables), sections as views into buf."""
    import numpy as np
    nb, D, M = (int(v) for v in buf[40:52].view("<i4"))
    n_blk = 1 << max(D - 12, 0)
    pad = lambda n: (n + 15) & ~15      # noqa: E731
    ent = buf[64:64 + 32 * nb].view("<i8").reshape(nb, 4)
    out = ([], [], [], [], [])
    for b in range(nb):
        off, tb, na = int(ent[b, 0]), int(ent[b, 1]), int(ent[b, 2])
        if off == 0:
            continue
        p = off
        dmap = buf[p:p + M + 1]
        p += pad(M + 1)
        top = buf[p:p + 2 * n_blk]
        p += pad(2 * n_blk)
        boff = buf[p:p + 4 * n_blk].view(np.uint32)
        p += pad(4 * n_blk)
        for lst, v in zip(out, (b, buf[p:p + tb], na, dmap, (boff, top))):
            lst.append(v)
    return out


def leg(name, args):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as g
    g.build()
    import numpy as np
    import torch
    import bench
    import volumerenderer_amd as vr
    from volumerenderer_amd.pipeline import ArchivePlayer, ArchiveSource, TimestepStreamer
    V = BD[0] * BD[1] * BD[2]
    B = args.bricks
    path = os.path.join(args.work, "bench.vrbs")
    say = lambda s: print("| " + s, flush=True)      # noqa: E731
    runs = lambda ms: " ".join("%.1f" % m for m in ms)      # noqa: E731

    def clock(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def volume():
        return bench.make_volume_gpu(torch, GD, BD, seed=12345).reshape(-1)[:B * V].contiguous()

    def pinned_file():
        n = os.path.getsize(path)
        t = torch.empty((n + 15) & ~15, dtype=torch.uint8).pin_memory()
        with open(path, "rb") as f:
            assert f.readinto(t.numpy()[:n]) == n
        return t, n

    if name == "prepare":
        bs = vr.BrickSet(B, BD, 1, 2).build(volume())
        bs.tree(0)                      # (the contiguous stream is made; not part of the save)
        ms = clock(lambda: bs.save_set(path))
        n = os.path.getsize(path)
        n_blk = 1 << max(sum(d.bit_length() - 1 for d in BD) - 12, 0)
        say("%d bricks of %s: vr_brickset_save_set %.0f ms; archive %d bytes = %.4f of the raw voxels (%d bytes); block tables %d bytes = %.4f of the archive"
            % (B, BD, ms, n, n / (B * V), B * V, B * 6 * n_blk, B * 6 * n_blk / n))
    elif name in ("install8", "install"):
        blob, n = pinned_file()
        bricks, trees, nas, dmaps, tables = parse_archive(blob.numpy()[:n])
        if name == "install8":
            k = min(8, len(bricks))
            top = sorted(np.argsort(nas)[-k:])          # the eight longest streams (the volume's first bricks are constant)
            sel = [[v[i] for i in top] for v in (bricks, trees, nas, dmaps, tables)]
            new, old = [], []
            for _ in range(5):
                a = vr.BrickSet(B, BD)
                new.append(clock(lambda: a.set_trees(*sel)))
                h = vr.BrickSet(B, BD)
                old.append(clock(lambda: [h.set_tree(b, t, na, d) for b, t, na, d in zip(*sel[:4])]))
                for b in sel[0]:
                    assert a.info(b) == h.info(b)
                del a, h
            say("install of %d bricks (%.1f M tokens): vr_brickset_set_trees runs (ms) %s; loop of vr_brickset_set_tree runs (ms) %s; slowest batched %s fastest host-path (%.1f vs %.1f ms)"
                % (k, sum(sel[2]) / 1e6, runs(new), runs(old), "<" if max(new) < min(old) else ">=", max(new), min(old)))
        else:
            bs = vr.BrickSet(B, BD)
            whole = [clock(lambda: bs.load_set(blob, nbytes=n)) for _ in range(5)]
            alone = [clock(lambda: bs.set_trees(bricks, trees, nas, dmaps, tables)) for _ in range(5)]
            out = torch.empty(B * V, dtype=torch.uint8, device="cuda")
            bs.decode(out)
            dec = [clock(lambda: bs.decode(out)) for _ in range(5)]
            say("install of all %d bricks (%.0f M tokens, %.2f GB): vr_brickset_load_set_memory runs (ms) %s; vr_brickset_set_trees alone (no parse, no checksums) runs (ms) %s; full-depth decode runs (ms) %s"
                % (len(bricks), sum(nas) / 1e6, n / 1e9, runs(whole), runs(alone), runs(dec)))
    elif name == "playback":
        T = 4
        paths = []
        for t in range(T):
            p = os.path.join(args.work, "t%d.vrbs" % t)
            if not os.path.exists(p):
                os.link(path, p)
            paths.append(p)
        player = ArchivePlayer(B, BD)
        src = ArchiveSource(paths)
        player.run(src)
        play = [clock(lambda: player.run(src)) / T for _ in range(3)]
        del player
        torch.cuda.empty_cache()
        host = volume().cpu().pin_memory()
        st = TimestepStreamer(B, BD, 1, 2)
        st.run([host] * T)
        raw = [clock(lambda: st.run([host] * T)) / T for _ in range(3)]
        say("playback, %d timesteps of %d bricks: archive -> decoded volume %s ms per timestep (files read through the page cache); raw -> build -> decode %s ms per timestep (voxels in pinned memory, no disk)"
            % (T, B, runs(play), runs(raw)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "archive_bench.txt"))
    ap.add_argument("--bricks", type=int, default=960)
    ap.add_argument("--work", default=None)
    ap.add_argument("--legs", default="prepare,install8,install,playback")
    ap.add_argument("--leg", default=None)
    args = ap.parse_args()
    if args.leg:
        return leg(args.leg, args)
    lines = []
    with tempfile.TemporaryDirectory(dir=args.work) as work:
        failed = False
        for name in args.legs.split(","):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", name, "--bricks", str(args.bricks), "--work", work]
            got = []
            try:
                if failed:
                    raise RuntimeError("an earlier leg failed: nothing more is started on the GPU")
                r = subprocess.run(cmd, capture_output=True, text=True, timeout=LIMITS[name])
                got = [ln[2:] for ln in r.stdout.splitlines() if ln.startswith("| ")]
                if r.returncode != 0:
                    raise RuntimeError("exit status %d: %s" % (r.returncode, (r.stderr or "").strip().splitlines()[-1:]))
            except Exception as ex:      # the leg's own lines, then what went wrong
                failed = True
                got.append("%s: unmeasured (%s)" % (name, ex))
            for ln in got:
                print(ln, flush=True)
            lines += got
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
