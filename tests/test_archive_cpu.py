"""The GPU-free half of the compressed brick-set archives (volumerenderer_amd/csrc/host_plan.*): the block table of a
stream, the per-block index walker that k_index_from_stream runs on the device, and the archive's writer and parser,
checked by tests/archive_main.cpp -- a stand-alone program built with plain g++ under the address and undefined-
behaviour sanitizers and run as a child process.  No device, nothing loaded into Python.

The streams are tests/refstream.py's; what the program compares the unit with is derived here in NumPy from their
Levels: block offsets by assemble's size recurrence, scalars from decode_levels."""
import os
import struct
import subprocess
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refstream as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "volumerenderer_amd", "csrc")
EXTENTS = [(4, 1, 2), (16, 8, 4), (128, 8, 4), (128, 8, 8), (32, 32, 16)]     # D = 3, 9, 12 (one block), 13 (two), 14
LAWS = ("std", "sat", "zero", "chain_ns")
DEAD = 0xFFFFFFFF


def node_offsets(lv, depth):
    """Token index of every depth-`depth` node (assemble's recurrence: subtree sizes bottom-up, offsets top-down);
    DEAD where the node does not exist."""
    D = lv.D
    cl = lv.chain_len.astype(np.int64)
    size = [None] * (D + 1)
    size[D] = (lv.tok[D] != 255).astype(np.int64) + np.where(cl >= 0, np.minimum(cl + 1, R.CHAIN), 0)
    for d in range(D - 1, -1, -1):
        below = size[d + 1].reshape(-1, 2)
        size[d] = np.where(lv.tok[d] == 255, 0, 1 + below[:, 0] + below[:, 1])
    off = np.zeros(1, np.int64)
    for d in range(depth):
        nxt = np.empty(2 << d, np.int64)
        nxt[0::2] = off + 1
        nxt[1::2] = off + 1 + size[d + 1][0::2]
        off = nxt
    return np.where(lv.tok[depth] == 255, DEAD, off).astype(np.uint32)


def heap(dec, depth):
    """1-based heap of the decoded scalars of depths 0 .. depth (entry 0 unused): a pruned node's value stands for the
    nodes below it, which is what decode_levels' val[j] holds at cut j."""
    return np.concatenate([np.zeros(1, np.uint8)] + [dec.val[j] for j in range(depth + 1)])


def case_bytes(lv):
    D = lv.D
    Dc, K = max(D - 12, 0), min(D, 6)
    Ds = D - K
    dec = R.decode_levels(lv)
    tree = R.pack(lv.tokens)
    top_val, idx_top = heap(dec, Dc), heap(dec, Ds)
    assert top_val.size == 2 << Dc and idx_top.size == 2 << Ds
    std_chain = int(tuple(lv.dmap[D + 1:]) == R.STD_CHAIN)
    head = struct.pack("<9q", *lv.dims, D, lv.tokens.size, tree.size, 1 << Dc, 1 << Ds, std_chain)
    return b"".join([head, lv.dmap.tobytes(), tree.tobytes(), node_offsets(lv, Dc).tobytes(), top_val.tobytes(),
                     idx_top.tobytes()])


def test_node_offsets_point_at_the_nodes_tokens():
    """The derivation itself, against the assembled stream: the token at a live node's offset is the node's."""
    for dims in EXTENTS:
        lv = R.make(dims, "mixed", "std")
        for depth in (0, max(lv.D - 12, 0), lv.D - min(lv.D, 6)):
            off = node_offsets(lv, depth)
            live = off != DEAD
            assert np.array_equal(live, lv.tok[depth] != 255)
            assert np.array_equal(lv.tokens[off[live].astype(np.int64)], lv.tok[depth][live])


def test_archive_unit_under_sanitizers(tmp_path):
    src = open(os.path.join(CSRC, "host_plan.h")).read() + open(os.path.join(CSRC, "host_plan.cpp")).read()
    assert "hip/" not in src and "hip_runtime" not in src           # the unit includes no HIP header
    cases = [case_bytes(R.make(dims, family, law)) for dims in EXTENTS for family in R.FAMILIES for law in LAWS]
    case_file = str(tmp_path / "cases.bin")
    with open(case_file, "wb") as f:
        f.write(struct.pack("<q", len(cases)))
        for c in cases:
            f.write(c)
    exe = str(tmp_path / "archive_main")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", os.path.join(ROOT, "tests", "archive_main.cpp"),
                           os.path.join(CSRC, "host_plan.cpp"), "-o", exe])
    r = subprocess.run([exe, case_file, str(tmp_path)], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "archive unit: %d cases ok" % len(cases) in r.stdout
