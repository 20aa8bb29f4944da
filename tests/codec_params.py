"""The tolerance and epoch ladders of test_codec_params_cpu.py and test_gpu_codec_params.py: values, shapes, volumes and
case lists in one place, so that the CPU census speaks about exactly the cases the GPU module runs.

Shapes are (z, y, x); the comments name them X x Y x Z.  Nothing here needs a GPU."""
import json
import os

import numpy as np

from test_gpu_codec import rm_like, _mixed_volume
from test_gpu_const_boxes import MIX_VALUES, _mixed

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
KNOWN_ANSWERS = os.path.join(GOLD, "codec_param_known_answers.json")

# Every value the suite ran before lies in tolerance 0 .. 12 and max_epochs 0 .. 5.  The ladder goes on from there: the
# powers of two and their neighbours up to the largest leaf error (255), the first value no leaf error reaches (256),
# the ends of the signed and unsigned 16-bit ranges (the fused prune kernels carry the tolerance in 16-bit lanes) and
# the largest value the interface takes.
TOL_X = (13, 16, 31, 32, 63, 64, 100, 127, 128, 200, 254, 255, 256, 257, 1000, 32767, 32768, 32769, 40000, 65535,
         65536, 65537, 2 ** 31 - 1)
TOL_THIN = (13, 64, 255, 256, 32767, 32769, 65536, 2 ** 31 - 1)
EP_X = (6, 8, 13, 40, 200)
EP_TOL = (0, 1, 13)
TOL_SETTINGS = [(t, e) for t in TOL_X for e in (0, 2)]
EP_SETTINGS = [(t, e) for e in EP_X for t in EP_TOL]

S9, S12, S14, S15, S19 = (8, 8, 8), (16, 16, 16), (16, 32, 32), (32, 32, 32), (64, 64, 128)
G840, G15360 = (7, 10, 12), (24, 16, 40)       # 12 x 10 x 7 and 40 x 16 x 24: general extents
IDX64 = (16, 32, 128)
CPU_SHAPES = [S9, S12, S14, S15, G840, G15360]
VOLUMES = ("noise", "rm_like", "mixed")
VARIANTS = {"kd": 0, "guarded": 1, "mid": 2}


def sid(shape):
    return "%dx%dx%d" % (shape[2], shape[1], shape[0])


def volume(name, shape, seed=0):
    """noise, the smooth rm_like field and _mixed_volume of test_gpu_codec.py; `const<k>`: the constant-block mixes of
    test_gpu_const_boxes._mixed (box k % boxes busy, the others constant), for shapes of whole 4096-leaf boxes."""
    if name == "noise":
        return np.random.default_rng(1000 + seed).integers(0, 256, shape, dtype=np.uint8)
    if name == "rm_like":
        return rm_like(shape, 3 + seed)
    if name == "mixed":
        return _mixed_volume(np.random.default_rng(2000 + seed), shape)
    if name.startswith("const"):
        from oracle import oracle as O
        nb = shape[0] * shape[1] * shape[2] // 4096
        k = int(name[5:])
        return _mixed(O, shape, 3000 + k + seed, MIX_VALUES, busy=(k % nb,))
    raise KeyError(name)


# the constant-block mix of each shape of whole 4096-leaf boxes: found by a search over k on the CPU oracle for a brick
# that, at tolerance >= 256 and two epochs, holds blocks pruned whole next to a live block with pruned and coded leaves
CONST_MIX = {S14: "const2", S15: "const6", IDX64: "const5", S19: "const6"}


def gpu_volumes(shape):
    """volume names of the GPU tolerance ladder for `shape`"""
    return VOLUMES + ((CONST_MIX[shape],) if shape in CONST_MIX else ())


def mixes_dead_and_live_blocks(name, shape):
    """The cases whose high-tolerance streams must hold both kinds of block (test_codec_params_cpu.py census).  Noise
    cannot: no 4096-leaf block of it is ever pruned whole; nor can the smooth fields below 128 x 64 x 64."""
    return name.startswith("const") or (shape == S19 and name in ("rm_like", "mixed"))


_ORACLE = {}


def oracle_tree(O, name, shape, tol, ep, variant, seed=0):
    """The oracle's build of one case, made once per session and never changed."""
    key = (name, shape, tol, ep, variant, seed)
    if key not in _ORACLE:
        _ORACLE[key] = O.OracleTree(volume(name, shape, seed), tolerance=tol, max_epochs=ep, midrange=variant == 2,
                                    guarded=variant != 0).build()
    return _ORACLE[key]


# ---- the GPU module's cases ---------------------------------------------------------------------------------------
def tolerance_cases():
    """(shape, tolerance, [(epochs, variant, volume name)]): the full ladder on the small, fused and skip-block shapes,
    the thinned one on the general, 64-bit-offset and region-decode shapes.  One entry is one test: the largest shape,
    where the oracle takes a few tenths of a second per build, gets an entry per epoch setting and variant."""
    out = []
    for shape in (S9, S12, S14, S15):
        for tol in TOL_X:
            out.append((shape, tol, [(ep, v, n) for ep in (0, 2) for v in (0, 1, 2) for n in gpu_volumes(shape)]))
    for shape in (G840, G15360, IDX64):
        for tol in TOL_THIN:
            out.append((shape, tol, [(ep, v, n) for ep in (0, 2) for v in (0, 1, 2) for n in gpu_volumes(shape)]))
    for tol in TOL_THIN:
        for ep in (0, 2):
            for v in (0, 1, 2):
                out.append((S19, tol, [(ep, v, n) for n in gpu_volumes(S19)]))
    return out


def epoch_cases():
    """(shape, epochs, [(tolerance, variant, volume name)]), one entry per test"""
    out = [(shape, ep, [(t, v, n) for t in EP_TOL for v in (0, 2) for n in ("rm_like", "noise")])
           for shape in (S12, S15, G15360) for ep in EP_X]
    return out + [(S19, ep, [(t, v, n) for n in ("rm_like", "noise")]) for ep in EP_X for t in EP_TOL for v in (0, 2)]


def high_tolerance_fused_cases():
    """Every (volume name, shape, tolerance, epochs) of the GPU module with tolerance >= 256, a level loop that runs
    and D >= 14 (power-of-two extents: whole 4096-leaf boxes)."""
    seen = []
    for shape, tol, rest in tolerance_cases():
        if shape in (S14, S15, S19, IDX64) and tol >= 256:
            seen += [(n, shape, tol, ep) for ep, v, n in rest if ep >= 1 and v == 0]
    return seen


# ---- the oracle's stream, box by box (test_gpu_uniform_blocks._box_tokens with the leaves told apart) --------------
def box_leaf_census(ref):
    """Per depth-(D-12) box of a D >= 12 tree: None where an ancestor or the box's own root is pruned (the whole
    4096-leaf block is dead), else (leaves under a pruned node or pruned themselves, live leaves with a non-zero code)."""
    D, chain = ref.origTreeDepth, ref.maxTreeDepth - ref.origTreeDepth
    top = D - 12
    n = int(ref.numActiveNodes)
    t = np.asarray(ref.tree)
    tok = ((t[:, None] >> np.array([0, 2, 4, 6], np.uint8)) & 3).reshape(-1)[:n].tolist()
    out = [None] * (1 << top)

    def walk(i, d, idx):
        """preorder from token i, a node of depth d whose leftmost box is idx; returns the next token"""
        stack = [(d, idx)]
        while stack:
            d, idx = stack.pop()
            c = tok[i]
            i += 1
            if d == top:
                out[idx] = [0, 0]
            box = idx if d >= top else None
            if c == 3:
                if d == top:
                    out[idx] = None
                elif d > top:
                    out[box][0] += 1 << (D - d)
                continue
            if d < D:
                if d < top:
                    span = 1 << (top - d - 1)
                    stack.append((d + 1, idx + span))
                    stack.append((d + 1, idx))
                else:
                    stack.append((d + 1, idx))
                    stack.append((d + 1, idx))
            else:
                out[box][1] += c != 0
                for _ in range(chain):
                    c = tok[i]
                    i += 1
                    if c == 3:
                        break
        return i

    assert walk(0, 0, 0) == len(tok)
    return out


# ---- known answers ------------------------------------------------------------------------------------------------
# (volume name, seed, shape, tolerance, epochs, variant name): both sides of 256 with no level loop, both sides of the
# 16-bit ranges with one, long epoch runs, a general extent; small enough for the file to stay a few KB
KNOWN_CASES = ([("noise", 0, S12, t, 0, "kd") for t in (64, 100, 255, 256, 40000)]
               + [("noise", 0, S15, t, 2, v) for t in (13, 64, 32767, 32769, 65536, 2 ** 31 - 1) for v in ("kd", "mid")]
               + [("rm_like", 0, S15, 1, e, "kd") for e in (6, 8, 13, 40)]
               + [("rm_like", 0, S12, 13, 40, "mid"), ("mixed", 0, S14, 256, 2, "kd"), ("mixed", 0, S14, 40000, 0, "mid"),
                  ("const2", 0, S14, 65537, 2, "kd"), ("noise", 0, S9, 32769, 2, "kd"), ("rm_like", 0, G840, 257, 2, "mid"),
                  ("mixed", 0, G15360, 1000, 6, "kd")])


def known_record(O, tree, name, seed, shape, tol, ep, vname):
    """One record of tests/golden/codec_param_known_answers.json from a built tree (reference, oracle or GPU adapter:
    numActiveNodes, tree, tree_range and levelCut())."""
    rec = dict(volume=name, seed=seed, shape=list(shape), tolerance=tol, max_epochs=ep, variant=vname,
               numActiveNodes=int(tree.numActiveNodes), tree_fnv="%016x" % O.fnv1a64(tree.tree))
    if vname == "mid":
        rec["tree_range_fnv"] = "%016x" % O.fnv1a64(tree.tree_range)
    rec["voxels_fnv"] = "%016x" % O.fnv1a64(tree.levelCut())
    return rec


def known_answers():
    return json.load(open(KNOWN_ANSWERS))["cases"]
