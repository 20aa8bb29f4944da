"""Many-brick sets without a GPU: the conditions tests/manybricks.py rests on, the oracle held to the reference codec on
its contents, the compact stream layout restated, and the brick-count limit, which is checked before the device."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import manybricks as MB  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# every set the GPU module builds: (dims, B, midrange)
SETS = [(MB.FUSED, B, False) for B in MB.FUSED_B] + [(d, B, False) for d in (MB.UNFUSED, MB.GENERAL) for B in MB.OTHER_B] \
    + [(MB.FUSED, B, True) for B in MB.MIDRANGE_B] + [(MB.TINY, 65535, False)]
# every oracle setting it uses: (dims, tolerance, epochs, midrange)
SETTINGS = [(MB.FUSED, 1, 2, False), (MB.FUSED, 6, 5, False), (MB.FUSED, 1, 2, True), (MB.UNFUSED, 1, 2, False),
            (MB.GENERAL, 1, 2, False), (MB.TINY, 1, 2, False)]


def _id(v):
    return "x".join(str(q) for q in v) if isinstance(v, tuple) else str(v)


# ---- the builder's conditions --------------------------------------------------------------------------------------
def test_period_is_coprime_with_every_stride():
    import math
    for k in (16, 32, 64, 1024):
        assert math.gcd(MB.PERIOD, k) == 1
    for B in (1025, 3000, 65535):
        c = MB.content_of(B)
        for k in MB.STEPS:
            assert not np.any(c[k:] == c[:-k]), (B, k)
        assert not np.any(MB.content_of(B, 1) == c)                  # the rotated set differs in every brick


@pytest.mark.parametrize("dims,B,midrange", SETS, ids=_id)
def test_builder_conditions(dims, B, midrange):
    """Distinct contents, constants where is_constant says, no brick equal to a neighbour at any stride, and a constant
    and a non-constant brick within SEAM_WINDOW bricks on each side of every seam of this B."""
    MB.check_builder(dims, B, midrange)


def test_seams_are_the_ones_the_issue_names():
    assert MB.seams(31) == []
    assert MB.seams(32) == [16]
    assert MB.seams(33) == [16, 32]
    assert MB.seams(63) == [21, 31, 32, 42]
    assert MB.seams(64) == [16, 21, 32, 42, 48]
    assert MB.seams(65) == [16, 21, 32, 43, 48, 64]
    assert MB.seams(67) == [16, 22, 32, 33, 44, 50, 64]
    assert MB.seams(65, midrange=True) == [32, 64]                  # a MidRangeTree build never splits
    for B in (1023, 1024, 1025, 2049, 3000):
        s = MB.seams(B)
        assert {B // 2, B // 3, 2 * B // 3, B // 4, 3 * B // 4} <= set(s)
        assert (1024 in s) == (B > 1024) and (2048 in s) == (B > 2048)
    # the part counts themselves: a part holds at least 16 bricks or the build does not split
    assert [MB.parts_of(B, 2) for B in (31, 32, 33)] == [1, 2, 2]
    assert [MB.parts_of(B, 3) for B in (47, 48, 49)] == [1, 3, 3]
    assert [MB.parts_of(B, 4) for B in (63, 64, 65)] == [1, 4, 4]
    assert MB.part_bounds(67, 4) == [0, 16, 33, 50, 67] and MB.part_bounds(65, 3) == [0, 21, 43, 65]


@pytest.mark.parametrize("dims", [MB.FUSED, MB.UNFUSED, MB.GENERAL, MB.TINY], ids=_id)
def test_cut_pattern_hits_every_decode_class(dims):
    """The per-brick cuts of the decode_lod tests reach every class the plan has for the shape (one kernel each for these
    shapes: the lane kernel, or the general one), with scalars from above the index level and without, and skip some."""
    want = MB.decode_classes(dims)
    assert ("skip",) in want and len(want) >= 2
    for B in (33, 65, 1025):
        cuts = MB.cut_pattern(dims, B)
        got = {MB.decode_class(dims, int(c)) for c in cuts}
        assert got == want, (dims, B, want - got)
        assert -1 in cuts and MB.max_depth(dims) in cuts and 0 in cuts
    # at 1025 bricks every cut's bricks are a hundred or so, none next to another
    cuts = MB.cut_pattern(dims, 1025)
    for c in set(cuts.tolist()):
        at = np.flatnonzero(cuts == c)
        assert at.size >= 100 and np.all(np.diff(at) > 1), (dims, c)
    # and every content meets every cut
    seen = {(int(w), int(c)) for w, c in zip(MB.content_of(1025), cuts)}
    assert len(seen) == MB.PERIOD * len(MB.cut_pool(dims))


def test_shape_facts():
    assert [MB.depth(d) for d in (MB.FUSED, MB.UNFUSED, MB.GENERAL, MB.TINY)] == [12, 9, 7, 3]
    assert [MB.index_depth(d) for d in (MB.FUSED, MB.UNFUSED, MB.GENERAL, MB.TINY)] == [6, 3, 1, 0]
    assert MB.is_general(MB.GENERAL) and not MB.is_general(MB.FUSED)
    assert MB.uniform_cuts(MB.FUSED) == [0, 5, 6, 12, 19]


# ---- the oracle ----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def expects(oracle):
    return {s: MB.Expect(oracle, *s) for s in SETTINGS}


@pytest.mark.parametrize("setting", SETTINGS, ids=_id)
def test_oracle_results_tell_the_bricks_apart(expects, setting):
    """Two different contents never give the same (stream, distance map, full decode): a result that lands on another
    brick is a mismatch whatever is compared.  Constants take the closed form (one token), the others do not."""
    e = expects[setting]
    key = [(e.tree[i].tobytes(), e.dmap[i].tobytes(), int(e.num_active[i])) for i in range(MB.PERIOD)]
    full = e.cut(-1)
    for i in range(MB.PERIOD):
        for j in range(i):
            assert key[i] != key[j] or not np.array_equal(full[i], full[j]), (i, j)
            assert not np.array_equal(full[i], full[j]), (i, j)
        if MB.is_constant(i):
            assert np.all(full[i] == MB.CONSTANTS[i // MB.CONST_EVERY])
    if setting[1] == 6:            # the tolerance-6, five-epoch set is there for prunes and reverts
        lossy = sum(int(np.any(full[i] != MB.contents(setting[0])[1][i].reshape(-1))) for i in range(MB.PERIOD))
        assert lossy >= 10 and any(t.numReverts > 0 for t in e.trees)


@pytest.mark.parametrize("setting", SETTINGS, ids=_id)
def test_oracle_matches_the_reference_codec_on_the_contents(oracle, setting, tmp_path):
    if not oracle.ref_available():
        pytest.skip("oracle/_ref/libvkref.so is not built: no reference sources at %s" % oracle.ref_dir())
    from test_ref_parity import compare
    dims, tol, ep, midrange = setting
    names, vols = MB.contents(dims)
    for n, v in zip(names, vols):
        compare(oracle, v, tol, ep, midrange, tmp_path, (dims, n, tol, ep, midrange))


# ---- the compact layout ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1025, 2049])
def test_compact_layout_offsets(expects, B):
    """The layout the compact streams have (vrhip.h: back to back, 16-byte aligned, one spare word each), per brick and
    summed two ways: one brick after the other, and in k_brick_offsets' rounds of 1024 with a carry.  The API hands out
    no offsets -- tree(b) copies from them -- so the GPU module checks them through every brick's bytes."""
    e = expects[(MB.FUSED, 1, 2, False)]
    n = e.num_active[MB.content_of(B)]
    import math
    for k in (1, 15, 16, 17, 4095, 4096):
        assert MB.compact_bytes(k) == math.ceil((math.ceil(k / 16) + 1) * 4 / 16) * 16
    assert [MB.compact_bytes(k) for k in (1, 16, 17, 48, 49, 112, 113)] == [16, 16, 16, 16, 32, 32, 48]
    off = MB.compact_offsets(n)
    assert off == MB.compact_offsets_in_rounds(n)
    assert len(off) == B + 1 and off[0] == 0 and all(o % 16 == 0 for o in off)
    for b in range(B):
        assert off[b + 1] - off[b] >= (int(n[b]) + 3) // 4 + 4              # the stream and its spare word fit
        assert off[b + 1] - off[b] == MB.compact_bytes(n[b])
    # what a dropped carry would do: brick 1024 back at offset 0, on top of brick 0
    assert off[1024] > 0 and off[1024] == sum(MB.compact_bytes(k) for k in n[:1024])
    # the periodic contents make the offsets periodic too: a whole period takes the same bytes wherever it starts
    per = sum(MB.compact_bytes(k) for k in e.num_active)
    assert off[MB.PERIOD * 27] == 27 * per


# ---- the limit -------------------------------------------------------------------------------------------------------
def test_brick_count_limit_is_checked_before_the_device():
    import __graft_entry__ as g
    g.build()
    from volumerenderer_amd import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "vrhip.h")).read()
    limit = int(re.search(r"#define\s+VR_MAX_BRICKS\s+(\d+)", hdr).group(1))
    assert limit == 65535
    n = C.c_int32(-1)
    assert L.vr_device_count(C.byref(n)) == 0
    h = C.c_void_p()
    for dims in ((2, 2, 2), (16, 16, 16), (12, 6, 5)):
        d = (C.c_int64 * 3)(*dims)
        for nb in (limit + 1, 1 << 20, 2 ** 31 - 1):
            assert L.vr_brickset_create(C.byref(h), nb, d, 1, 2, 0) == -7 and not h, (dims, nb)    # VR_ERR_UNSUPPORTED
        assert L.vr_brickset_create(C.byref(h), 0, d, 1, 2, 0) == -1                                # (as before)
        if n.value == 0:           # the limit itself passes the argument checks and reaches the device check
            assert L.vr_brickset_create(C.byref(h), limit, d, 1, 2, 0) == -2
    # vr_assemble_bricks / vr_disassemble_bricks: the same bound on their own count, after the other argument checks
    nb = limit + 1
    ijk = np.zeros(nb * 3, np.int64)
    buf = (C.c_uint8 * 16)()
    bd, grid = (C.c_int64 * 3)(16, 1, 1), (C.c_int64 * 3)(1, 1, 1)
    for fn in (L.vr_assemble_bricks, L.vr_disassemble_bricks):
        assert fn(buf, nb, bd, ijk.ctypes.data_as(C.POINTER(C.c_int64)), grid, buf, None) == -7
        assert fn(buf, nb, (C.c_int64 * 3)(8, 1, 1), ijk.ctypes.data_as(C.POINTER(C.c_int64)), grid, buf, None) == -7
        assert fn(None, nb, bd, ijk.ctypes.data_as(C.POINTER(C.c_int64)), grid, buf, None) == -1
        if n.value == 0:
            assert fn(buf, 1, bd, ijk.ctypes.data_as(C.POINTER(C.c_int64)), grid, buf, None) == -2
