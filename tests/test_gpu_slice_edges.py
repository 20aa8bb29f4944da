"""k_reslice (vr_reslice, vr_reslice_partial) on the case table of tests/slicecases.py: planes, boxes, voxels and tiles at
their edges.  Every case, op and filter is held bit for bit to the float32 restatement (refslice.py) AND directly to the
independent float64 reference (slicecases.ref64, on the decided pixels), to the answers its family knows, to its own
reversed stack and to itself with the axes rotated; the exact slabs to the single-GPU slice; then the buffers (the volume
at odd bytes, the frame at every float offset of an allocation) and the wave's tile at the frame sizes around it."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import refslice as RS  # noqa: E402
import slicecases as SC  # noqa: E402
from test_gpu_transfer_function import smooth_table  # noqa: E402
from test_reslice_cpu import SCENE_DIMS, oblique_plane, scene_volume  # noqa: E402

pytestmark = pytest.mark.gpu
CASES = SC.cases()
BG = (0.2, 0.4, 0.6)
POISON = -7.0


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def L(vr):
    from volumerenderer_amd import _lib
    return _lib.lib()


def _dev(vol, offset=0):
    """The volume on the device, flat, `offset` bytes into its allocation."""
    import torch
    flat = torch.from_numpy(np.array(vol)).reshape(-1)              # a copy: the table's volumes are read-only
    buf = torch.zeros(flat.numel() + offset, dtype=torch.uint8, device="cuda")
    buf[offset:] = flat
    return buf[offset:]


class Slicer:
    """run(vol, geo, flt, op) of slicecases' checks on the kernel: the partial as a NumPy array.  Volumes stay on the
    device between calls."""

    def __init__(self, vr):
        self.vr, self.vols = vr, {}

    def dev(self, vol):
        key = (hash(vol.tobytes()), vol.shape)
        if key not in self.vols:
            self.vols[key] = _dev(vol)
        return self.vols[key]

    def partial(self, vol, geo, flt, op, proj=None):
        Z, Y, X = vol.shape
        proj = proj or self.vr.Projection(SC.OP_NAMES[op])
        return self.vr.reslice_partial(self.dev(vol), (X, Y, Z), SC.plane_of(geo, flt), proj)

    def __call__(self, vol, geo, flt, op):
        return self.partial(vol, geo, flt, op).cpu().numpy()


@pytest.fixture(scope="module")
def run(vr):
    return Slicer(vr)


@pytest.fixture(scope="module")
def lut(vr):
    return vr.transfer_function_table(smooth_table(np.random.default_rng(5)))


# ---- every case, op and filter -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(CASES)), ids=[c["name"].replace(" ", "-") for c in CASES])
def test_slice_case(vr, run, lut, k):
    import torch
    from volumerenderer_amd import distributed as D
    c = CASES[k]
    vol, geo = c["vol"], c["geo"]
    dims = vol.shape[::-1]
    line = []
    for flt in (SC.NEAREST, SC.LINEAR):
        for op in SC.OPS:
            tag = (c["name"], SC.FILTER_NAMES[flt], SC.OP_NAMES[op])
            pl = SC.plane_of(geo, flt)
            grey = vr.Projection(SC.OP_NAMES[op], background=BG)
            dpart = run.partial(vol, geo, flt, op, grey)
            part = dpart.cpu().numpy()
            # 1. bit for bit against the float32 restatement
            want = SC.ref32(vol, pl, op)
            assert np.array_equal(part, want), tag
            # 2. against the independent reference, and what the family knows
            err, masked = SC.compare(c, vol, geo, flt, op, part)
            SC.check_known(c, flt, op, part, run)
            line.append("%s/%s %.2g/%d" % (SC.FILTER_NAMES[flt][:3], SC.OP_NAMES[op], err, masked))
            # 3. the frame is the finish of the partial; n == 0 is (background, 0)
            empty = part[..., 1] == 0
            for proj in (grey, vr.Projection(SC.OP_NAMES[op], (0.1, 0.9), BG, lut)):
                frame = vr.reslice(run.dev(vol), dims, pl, proj)
                assert torch.equal(vr.composite_finish_proj(dpart, proj), frame), tag
                table = None if proj.lut is None else lut
                with np.errstate(all="ignore"):
                    fwant = RS.finish(want, op, proj.window, BG, table)
                got = frame.cpu().numpy()
                assert np.array_equal(got, fwant), tag + (table is not None,)
                assert np.array_equal(got[empty], np.broadcast_to(np.float32(BG + (0.0,)), got[empty].shape)), tag
            # 4. the stack walked backwards   5. the axes rotated
            if c["exact"] and c["family"] != "deep":
                SC.check_reversed(c, flt, op, part, run)
            if not c["slabs"]:
                SC.check_rotated(c, flt, op, part, run)
            # 6. exact slabs: every boundary sample is owned exactly once
            if c["slabs"]:
                parts = [run.partial(sub, g, flt, op) for g, sub in c["slabs"]]
                for (g, sub), p in zip(c["slabs"], parts):
                    assert np.array_equal(p.cpu().numpy(), SC.ref32(sub, SC.plane_of(g, flt), op)), tag
                stack = torch.stack([p.reshape(-1, 4) for p in parts], 0)
                assert torch.equal(stack[..., 1].sum(0), dpart.reshape(-1, 4)[:, 1]), tag
                if op != SC.MEAN or geo["layers"] == 1:
                    frame = vr.reslice(run.dev(vol), dims, pl, grey)
                    got = D._gpu_combine_proj(stack.contiguous(), grey).reshape(frame.shape)         # vr_composite_slabs_proj
                    assert torch.equal(got, frame), tag
    print("SLICE-EDGE %-8s %-26s %s" % (c["family"], c["name"], "  ".join(line)))


# ---- buffers -------------------------------------------------------------------------------------------------------------
def _buffer_scenes():
    lattice = CASES[SC.family("lattice")[2]]
    oblique = [CASES[k] for k in SC.family("general") if CASES[k]["name"] == "plane 2 28x20x24 x7"][0]
    return [lattice, oblique]


@pytest.mark.parametrize("which", [0, 1], ids=["lattice", "oblique"])
def test_volume_at_odd_bytes_and_frame_at_every_float_offset(vr, run, lut, which):
    """volume_dev at byte 1 and 7 of its allocation; rgba_dev / partial_dev at float 1, 2 and 3 of a poisoned one (the
    header's rule: any 4-byte-aligned address).  The frame is the aligned one bit for bit and the guards keep their poison."""
    import torch
    c = _buffer_scenes()[which]
    vol, geo = c["vol"], c["geo"]
    dims = vol.shape[::-1]
    H, W = geo["height"], geo["width"]
    N = H * W * 4
    for flt in (SC.NEAREST, SC.LINEAR):
        pl = SC.plane_of(geo, flt)
        for op, proj in ((SC.MAX, vr.Projection("max", background=BG)), (SC.MEAN, vr.Projection("mean", (0.1, 0.9), BG, lut))):
            for fn in (vr.reslice_partial, vr.reslice):
                want = fn(run.dev(vol), dims, pl, proj)
                if fn is vr.reslice_partial:
                    assert np.array_equal(want.cpu().numpy(), SC.ref32(vol, pl, op))
                for off in (1, 7):
                    dvol = _dev(vol, off)
                    assert dvol.data_ptr() % 8 == off
                    assert torch.equal(fn(dvol, dims, pl, proj), want), (c["name"], flt, op, off)
                for off in (1, 2, 3):
                    big = torch.full((N + 8,), POISON, dtype=torch.float32, device="cuda")
                    out = big[off:off + N].view(H, W, 4)
                    assert out.data_ptr() % 16 == 4 * off
                    assert fn(run.dev(vol), dims, pl, proj, out=out) is out
                    assert torch.equal(out, want), (c["name"], flt, op, off)
                    assert (big[:off] == POISON).all() and (big[off + N:] == POISON).all(), (c["name"], flt, op, off)


# ---- tiles ---------------------------------------------------------------------------------------------------------------
TILE_SIZES = [(1, 1), (1, 130), (130, 1), (15, 5), (17, 3), (63, 2), (64, 1), (65, 4), (257, 3)]


def test_tile_edges_at_every_footprint(vr, L):
    """Widths and heights of 1 and widths around 16 and 64 under the 8 x 8, 16 x 4 and 64 x 1 footprints: the partial is
    refslice's bit for bit and the row after the frame is untouched."""
    import torch
    vol = scene_volume()
    dvol = _dev(vol)
    try:
        for W, H in TILE_SIZES:
            for flt in ("nearest", "linear"):
                plane = oblique_plane(2, W, H, 7, flt)
                want = torch.from_numpy(RS.partial(vol, plane, RS.MEAN))
                for tw in (8, 16, 64):
                    assert L.vr_debug_set(b"reslice_tile_w", tw) == 0
                    out = torch.full((H + 1, W, 4), POISON, dtype=torch.float32, device="cuda")
                    vr.reslice_partial(dvol, SCENE_DIMS, plane, vr.Projection("mean"), out=out[:H])
                    assert torch.equal(out[:H].cpu(), want), (W, H, flt, tw)
                    assert (out[H] == POISON).all(), (W, H, flt, tw)
    finally:
        assert L.vr_debug_set(b"reslice_tile_w", 16) == 0           # the library's default
