"""GPU tests of the iso-surface mesh (vr_isomesh_count / vr_isomesh_emit, render.isosurface_mesh): counts, positions,
gradients and indices against the NumPy restatement of the header's rule (tests/refmesh.py), bit for bit; slabs of
several ranks against the single call; the guards of every output; determinism; the C++ example's hashes."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))

import refmesh  # noqa: E402

pytestmark = pytest.mark.gpu
I64x3 = C.c_int64 * 3


@pytest.fixture(scope="module")
def vr():
    import __graft_entry__ as g
    g.build()
    import torch
    assert torch.cuda.is_available()
    import volumerenderer_amd as vr
    return vr


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def u32(t):
    """The uint32 indices an int32 tensor carries, as int64."""
    import torch
    return t.to(torch.int64) & 0xFFFFFFFF


def assert_equals_ref(m, ref, what):
    import torch
    assert (m.num_vertices, m.num_triangles) == ref.counts, (what, m.num_vertices, m.num_triangles, ref.counts)
    assert torch.equal(m.positions.cpu(), torch.from_numpy(ref.positions)), what
    assert torch.equal(u32(m.triangles).cpu(), torch.from_numpy(ref.triangles.astype(np.int64))), what
    if ref.gradients is not None:
        assert torch.equal(m.gradients.cpu(), torch.from_numpy(ref.gradients)), what
    else:
        assert m.gradients is None


def soup(m):
    """(T, 9) or (T, 18): the corner positions (and gradients) of every triangle, in order."""
    import torch
    rows = m.positions if m.gradients is None else torch.cat([m.positions, m.gradients], 1)
    return rows[u32(m.triangles).reshape(-1)].reshape(m.num_triangles, -1)


def sorted_rows(a):
    a = a.cpu().numpy()
    return a[np.lexsort(a.T[::-1])] if len(a) else a


def scene_volume():
    """The 28 x 20 x 24 random volume of the slice tests, [Z][Y][X]."""
    vol = np.random.default_rng(17).integers(0, 256, (24, 20, 28), dtype=np.uint8)
    vol[8:16] //= 8
    return vol


def random_volume(dims, seed):
    return np.random.default_rng(seed).integers(0, 256, dims[::-1], dtype=np.uint8)


SHAPES = {
    "1x1x1": lambda: np.full((1, 1, 1), 255, np.uint8),
    "2x2x2": lambda: random_volume((2, 2, 2), 1),
    "7x1x3": lambda: random_volume((7, 1, 3), 2),
    "1x1x300": lambda: random_volume((1, 1, 300), 3),
    "63x3x2": lambda: random_volume((63, 3, 2), 4),            # a run is 64 points: rows that end before, at and after one
    "64x3x2": lambda: random_volume((64, 3, 2), 5),
    "65x3x2": lambda: random_volume((65, 3, 2), 6),
    "129x3x2": lambda: random_volume((129, 3, 2), 7),
    "scene": scene_volume,
    "ball": lambda: refmesh.ball(12),
    "noise": lambda: random_volume((5, 6, 7), 8),              # the densest: nearly every edge crosses
}


@pytest.mark.parametrize("cap", [False, True])
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_mesh_equals_the_rule(vr, shape, cap):
    vol = SHAPES[shape]()
    dims = vol.shape[::-1]
    grads = shape != "scene" or cap                            # (the scene once with and once without gradients)
    m = vr.isosurface_mesh(dev(vol).reshape(-1), dims, 0.5, cap=cap, gradients=grads)
    ref = refmesh.mesh(vol, 0.5, cap, gradients=grads)
    assert_equals_ref(m, ref, (shape, cap))
    if shape in ("1x1x1", "ball"):
        assert ref.counts == {"1x1x1": (14, 24) if cap else (0, 0), "ball": (302, 600)}[shape]
    if cap:
        assert refmesh.is_closed(u32(m.triangles).cpu().numpy())


@pytest.mark.parametrize("cap", [False, True])
def test_iso_settings(vr, cap):
    """iso at 0, at k / 255 for a k the volume holds (t == 0: v(p) == level), between values, at 1.0 and above 1."""
    for shape in ("noise", "7x1x3"):
        vol = SHAPES[shape]()
        vol.reshape(-1)[::5] = 255                             # 1.0 is a value the volume holds
        dims = vol.shape[::-1]
        F = np.float32
        exact = [int(k) for k in np.unique(vol) if 0 < k < 255 and F(k / 255.0) * F(255.0) == F(k)]
        held = exact[len(exact) // 2]                          # level == a value the volume holds, exactly
        d = dev(vol).reshape(-1)
        for iso in (0.0, held / 255.0, 100.5 / 255.0, 1.0, 1.5, -0.25):
            m = vr.isosurface_mesh(d, dims, iso, cap=cap, gradients=True)
            assert_equals_ref(m, refmesh.mesh(vol, iso, cap, gradients=True), (shape, cap, iso))
            if iso in (0.0, 1.5) and cap:
                assert (m.num_vertices, m.num_triangles) == (0, 0)
            if iso == 1.0 and (cap or shape == "noise"):       # (7 x 1 x 3 has no cell without the cap)
                assert m.num_triangles > 0


def test_own_boxes_inside_a_held_part(vr):
    """A box in the middle of the volume, the caller holding no more than the rule asks for; boxes empty on an axis."""
    vol = random_volume((9, 8, 10), 11)
    for cap, lo, hi, grads in ((False, (2, 1, 3), (6, 7, 8), False), (False, (2, 1, 3), (6, 7, 8), True),
                               (True, (-1, 2, 4), (9, 5, 10), True), (True, (3, -1, -1), (4, 8, 2), False),
                               (True, (3, 4, -1), (3, 6, 2), False), (False, (0, 0, 9), (8, 7, 9), True)):
        g = 1 if grads else 0
        a = [max(lo[k] - g, 0) for k in range(3)]
        b = [min(hi[k] + g, vol.shape[2 - k] - 1) + 1 for k in range(3)]
        part = vol[a[2]:b[2], a[1]:b[1], a[0]:b[0]]
        m = vr.isosurface_mesh(dev(part).reshape(-1), part.shape[::-1], 0.5, cap=cap, gradients=grads, global_dims=(9, 8, 10),
                               vol_origin=a, own_lo=lo, own_hi=hi)
        assert_equals_ref(m, refmesh.mesh(vol, 0.5, cap, lo, hi, grads), (cap, lo, hi, grads))


# ---- slabs ---------------------------------------------------------------------------------------------------------------
SLAB_DIMS = (9, 10, 11)


@pytest.fixture(scope="module")
def slab_whole(vr):
    """The single call's mesh per (cap, gradients), checked against the rule once."""
    vol = random_volume(SLAB_DIMS, 12)
    vol[2:4] //= 4                                             # two dim layers: no crossing edge inside them
    out = {}
    for cap in (False, True):
        for grads in (False, True):
            m = vr.isosurface_mesh(dev(vol).reshape(-1), SLAB_DIMS, 0.45, cap=cap, gradients=grads)
            out[cap, grads] = m
        assert_equals_ref(out[cap, True], refmesh.mesh(vol, 0.45, cap, gradients=True), cap)
    return vol, out


@pytest.mark.parametrize("world", [2, 3, 5, 8])
@pytest.mark.parametrize("axis", [0, 1, 2])
def test_slab_meshes_concatenate_to_the_single_call(vr, slab_whole, axis, world):
    import torch
    from volumerenderer_amd import distributed as D
    vol, whole = slab_whole
    for (cap, grads), one in whole.items():
        parts = []
        for rank in range(world):
            org, lo, hi, local, (a0, a1) = D.slab_cells(SLAB_DIMS, axis, rank, world, cap, grads)
            sl = [slice(None)] * 3
            sl[2 - axis] = slice(a0, a1)
            held = np.ascontiguousarray(vol[tuple(sl)])        # the rank's voxels and no others
            assert held.shape[::-1] == local
            parts.append(vr.isosurface_mesh(dev(held).reshape(-1), local, 0.45, cap=cap, gradients=grads, global_dims=SLAB_DIMS,
                                            vol_origin=org, own_lo=lo, own_hi=hi))
        assert sum(p.num_triangles for p in parts) == one.num_triangles
        both = vr.IsoMesh.concat(parts)
        assert both.num_vertices >= one.num_vertices
        if axis == 2:                                          # cells x fastest, z slowest: the ranks follow one another
            assert torch.equal(soup(both), soup(one)), (cap, grads)
        else:
            assert np.array_equal(sorted_rows(soup(both)), sorted_rows(soup(one))), (cap, grads)
        # seam vertices are stored by both neighbours, bit for bit: the slabs add no vertex the single call lacks
        rows = lambda m: {r.tobytes() for r in (m.positions if not grads else torch.cat([m.positions, m.gradients], 1)).cpu().numpy()}
        assert rows(both) == rows(one)
        assert both.num_vertices > one.num_vertices            # (some cut plane of every set of slabs holds a crossing edge)


def test_scan_levels_beyond_one_group_and_one_chunk(vr):
    """More than 1024 runs (a second scan level) and more than 1024 x 1024 runs (its carry loop): the whole call equals
    its z-slabs, each of which stays below the size in question, triangle for triangle and in order."""
    import torch
    from volumerenderer_amd import distributed as D
    g = torch.Generator(device="cuda").manual_seed(5)
    for dims, world in (((64, 40, 40), 4), ((512, 512, 258), 2)):
        X, Y, Z = dims
        vol = torch.zeros((Z, Y, X), dtype=torch.uint8, device="cuda")
        for z0, z1 in ((1, 3), (Z // 2 - 1, Z // 2 + 2), (Z - 2, Z)):    # noise where the runs begin, at the cut, and at the end
            vol[z0:z1, :24, X - 40:] = torch.randint(0, 256, (z1 - z0, 24, 40), dtype=torch.uint8, device="cuda", generator=g)
        one = vr.isosurface_mesh(vol.reshape(-1), dims, 0.5, gradients=True)
        points = X * Y * Z
        assert points // 64 > (1024 if world == 4 else 1024 * 1024) and one.num_triangles > 10000
        parts = []
        for rank in range(world):
            org, lo, hi, local, (a0, a1) = D.slab_cells(dims, 2, rank, world, False, True)
            assert local[0] * local[1] * (hi[2] - lo[2] + 1) // 64 < (1024 if world == 4 else 1024 * 1024)
            parts.append(vr.isosurface_mesh(vol[a0:a1].reshape(-1), local, 0.5, gradients=True, global_dims=dims, vol_origin=org,
                                            own_lo=lo, own_hi=hi))
        assert torch.equal(soup(vr.IsoMesh.concat(parts)), soup(one))
        # and the lowest slab of the first volume against the rule itself
        if world == 4:
            org, lo, hi, local, (a0, a1) = D.slab_cells(dims, 2, 0, world, False, True)
            assert_equals_ref(parts[0], refmesh.mesh(vol.cpu().numpy()[:a1 + 1], 0.5, False, lo, hi, True), "lowest slab")


def test_point_indices_beyond_32_bits(vr):
    """A point box of more than 2^32 points -- more than one launch can have threads, and point indices that need 64
    bits: the whole call finds the noise at the far end of the volume exactly as a call that owns only its corner."""
    import torch
    dims = (2048, 2048, 1025)
    assert dims[0] * dims[1] * dims[2] > 1 << 32
    vol = torch.zeros(dims[::-1], dtype=torch.uint8, device="cuda")
    g = torch.Generator(device="cuda").manual_seed(9)
    vol[1020:1024, 2000:2040, 2000:2040] = torch.randint(0, 256, (4, 40, 40), dtype=torch.uint8, device="cuda", generator=g)
    vol[0:2, 0:8, 0:70] = torch.randint(0, 256, (2, 8, 70), dtype=torch.uint8, device="cuda", generator=g)
    one = vr.isosurface_mesh(vol.reshape(-1), dims, 0.5, gradients=True)
    near = vr.isosurface_mesh(vol.reshape(-1), dims, 0.5, gradients=True, own_lo=(0, 0, 0), own_hi=(80, 16, 8))
    far = vr.isosurface_mesh(vol.reshape(-1), dims, 0.5, gradients=True, own_lo=(1990, 1990, 1015), own_hi=(2047, 2047, 1024))
    assert near.num_triangles > 1000 and far.num_triangles > 10000
    assert one.num_vertices == near.num_vertices + far.num_vertices
    assert torch.equal(soup(one), torch.cat([soup(near), soup(far)]))
    del vol, one
    torch.cuda.empty_cache()


# ---- guards ----------------------------------------------------------------------------------------------------------------
class Raw:
    """count + emit through the C ABI with buffers of the test's own."""

    def __init__(self, vr, vol_t, dims, iso=0.5, cap=True):
        import torch
        from volumerenderer_amd import _lib, render
        self.L, self.vol, self.dims = _lib.lib(), vol_t, I64x3(*dims)
        self.desc = render.isomesh_desc(dims, iso, cap, True)
        n = C.c_int64()
        assert self.L.vr_isomesh_workspace_bytes(self.dims, C.byref(self.desc), C.byref(n)) == 0
        self.ws = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        self.stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)

    def count(self):
        c = (C.c_uint64 * 2)()
        rc = self.L.vr_isomesh_count(C.c_void_p(self.vol.data_ptr()), self.dims, C.byref(self.desc), C.c_void_p(self.ws.data_ptr()),
                                     c, self.stream)
        assert rc == 0
        return int(c[0]), int(c[1])

    def emit(self, nv, nt, pos, grad, idx):
        p = lambda t: None if t is None else C.c_void_p(t.data_ptr())
        return self.L.vr_isomesh_emit(C.c_void_p(self.vol.data_ptr()), self.dims, C.byref(self.desc), C.c_void_p(self.ws.data_ptr()),
                                      nv, nt, p(pos), p(grad), p(idx), self.stream)


def test_outputs_at_four_byte_offsets_inside_poisoned_allocations(vr):
    import torch
    vol = SHAPES["noise"]()
    ref = refmesh.mesh(vol, 0.5, True, gradients=True)
    V, T = ref.counts
    r = Raw(vr, dev(vol).reshape(-1), (5, 6, 7))
    assert r.count() == (V, T)
    for off in (1, 2, 3):                                      # in 4-byte words
        bufs = [torch.full((3 * n + 8,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for n in (V, V, T)]
        views = [b[off:off + 3 * n] for b, n in zip(bufs, (V, V, T))]
        assert all(v.data_ptr() % 16 == 4 * off for v in views)
        assert r.emit(V, T, views[0], views[1], views[2]) == 0
        torch.cuda.synchronize()
        for b, n in zip(bufs, (V, V, T)):
            assert (b[:off] == 0x5A5A5A5A).all() and (b[off + 3 * n:] == 0x5A5A5A5A).all()
        assert torch.equal(views[0].view(torch.float32).reshape(V, 3).cpu(), torch.from_numpy(ref.positions))
        assert torch.equal(views[1].view(torch.float32).reshape(V, 3).cpu(), torch.from_numpy(ref.gradients))
        assert torch.equal(u32(views[2]).reshape(T, 3).cpu(), torch.from_numpy(ref.triangles.astype(np.int64)))


def test_counts_passed_short_stop_every_store(vr):
    """num_vertices / num_triangles one short (and a lot short): nothing is written beyond them, and what is written is
    the mesh's beginning."""
    import torch
    vol = SHAPES["noise"]()
    ref = refmesh.mesh(vol, 0.5, True, gradients=True)
    V, T = ref.counts
    r = Raw(vr, dev(vol).reshape(-1), (5, 6, 7))
    assert r.count() == (V, T)
    for nv, nt in ((V - 1, T - 1), (V, T - 1), (V - 1, T), (7, 5), (0, T), (V, 0)):
        pos, grad, idx = [torch.full((3 * n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda") for n in (V, V, T)]
        assert r.emit(nv, nt, pos, grad, idx) == 0
        torch.cuda.synchronize()
        assert (pos[3 * nv:] == 0x5A5A5A5A).all() and (grad[3 * nv:] == 0x5A5A5A5A).all() and (idx[3 * nt:] == 0x5A5A5A5A).all()
        assert torch.equal(pos[:3 * nv].view(torch.float32).cpu(), torch.from_numpy(ref.positions.reshape(-1)[:3 * nv]))
        assert torch.equal(grad[:3 * nv].view(torch.float32).cpu(), torch.from_numpy(ref.gradients.reshape(-1)[:3 * nv]))
        assert torch.equal(u32(idx[:3 * nt]).cpu(), torch.from_numpy(ref.triangles.astype(np.int64).reshape(-1)[:3 * nt]))
    # zero counts launch nothing: null outputs are fine
    assert r.emit(0, 0, None, None, None) == 0
    # without gradients the gradient buffer is not an argument at all
    pos, idx = torch.empty(3 * V, dtype=torch.float32, device="cuda"), torch.empty(3 * T, dtype=torch.int32, device="cuda")
    assert r.emit(V, T, pos, None, idx) == 0
    assert torch.equal(pos.cpu(), torch.from_numpy(ref.positions.reshape(-1)))


def test_volume_at_odd_byte_offsets(vr):
    import torch
    vol = scene_volume()
    dims = vol.shape[::-1]
    flat = torch.from_numpy(vol.reshape(-1))
    base = torch.zeros(flat.numel() + 64, dtype=torch.uint8, device="cuda")
    first = vr.isosurface_mesh(dev(vol).reshape(-1), dims, 0.3, gradients=True)
    for off in (1, 7):
        v = base[off:off + flat.numel()]
        v.copy_(flat)
        assert v.data_ptr() % 16 == off
        m = vr.isosurface_mesh(v, dims, 0.3, gradients=True)
        assert torch.equal(m.positions, first.positions) and torch.equal(m.gradients, first.gradients)
        assert torch.equal(m.triangles, first.triangles)


def test_two_calls_write_the_same_bytes(vr):
    import torch
    vol = dev(scene_volume()).reshape(-1)
    a = vr.isosurface_mesh(vol, (28, 20, 24), 0.5, cap=True, gradients=True)
    b = vr.isosurface_mesh(vol, (28, 20, 24), 0.5, cap=True, gradients=True)
    for x, y in ((a.positions, b.positions), (a.gradients, b.gradients)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert torch.equal(a.triangles, b.triangles) and a.num_triangles > 0


def test_count_only_switch_is_for_measurements_and_leaves_no_trace(vr):
    """vr_debug_set("mesh_count_only", 1): vr_isomesh_count stops after its per-point pass and reports zero counts;
    switched off again, the same workspace gives the mesh as ever."""
    vol = SHAPES["noise"]()
    ref = refmesh.mesh(vol, 0.5, True)
    r = Raw(vr, dev(vol).reshape(-1), (5, 6, 7))
    try:
        assert r.L.vr_debug_set(b"mesh_count_only", 1) == 0
        assert r.count() == (0, 0)
    finally:
        assert r.L.vr_debug_set(b"mesh_count_only", 0) == 0
    assert r.count() == ref.counts
    assert_equals_ref(vr.isosurface_mesh(dev(vol).reshape(-1), (5, 6, 7), 0.5, cap=True), ref, "after the switch")


def test_wrapper_helpers_on_the_device(vr, tmp_path):
    import torch
    vol = refmesh.ball(12)
    m = vr.isosurface_mesh(dev(vol).reshape(-1), (12, 12, 12), 0.5, gradients=True)
    n = m.normals()
    assert torch.allclose(torch.linalg.vector_norm(n, dim=1), torch.ones(m.num_vertices, device="cuda"), atol=1e-6)
    centre = torch.tensor([5.5, 5.5, 5.5], device="cuda")
    assert ((m.positions - centre) * n).sum(1).min() > 0       # -g points away from the ball's centre
    w = m.world_positions((12, 12, 12))
    assert w.abs().max() < 0.5
    vr.write_ply(str(tmp_path / "ball.ply"), m)
    pos, nrm, faces = vr.read_ply(str(tmp_path / "ball.ply"))
    assert np.array_equal(pos, m.positions.cpu().numpy()) and np.array_equal(faces.astype(np.int64), u32(m.triangles).cpu().numpy())
    assert refmesh.signed_volume(pos, faces) > 0


# ---- the example -----------------------------------------------------------------------------------------------------------
def fnv1a64(data):
    h = 14695981039346656037
    for b in bytes(data):
        h = ((h ^ b) * 1099511628211) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


def test_cpp_example_prints_the_hashes_of_the_python_mesh(vr, tmp_path):
    from test_isomesh_cpu import compile_example, example_ball
    exe = compile_example(tmp_path)
    ply = tmp_path / "ball.ply"
    r = subprocess.run([exe, str(ply)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = [ln.split() for ln in r.stdout.strip().splitlines()]
    m = vr.isosurface_mesh(dev(example_ball()).reshape(-1), (24, 24, 24), 0.5, cap=True, gradients=True)
    assert lines[0] == ["vertices", str(m.num_vertices)] and lines[1] == ["triangles", str(m.num_triangles)] and m.num_triangles > 0
    for ln, (name, t) in zip(lines[2:5], (("positions", m.positions), ("gradients", m.gradients), ("indices", m.triangles))):
        assert ln == [name, "fnv1a64", fnv1a64(t.cpu().numpy().tobytes())], name
    assert lines[5] == ["OK"]
    pos, nrm, faces = vr.read_ply(str(ply))
    assert np.array_equal(pos, m.positions.cpu().numpy()) and nrm is None
    assert np.array_equal(faces.astype(np.int64), u32(m.triangles).cpu().numpy())
