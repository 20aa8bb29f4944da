"""vr_lod_select (host only, no device): the per-brick cuts of a view-dependent decode, against a NumPy restatement of
the rule written in include/vrhip.h, plus the properties the rule is for."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import volumerenderer_amd as vr
from volumerenderer_amd import _lib
from volumerenderer_amd.render import default_camera, default_params, select_lod

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _norm(v):
    l = F(np.sqrt(F(F(v[0] * v[0]) + F(v[1] * v[1])) + F(v[2] * v[2])))
    return (v / l).astype(F) if l > 0 else np.zeros(3, F)


def _cross(a, b):
    return np.array([F(a[1] * b[2]) - F(a[2] * b[1]), F(a[2] * b[0]) - F(a[0] * b[2]), F(a[0] * b[1]) - F(a[1] * b[0])], F)


def rule(cam, P, brick_dims, ijk, grid, otd, mtd, tol):
    """include/vrhip.h, vr_lod_select, restated."""
    bd, g = np.array(brick_dims, np.float64), np.array(grid, np.float64)
    G = np.array([P.global_dims[k] if P.global_dims[k] > 0 else g[k] * bd[k] for k in range(3)], np.float64)
    vs = 1.0 / G
    step = max(abs(float(F(P.step_size[k]))) for k in range(3))
    grow = vs + ((0.01 + step) if P.mode == _lib.RENDER_ISOSURFACE else 0.0)
    f = _norm(np.array(cam.front[:], F))
    s = _norm(_cross(f, np.array(cam.up[:], F)))
    u = _cross(s, f)
    tanYf = F(math.tan(float(F(0.5) * F(F(cam.fov_deg) * F(0.01745329251994329576923690768489)))))
    tanY, tanX = float(tanYf), float(F(tanYf * F(P.width) / F(P.height)))
    f, s, u = f.astype(np.float64), s.astype(np.float64), u.astype(np.float64)
    pos = np.array(cam.pos[:], F).astype(np.float64)
    zn, zf = float(F(cam.z_near)), float(F(cam.z_far)) + (max(P.max_samples, 0) + 1.0) * step
    out = []
    for ijk_b in np.asarray(ijk, np.int64).reshape(-1, 3):
        lo = ijk_b * bd * vs - grow - 0.5
        hi = (ijk_b + 1) * bd * vs + grow - 0.5
        bmin, bmax = np.array(P.box_min[:], F).astype(np.float64), np.array(P.box_max[:], F).astype(np.float64)
        culled = bool(np.any(hi + 0.5 < bmin) or np.any(lo + 0.5 >= bmax))
        corners = np.array([[hi[0] if c & 1 else lo[0], hi[1] if c & 2 else lo[1], hi[2] if c & 4 else lo[2]] for c in range(8)])
        d = corners - pos
        z, x, y = d @ f, d @ s, d @ u
        t = 1e-6 * (1.0 + np.abs(z))
        culled = culled or bool(np.all(z < zn - t) or np.all(z > zf + t))
        if np.any(s != 0):
            culled = culled or bool(np.all(x > tanX * z + t) or np.all(-x > tanX * z + t)
                                    or np.all(y > tanY * z + t) or np.all(-y > tanY * z + t))
        if culled:
            out.append(-1)
            continue
        e = np.maximum(np.maximum(lo - pos, 0.0), pos - hi)
        sz = (P.height / 2.0 / tanY) * vs.max() / max(math.sqrt(float(e @ e)), zn)
        k = 0 if sz >= tol else int(min(otd, math.floor(3.0 * math.log2(tol / sz))))
        out.append(mtd if k == 0 else otd - k)
    return np.array(out, np.int32)


def _grid_ijk(grid):
    return np.array([(i, j, k) for k in range(grid[2]) for j in range(grid[1]) for i in range(grid[0])], np.int64)


def _cam(pos, front, up=(0.0, 1.0, 0.0), fov=50.0, near=0.1, far=100.0):
    c = default_camera()
    c.pos[:], c.front[:], c.up[:] = pos, front, up
    c.fov_deg, c.z_near, c.z_far = fov, near, far
    return c


@pytest.mark.parametrize("grid,bd", [((3, 2, 5), (64, 32, 16)), ((8, 8, 15), (256, 256, 128)), ((1, 4, 2), (96, 80, 40))])
@pytest.mark.parametrize("mode", [_lib.RENDER_COMPOSITE, _lib.RENDER_ISOSURFACE])
def test_select_matches_numpy_rule(grid, bd, mode):
    rng = np.random.default_rng(1234 + sum(grid) + mode)
    ijk = _grid_ijk(grid)
    otd = int(round(math.log2(bd[0] * bd[1] * bd[2])))
    mtd = otd + 7
    n_culled = n_kept = 0
    for trial in range(40):
        where = trial % 3      # inside the cube, outside it, far behind it
        if where == 0:
            pos = rng.uniform(-0.45, 0.45, 3)
        elif where == 1:
            pos = rng.uniform(-2.0, 2.0, 3)
        else:
            pos = np.array([0.0, 0.0, 1.5]) + rng.uniform(-0.3, 0.3, 3)
        front = rng.normal(size=3)
        if where == 2:
            front[2] = abs(front[2]) + 0.5       # facing away from the cube
        P = default_params(int(rng.integers(64, 1921)), int(rng.integers(64, 1081)), bd, mode)
        cam = _cam(tuple(pos), tuple(front / np.linalg.norm(front)), fov=float(rng.uniform(10, 90)),
                   near=float(rng.uniform(0.01, 0.3)), far=float(rng.uniform(0.5, 100)))
        tol = float(rng.choice([0.25, 1.0, 4.0, 16.0]))
        got = select_lod(cam, P, bd, ijk, grid, otd, mtd, tol)
        want = rule(cam, P, bd, ijk, grid, otd, mtd, tol)
        assert np.array_equal(got, want), (trial, np.nonzero(got != want))
        n_culled += int(np.sum(got < 0))
        n_kept += int(np.sum(got >= 0))
    assert n_culled > 0 and n_kept > 0        # both branches of the rule were exercised


def test_far_camera_culls_nothing():
    grid, bd = (8, 8, 15), (256, 256, 128)
    ijk = _grid_ijk(grid)
    cam = _cam((0.0, 0.0, -3.0), (0.0, 0.0, 1.0))
    cuts = select_lod(cam, default_params(1920, 1080, bd), bd, ijk, grid, 23, 30, 1.0)
    assert np.all(cuts >= 0)


def test_centre_camera_culls_only_bricks_behind_or_outside_the_fov():
    grid, bd = (8, 8, 8), (64, 64, 64)
    ijk = _grid_ijk(grid)
    cam = _cam((0.0, 0.0, 0.0), (0.0, 0.0, 1.0), fov=50.0)
    P = default_params(800, 600, bd)
    cuts = select_lod(cam, P, bd, ijk, grid, 18, 25, 1.0)
    tanY = math.tan(math.radians(25.0))
    tanX = tanY * 800 / 600
    vs = 1.0 / 512
    for b, (i, j, k) in enumerate(ijk):
        lo = np.array([i, j, k]) * 64 * vs - vs - 0.5
        hi = (np.array([i, j, k]) + 1) * 64 * vs + vs - 0.5
        behind = hi[2] < 0.1                               # wholly nearer than z_near
        # wholly beyond one side plane: the plane's value is positive at the box's minimising corner
        xs, zs = [lo[0], hi[0]], [lo[2], hi[2]]
        ys = [lo[1], hi[1]]
        side = (min(x - tanX * z for x in xs for z in zs) > 1e-6 or min(-x - tanX * z for x in xs for z in zs) > 1e-6
                or min(y - tanY * z for y in ys for z in zs) > 1e-6 or min(-y - tanY * z for y in ys for z in zs) > 1e-6)
        assert (cuts[b] == -1) == (behind or side), (b, (i, j, k), cuts[b])
    assert 0 < np.sum(cuts == -1) < len(cuts)
    assert np.all(cuts[ijk[:, 2] < 4] == -1)              # the half behind the camera


def test_cut_never_increases_with_distance():
    grid, bd = (16, 16, 16), (32, 32, 32)
    ijk = _grid_ijk(grid)
    rng = np.random.default_rng(7)
    for _ in range(10):
        pos = np.array([rng.uniform(-0.3, 0.3), rng.uniform(-0.3, 0.3), -2.5])
        d = np.array([0.0, 0.0, 1.0]) + rng.uniform(-0.1, 0.1, 3)
        d /= np.linalg.norm(d)
        cam = _cam(tuple(pos), tuple(d))
        cuts = select_lod(cam, default_params(1920, 1080, bd), bd, ijk, grid, 15, 22, 4.0)
        # the bricks a ray from the camera passes through, in order of distance
        seen, order = set(), []
        for t in np.linspace(2.0, 3.0, 4000):
            p = pos + t * d + 0.5
            if np.all((p >= 0) & (p < 1)):
                c = tuple((p * 512 // 32).astype(int))
                if c not in seen:
                    seen.add(c)
                    order.append(c[0] + 16 * (c[1] + 16 * c[2]))
        seq = [int(cuts[b]) for b in order]
        assert len(seq) >= 16 and all(c >= 0 for c in seq)
        assert all(a >= b for a, b in zip(seq, seq[1:])), seq
        assert seq[0] > seq[-1]                            # the rule does make far bricks coarser here


def test_tiny_tolerance_keeps_full_depth():
    grid, bd = (4, 4, 4), (64, 64, 64)
    ijk = _grid_ijk(grid)
    for pos, front in [((0.0, 0.0, -0.75), (0.0, 0.0, 1.0)), ((0.6, 0.2, -1.5), (-0.3, 0.0, 1.0))]:
        cam = _cam(pos, tuple(np.array(front) / np.linalg.norm(front)))
        cuts = select_lod(cam, default_params(1600, 1200, bd), bd, ijk, grid, 18, 25, 1e-6)
        assert np.all((cuts == -1) | (cuts == 25)) and np.any(cuts == 25)


def test_outside_the_box_is_culled():
    grid, bd = (4, 1, 1), (64, 64, 64)
    ijk = _grid_ijk(grid)
    cam = _cam((0.0, 0.0, -3.0), (0.0, 0.0, 1.0))
    P = default_params(800, 600, bd, _lib.RENDER_PARTIAL)
    P.box_min[:] = (0.5, 0.0, 0.0)
    P.box_max[:] = (0.75, 1.0, 1.0)
    cuts = select_lod(cam, P, bd, ijk, grid, 18, 25, 1.0)
    # brick 1 reaches [0.25 - 1/256, 0.5 + 1/256]: its grown box overlaps the slab; brick 3 starts at 0.75 - 1/256
    assert cuts[0] == -1 and cuts[1] >= 0 and cuts[2] >= 0 and cuts[3] >= 0
    P.box_min[:] = (0.0, 0.0, 0.0)
    P.box_max[:] = (0.2, 1.0, 1.0)
    cuts = select_lod(cam, P, bd, ijk, grid, 18, 25, 1.0)
    assert cuts[0] >= 0 and np.all(cuts[1:] == -1)


def test_invalid_arguments():
    grid, bd = (2, 2, 2), (16, 16, 16)
    ijk = _grid_ijk(grid)
    cam, P = default_camera(), default_params(64, 64, bd)
    for tol in (0.0, -1.0):
        with pytest.raises(vr.VrError):
            select_lod(cam, P, bd, ijk, grid, 12, 19, tol)


CPROG = r"""
#include <vrhip.h>
#include <stdio.h>
int main(void)
{
    vr_camera cam = {{0.0f, 0.0f, -0.75f}, {0.0f, 0.0f, 1.0f}, {0.0f, 1.0f, 0.0f}, 50.0f, 0.1f, 100.0f};
    vr_render_params P = {0};
    P.width = 1920; P.height = 1080;
    for (int k = 0; k < 3; ++k) { P.step_size[k] = 1.0f / 64; P.box_min[k] = 0.0f; P.box_max[k] = 1.0f; }
    P.max_samples = 300;
    const int64_t bd[3] = {64, 64, 64}, grid[3] = {2, 2, 2};
    int64_t ijk[24];
    for (int b = 0; b < 8; ++b) { ijk[3 * b] = b & 1; ijk[3 * b + 1] = (b >> 1) & 1; ijk[3 * b + 2] = b >> 2; }
    int32_t cuts[8];
    vr_status rc = vr_lod_select(&cam, &P, 8, bd, ijk, grid, 18, 25, 1.0f, cuts);
    printf("rc %d cuts", (int)rc);
    for (int b = 0; b < 8; ++b) printf(" %d", (int)cuts[b]);
    printf("\nbad %d\n", (int)vr_lod_select(&cam, &P, 8, bd, ijk, grid, 18, 25, 0.0f, cuts));
    return rc == VR_OK ? 0 : 1;
}
"""


def test_c_program_calls_lod_select(tmp_path):
    import __graft_entry__ as g
    g.build()
    src = tmp_path / "lod.c"
    src.write_text(CPROG)
    exe = str(tmp_path / "lod")
    lib = os.path.join(ROOT, "volumerenderer_amd")
    subprocess.check_call(["g++", "-x", "c++", "-std=c++14", "-O2", "-Wall", "-Werror", "-I" + os.path.join(ROOT, "include"),
                           str(src), "-L" + lib, "-lvrhip", "-Wl,-rpath," + lib, "-o", exe])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    line = r.stdout.splitlines()[0].split()
    got = np.array([int(v) for v in line[3:]], np.int32)
    cam = _cam((0.0, 0.0, -0.75), (0.0, 0.0, 1.0))
    P = default_params(1920, 1080, (64, 64, 64))
    want = rule(cam, P, (64, 64, 64), _grid_ijk((2, 2, 2)), (2, 2, 2), 18, 25, 1.0)
    assert np.array_equal(got, want), (got, want)
    assert "bad %d" % -1 in r.stdout          # VR_ERR_INVALID: pixel_tolerance must be > 0
