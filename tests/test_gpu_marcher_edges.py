"""The transfer-function, shaded, two-dimensional-table and projection marchers (k_raycast_tf, k_raycast_tf2d,
k_raycast_proj in csrc/raymarch.hip) at their ray edges: the case table of tests/marchcases.py -- the families of
test_gpu_raymarch_edges.py, which drives vr.raycast alone -- against the float64 references of reftf.py, refshade.py,
reftf2d.py and refproject.py.  Between them the kernels hold two more copies of k_raycast's per-pixel set-up (an inline
one in k_raycast_tf, ray_setup() under the other two) and three more march loops.

The rule for every case and each of the seven frames (tf, shaded, tf2d unlit and lit, MAX, MIN, MEAN):
  * every pixel with slack > 1 (no decision of its ray can flip in float32) matches the reference within TOL = 2e-3, the
    project's tolerance for these kernels;
  * the other pixels are masked and counted against a cap: MASKED of the frame, MASKED_FINE in the two fine-step
    families, never the whole frame (test_marcher_edge_cases_cpu.py holds the references alone to the same caps).
And without any tolerance, on every pixel whose geometric slack exceeds 1:
  * a ray that owns no sample (the cube does not cover the pixel, the near plane cuts it away, max_samples = 0, the slab
    is missed) draws (background, 0) bit for bit; its colour partial is (0, 0, 0, 1), its projection partial zeros;
  * the projection partial's n is the reference's number of owned samples, for all three ops;
  * through a table of alpha exactly 0.5 with no opacity correction and no early exit the colour partial's T is 2^-n for
    that same number, in vr_raycast_tf_partial and vr_raycast_tf2d_partial, lit and unlit, at steps of at least 1 / 64;
  * finish(partial) is the frame bit for bit.
Each case prints one "EDGE" line per frame: the largest unmasked error and the masked count."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import marchcases as MC  # noqa: E402

pytestmark = pytest.mark.gpu
COMPOSITE, SHADED, PROJECTION = 0, 3, 4           # vr_render_params.mode
MODE = {"tf": COMPOSITE, "shaded": SHADED, "tf2d": SHADED, "tf2d_lit": SHADED, "max": PROJECTION, "min": PROJECTION,
        "mean": PROJECTION}
HALO = {"tf": 1, "shaded": 2, "tf2d": 2, "tf2d_lit": 2, "max": 1, "min": 1, "mean": 1}


@pytest.fixture(scope="module")
def vr():
    import torch
    assert torch.cuda.is_available()
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


def _dev(vol):
    import torch
    return torch.from_numpy(np.ascontiguousarray(vol)).cuda().reshape(-1)


class Scene:
    """A case on the GPU: its camera, tables and lighting (the case's own unless given), and the seven frames and
    partials.  `grid_cell` attaches a skip grid of that cell size."""

    def __init__(self, vr, c, lut=None, lut2=None, unit=None, shading=None, step_dims=None, nee=None, grid_cell=0):
        self.vr, self.c = vr, c
        clut, clut2, cunit, cshp = MC.inputs(c)
        unit = cunit if unit is None else unit
        self.tf = vr.TransferFunction(clut if lut is None else lut, unit, MC.BACKGROUND)
        self.tf2 = vr.TransferFunction2D(clut2 if lut2 is None else lut2, MC.GRAD_SCALE, unit, MC.BACKGROUND)
        self.sh = vr.Shading(*(cshp if shading is None else shading))
        self.proj = {m: vr.Projection(m, (0.0, 1.0), MC.PROJ_BACKGROUND) for m in MC.OPS}
        self.step_dims = step_dims or c["step_dims"]
        self.nee = c["nee"] if nee is None else nee
        self.cam = vr.default_camera()
        self.cam.pos[:] = c["pos"]; self.cam.front[:] = c["front"]; self.cam.up[:] = c["up"]
        self.cam.fov_deg, self.cam.z_near, self.cam.z_far = c["fov"], c["near"], c["far"]
        self.vols, self.grid_cell, self.grids = {}, grid_cell, {}

    def _source(self, halo):
        """(device volume, its dims, vol_origin or None) -- the whole volume, or the case's slab with `halo` layers."""
        c = self.c
        if halo not in self.vols:
            local, org = (c["vol"], None) if c["sub"] is None else c["sub"][halo]
            self.vols[halo] = (_dev(local), local.shape[::-1], org)
        return self.vols[halo]

    def _call(self, m):
        """(device volume, dims, params) of marcher m's frame and partial calls."""
        v, dims, org = self._source(HALO[m])
        c, vr = self.c, self.vr
        P = vr.default_params(c["W"], c["H"], self.step_dims, MODE[m])
        P.max_samples, P.no_early_exit = c["ns"], self.nee
        P.box_min[:] = c["box_min"]; P.box_max[:] = c["box_max"]
        if org is not None:
            Z, Y, X = c["vol"].shape
            P.global_dims[:] = (X, Y, Z); P.vol_origin[:] = org
        if self.grid_cell:
            if id(v) not in self.grids:
                self.grids[id(v)] = vr.build_skip_grid(v, dims, self.grid_cell)
            vr.use_skip_grid(P, self.grids[id(v)], self.grid_cell)
        return v, dims, P

    def frame(self, m, out=None):
        vr = self.vr
        v, dims, P = self._call(m)
        if m == "tf":
            return vr.raycast_tf(v, dims, self.cam, P, self.tf, out=out)
        if m == "shaded":
            return vr.raycast_tf_shaded(v, dims, self.cam, P, self.tf, self.sh, out=out)
        if m in ("tf2d", "tf2d_lit"):
            return vr.raycast_tf2d(v, dims, self.cam, P, self.tf2, self.sh if m == "tf2d_lit" else None, out=out)
        return vr.raycast_projection(v, dims, self.cam, P, self.proj[m], out=out)

    def partial(self, m, out=None):
        vr = self.vr
        lit = m in ("shaded", "tf2d_lit")
        v, dims, P = self._call(m)
        if m in ("tf", "shaded"):
            return vr.raycast_tf_partial(v, dims, self.cam, P, self.tf, self.sh if lit else None, out=out)
        if m in ("tf2d", "tf2d_lit"):
            return vr.raycast_tf2d_partial(v, dims, self.cam, P, self.tf2, self.sh if lit else None, out=out)
        return vr.raycast_projection_partial(v, dims, self.cam, P, self.proj[m], out=out)

    def finish(self, m, part):
        if m in MC.COLOUR:
            return self.vr.composite_finish_tf(part, self.tf2 if m.startswith("tf2d") else self.tf)
        return self.vr.composite_finish_proj(part, self.proj[m])


def _same(want, shape):
    return np.broadcast_to(np.float32(want), shape)


def compare(c, m, got, ref, slack):
    """The pixel rule of one frame (or of some of its rows): prints the EDGE line, returns the unmasked pixels."""
    ok = slack > 1
    d = np.abs(got.astype(np.float64) - ref).max(-1)
    masked = int((~ok).sum())
    worst = float(d[ok].max()) if ok.any() else 0.0
    print("EDGE %-34s %5dx%-5d %-8s max unmasked err %.3e  masked %d/%d" % (c["name"], c["W"], c["H"], m, worst, masked, ok.size))
    assert np.isfinite(got).all(), (c["name"], m)
    bad = ok & (d > MC.TOL)
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s %s: pixel %s: kernel %s, float64 %s (slack %.3g); %d such"
                             % (c["name"], m, i, got[i], ref[i], slack[i], int(bad.sum())))
    MC.check_masked(c, m, slack)
    return ok


def check_case(vr, k):
    """Every frame and partial of case k: the pixel rule and the exact checks.  Returns the scene and its frames."""
    import torch
    c, refs = MC.cases()[k], MC.references(k)
    S = Scene(vr, c)
    n, nslack = refs["n"]
    decided = nslack > 1
    empty = decided & (n == 0)
    frames = {}
    for m in MC.MARCHERS:
        frame, part = S.frame(m), S.partial(m)
        frames[m] = frame
        got, gpart = frame.cpu().numpy(), part.cpu().numpy()
        ref, slack = refs[m]
        compare(c, m, got, ref, slack)
        colour = m in MC.COLOUR
        bg = (MC.BACKGROUND if colour else MC.PROJ_BACKGROUND) + (0.0,)
        assert np.array_equal(got[empty], _same(bg, got[empty].shape)), (c["name"], m)
        assert np.array_equal(gpart[empty], _same((0, 0, 0, 1) if colour else (0, 0, 0, 0), gpart[empty].shape)), (c["name"], m)
        assert torch.equal(S.finish(m, part), frame), (c["name"], m)
        if not colour:
            assert MC.count_mismatches(gpart[..., 1], n, nslack) == 0, (c["name"], m, gpart[..., 1][decided], n[decided])
            assert (gpart[..., 2:] == 0).all()
    # the owned samples through T = 2^-n
    cn, cslack = refs["count"]
    flat = MC.constant_alpha_table()
    Sc = Scene(vr, c, lut=flat, lut2=np.stack([flat] * 3), unit=0.0, step_dims=MC.count_step_dims(c), nee=1)
    for m in MC.COLOUR:
        T = Sc.partial(m).cpu().numpy()[..., 3]
        mant, expo = np.frexp(T)
        ngot = np.where(mant == 0.5, 1 - expo, -1)            # T = 0.5 * 2^(1 - n), or not a power of two at all
        assert MC.count_mismatches(ngot, cn, cslack) == 0, (c["name"], m, ngot[cslack > 1], cn[cslack > 1])
    return S, frames


# ---- the case families -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", MC.family("size"))
def test_image_sizes(vr, k):
    """Frames that are not whole 8x8 wave tiles, down to one pixel (its ray is the exact centre ray); the odd sizes have
    exact-zero direction components on their centre row / column."""
    check_case(vr, k)


@pytest.mark.parametrize("k", MC.family("dims"))
def test_volume_dims(vr, k):
    """Extents of 1 and 2, primes, a long axis, white noise, saturated data, brick steps of 1 / 256 and 1 / 8."""
    check_case(vr, k)


@pytest.mark.parametrize("k", MC.family("side"))
def test_cameras_on_each_side(vr, k):
    """Outside on each of the six sides, the front along an axis: lo and hi swap on every axis in turn."""
    check_case(vr, k)


@pytest.mark.parametrize("k", MC.family("cam"))
def test_camera_edges(vr, k):
    """The eleven cameras of the edges module (face planes, the edge, inside, near and far planes, tilt, narrow and wide);
    and at each an ambient-only lighting draws the unlit frame bit for bit."""
    import torch
    S, frames = check_case(vr, k)
    A = Scene(vr, S.c, shading=MC.AMBIENT_ONLY)
    assert torch.equal(A.frame("shaded"), frames["tf"]), S.c["name"]
    assert torch.equal(A.frame("tf2d_lit"), frames["tf2d"]), S.c["name"]
    assert torch.equal(A.partial("shaded"), S.partial("tf")) and torch.equal(A.partial("tf2d_lit"), S.partial("tf2d"))


@pytest.mark.parametrize("k", MC.family("ns"))
def test_max_samples(vr, k):
    """max_samples 0, 1, 2, 300 and 2000 (at steps of 1 / 256), early exit on and off, through an opaque slab."""
    check_case(vr, k)


@pytest.mark.parametrize("axis", [0, 1, 2])
def test_partial_slabs(vr, axis):
    """Rank r of 3 along `axis`: box [lo/n, hi/n) (the last rank's box_max 2.0), one halo voxel each side (two for the lit
    and two-dimensional-table frames), vol_origin; the references march the GLOBAL volume with the same box."""
    for k in MC.family("slab")[3 * axis:3 * axis + 3]:
        check_case(vr, k)


# ---- skip grids ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", [1, 3, 7, 31])
def test_skip_grid_frames_bit_identical(vr, cell):
    """Cells that do not divide 37 x 29 x 23, on tables with a transparent low range: every frame and partial with the
    grid is the one without it."""
    import torch
    c = MC.special("skip")
    lut, lut2 = MC.skip_tables()
    for nee in (0, 1):
        plain, grid = (Scene(vr, c, lut=lut, lut2=lut2, nee=nee, grid_cell=g) for g in (0, cell))
        for m in MC.MARCHERS:
            want = plain.frame(m)
            assert torch.equal(grid.frame(m), want), (cell, nee, m)
            assert torch.equal(grid.partial(m), plain.partial(m)), (cell, nee, m)
            a = want[..., 3]
            assert bool((a > 0).any()) and bool((a == 0).any()), (cell, nee, m)       # the sphere, and rays past it


# ---- every pixel is written ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(1, 1), (7, 5), (65, 63)])
def test_nan_prefilled_out_is_written_everywhere(vr, W, H):
    import torch
    for name in ("hit", "miss"):
        S = Scene(vr, MC.special(name, W, H))
        for m in MC.MARCHERS:
            for draw in (S.frame, S.partial):
                out = torch.full((H, W, 4), float("nan"), dtype=torch.float32, device="cuda")
                got = draw(m, out=out)
                assert got.data_ptr() == out.data_ptr() and not bool(torch.isnan(out).any()), (name, m, draw.__name__)
            if name == "miss":
                bg = (MC.BACKGROUND if m in MC.COLOUR else MC.PROJ_BACKGROUND) + (0.0,)
                assert np.array_equal(S.frame(m).cpu().numpy(), _same(bg, (H, W, 4))), m


def test_full_hd_frame(vr):
    """One 1920x1080 frame of the tf, lit-tf and MAX marchers into a NaN-prefilled `out`: every pixel is written, and
    eight rows (the first and last two, the two about the middle, two others) keep the pixel rule."""
    import torch
    c = MC.special("hd")
    S = Scene(vr, c)
    for m in ("tf", "shaded", "max"):
        out = torch.full((1080, 1920, 4), float("nan"), dtype=torch.float32, device="cuda")
        S.frame(m, out=out)
        got = out.cpu().numpy()
        assert not np.isnan(got).any(), m
        ref, slack = MC.reference(c, m, MC.HD_ROWS)
        ok = compare(c, m, got[MC.HD_ROWS], ref, slack)
        assert (ok & (ref[..., 3] > 0)).any() and (ok & (ref[..., 3] == 0)).any()
