"""The ray-march kernels against the reference's fragment shaders themselves (oracle/_ref/libvkfrag.so: raycaster.frag
and isosurface.frag compiled in place), with no restatement in between.

vr.raycast in modes 0 and 1 is compared with the frame the shader produces from the oracle's fragments (vro_fragments,
computed on the host: the camera and the rasteriser are the one part the reference does not pin).  The float frame
carries the upper clamp only, so the shader's raw vFragColor is compared as min(v, 1): bright data's red below 0 is
pinned too, not clamped away (and two frames that agree so agree after a framebuffer's clamp to [0, 1]).  Bound: the
project's 2e-3 per channel (tests/test_gpu_render.py), on every pixel, none left out.
Mode 2: a full-box partial image finished by vr_composite_finish against the same shader frame, on a volume whose
alpha never passes the shader's 0.99 exit (asserted), since a partial image has no early exit.

Each case prints one "SHADER" line with its largest difference; DESIGN.md section 2 records the largest per mode."""
import numpy as np
import pytest

import fragcases as F

pytestmark = pytest.mark.gpu
TOL = 2e-3            # tests/test_gpu_render.py


@pytest.fixture(scope="module")
def vr():
    import __graft_entry__ as g
    g.build()
    import volumerenderer_amd as vr
    return vr


@pytest.fixture(scope="module")
def O(oracle):
    if not oracle.frag_available():
        pytest.skip("oracle/_ref/libvkfrag.so is not built: no reference shaders at %s" % oracle.ref_dir())
    return oracle


def _smooth(dims, seed):
    from test_gpu_raymarch_edges import smooth
    return smooth(dims, seed)


def _iso_volume():
    vol = _smooth((21, 19, 17), 40)                         # test_gpu_raymarch_edges.py::test_iso_values
    vol[5:12, 8:11, 6:14] = 255
    vol[:, :6, :] = 0
    return vol


# (name, volume, W, H, (pos, front), step_dims or None (1 / dims), iso, modes)
def cases():
    out = [("sphere", lambda O: O.gen_sphere(64, 3), 160, 120, F.DEFAULT_CAM, None, 40 / 255.0, (0, 1))]
    noise = lambda O: np.random.default_rng(1).integers(0, 256, (32, 48, 16), dtype=np.uint8)
    for i, cam in enumerate(F.OFF_AXIS + [F.INSIDE]):       # test_gpu_render.py::test_camera_positions
        out.append(("camera %d" % i, noise, 200, 96, cam, F.BRICK_STEP, 0.5, (0, 1)))
    for iso in (0.0, 1 / 255.0, 77 / 255.0, 200 / 255.0, 1.0):
        out.append(("iso %.4f" % iso, lambda O: _iso_volume(), 33, 25, ((0.3, -0.2, -1.3), (-0.25, 0.15, 1.0)), None,
                    iso, (1,)))
    for W, H in ((7, 5), (65, 63)):                         # test_gpu_raymarch_edges.py::test_image_sizes
        out.append(("size %dx%d" % (W, H), lambda O: _smooth((24, 20, 28), 1), W, H,
                    ((0.05, -0.03, -1.4), (-0.02, 0.01, 1.0)), None, 0.55, (0, 1)))
    return out


def shader_rows(O, vol, cam, P, rows):
    """The shader's frame on the given rows only, with the upper clamp: ([len(rows)][W][4], raw, covered)."""
    vuv, covered = O.fragments(cam, P)
    vuv, covered = vuv[rows], covered[rows]
    S = O.RefShader(1 if P.mode == 1 else 0)
    assert S.max_samples == P.max_samples
    raw = np.ones(covered.shape + (4,), np.float32)
    raw[covered] = S.shade(vol, tuple(cam.pos), tuple(P.step_size), P.iso_value, vuv[covered])
    return np.minimum(raw, np.float32(1)), raw, covered


def _gpu_frame(vr, vol, cam, P, mode):
    """The kernels' frame for the oracle-side (cam, P): the two libraries' structs share one layout."""
    z, y, x = vol.shape
    cg = vr.default_camera()
    cg.pos[:] = cam.pos[:]; cg.front[:] = cam.front[:]; cg.up[:] = cam.up[:]
    cg.fov_deg, cg.z_near, cg.z_far = cam.fov_deg, cam.z_near, cam.z_far
    Pg = vr.default_params(P.width, P.height, (1, 1, 1), mode, P.iso_value)
    Pg.step_size[:] = P.step_size[:]
    assert Pg.max_samples == P.max_samples
    img = vr.raycast(vol.copy(), (x, y, z), cg, Pg)
    return vr.composite_finish(img).cpu().numpy() if mode == 2 else img.cpu().numpy()


def _compare(name, mode, got, want, raw, covered):
    assert np.isfinite(raw).all(), "%s: the shader left %d pixels undefined" % (name, int((~np.isfinite(raw).all(-1)).sum()))
    d = np.abs(got - want)
    print("SHADER %-14s mode %d  %5dx%-4d covered %7d  max diff %.3e" % (name, mode, got.shape[1], got.shape[0],
                                                                         int(covered.sum()), float(d.max())))
    assert covered.any() and d.max() <= TOL, (name, mode, float(d.max()), tuple(np.argwhere(d > TOL)[0]) if (d > TOL).any() else None)


@pytest.mark.parametrize("case", range(len(cases())))
def test_kernels_match_the_shader(vr, O, case):
    name, make, W, H, camera, sd, iso, modes = cases()[case]
    vol = make(O)
    z, y, x = vol.shape
    for mode in modes:
        cam, P = F.setup(O, (x, y, z), W, H, mode, camera, sd, iso)
        want, raw, covered = shader_rows(O, vol, cam, P, np.arange(H))
        _compare(name, mode, _gpu_frame(vr, vol, cam, P, mode), want, raw, covered)
        if name == "camera 0" and mode == 0:
            assert (want[covered][:, 0] < -0.1).any()       # bright data: red below 0, held to the shader's value


def test_1080p_frame_on_sampled_rows(vr, O):
    """test_gpu_raymarch_edges.py::test_full_hd_frame_every_row's frame; the shader runs every 24th row and the rows
    at both edges."""
    vol = _smooth((20, 20, 20), 2)
    W, H = 1920, 1080
    rows = np.unique(np.concatenate([np.arange(0, H, 24), [1, H // 2 - 1, H // 2, H - 2, H - 1]]))
    for mode in (0, 1):
        cam, P = F.setup(O, (20, 20, 20), W, H, mode, ((0.3, 0.2, -2.2), (-0.12, -0.08, 1.0)), (16, 16, 16), 0.5)
        want, raw, covered = shader_rows(O, vol, cam, P, rows)
        got = _gpu_frame(vr, vol, cam, P, mode)
        assert got.shape == (H, W, 4)
        _compare("1080p", mode, got[rows], want, raw, covered)


@pytest.mark.parametrize("camera", [F.DEFAULT_CAM, ((0.3, 0.2, -0.9), (-0.25, -0.15, 1.0))], ids=["default", "off-axis"])
def test_finished_partial_matches_the_shader(vr, O, camera):
    """Mode 2 over the whole box, finished by vr_composite_finish, against raycaster.frag.  A partial image marches
    without the early exit, so the volume is one on which the shader never takes it (alpha stays <= 0.99, asserted):
    both then sum the same samples, the partial as an associative (c, tau) pair."""
    vol = O.gen_sphere(32, 3) >> 2                  # a quarter of the sphere's density: alpha ends near 0.92
    cam, P = F.setup(O, (32, 32, 32), 160, 120, 0, camera)
    assert P.no_early_exit == 0
    want, raw, covered = shader_rows(O, vol, cam, P, np.arange(120))
    assert raw[covered][:, 3].max() <= 0.99 and raw[covered][:, 3].max() > 0.5
    _compare("partial", 2, _gpu_frame(vr, vol, cam, P, 2), want, raw, covered)
