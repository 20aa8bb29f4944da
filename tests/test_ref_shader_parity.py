"""The ray-march oracle against the reference's fragment shaders themselves (oracle/_ref/libvkfrag.so: raycaster.frag
and isosurface.frag compiled in place as C++ by oracle/Makefile's `ref` target): CPU only, bit-exact.

oracle/raymarch_oracle.c, tests/refmarch.py and the kernels were written from one reading of the shader text; these
tests take that reading out of the loop.  The shader is handed exactly the fragments the oracle marches from
(vro_fragments).  On every covered pixel vro_render's frame equals the shader's raw vFragColor with the upper clamp,
min(v, 1), bit for bit; so after the framebuffer's clamp to [0, 1] the two frames are equal too, which is asserted
as well, and the uncovered pixels hold the clear colour.  Both sides are float32 with contraction off and one libm, and
the stand-in (oracle/ref/glsl.h) writes dot / normalize / texture in the oracle's operation order: no tolerance.

Pinned to the reference text: the march of both shaders (the sign() stop test, the order of prev_alpha, the colour
update and the * 0.6, the > 0.99 exit, the crossing test, the bisection, DELTA, the Phong clamp, b = 255).
Not pinned by the reference: the texture filter (the stand-in's, SURVEY C-8) and the camera / rasteriser (no GLM;
vro_fragments is the oracle's own).

A pixel is left out only where the shader's raw output is not finite: normalize() of a zero gradient, which GLSL leaves
undefined and the oracle defines as N = 0.  The matrix below leaves out no pixel; test_zero_gradient_is_the_oracles_choice
provokes the case on purpose.

What the pin showed beside equality: the float frame carries the upper half of the framebuffer's clamp only.  1 - rgb
goes below 0 in bright data (rgb passes 1 because alpha takes only 0.6 of each sample: -0.66 on a constant-255
volume), exactly as the shader computes it, and vro_render and the kernels hand that on; a normalised framebuffer
clamps it to 0.  The frames keep that form (every render path and its float64 references agree on it, DESIGN.md
section 2); a consumer clamps to [0, 1] before display."""
import json
import os

import numpy as np
import pytest

import fragcases as F

GOLD = os.path.join(os.path.dirname(__file__), "golden", "ref_frag_frames.npz")
W, H = 160, 120


@pytest.fixture(scope="module")
def O(oracle):
    if not oracle.frag_available():
        pytest.skip("oracle/_ref/libvkfrag.so is not built: no reference shaders at %s" % oracle.ref_dir())
    return oracle


def check_frame(O, name, vol, cam, P):
    """Exact equality on every covered pixel (raw with the upper clamp, hence also after the framebuffer's clamp), the
    clear colour elsewhere, and no pixel left out."""
    raw, fb, covered = F.shader_frame(O, vol, cam, P)
    got = O.render(vol, cam, P)
    want = np.minimum(raw, np.float32(1))
    assert np.isfinite(raw).all(), "%s: %d pixels of the shader are not finite" % (name, int((~np.isfinite(raw).all(-1)).sum()))
    assert (got[~covered] == 1.0).all(), name
    bad = (got != want).any(-1) & covered
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        raise AssertionError("%s: pixel %s: oracle %s, shader %s (raw %s); %d such, largest difference %.3g"
                             % (name, i, got[i], want[i], raw[i], int(bad.sum()), float(np.abs(got - want)[bad].max())))
    assert np.array_equal(O.RefShader(0).clamp(got), fb), name          # what a framebuffer keeps of either
    return raw, covered


def _modes(isos):
    return [(0, 0.5)] + [(1, iso) for iso in isos]


@pytest.mark.parametrize("kind", F.KINDS)
@pytest.mark.parametrize("dims", F.DIMS, ids=lambda d: "%dx%dx%d" % d)
def test_volumes(O, kind, dims):
    """Every kind of volume at every extent: the default camera, step 1 / dims, the composite and two iso values."""
    vol = F.volume(kind, dims, 1)
    seen = 0
    for mode, iso in _modes((77 / 255.0, 0.5)):
        cam, P = F.setup(O, dims, W, H, mode, F.DEFAULT_CAM, None, iso)
        raw, covered = check_frame(O, "%s %s mode %d iso %.3f" % (kind, dims, mode, iso), vol, cam, P)
        seen += int(covered.sum())
    assert seen > 0


@pytest.mark.parametrize("ci", range(len(F.CAMERAS)))
@pytest.mark.parametrize("kind,dims", [("sphere", (64, 64, 64)), ("noise", (32, 48, 16)), ("checker", (12, 6, 5)),
                                       ("ramp_z", (1, 1, 8))])
def test_cameras_and_steps(O, ci, kind, dims):
    """Every camera with both step sizes (1 / dims and the reference's BRICK_DIM style)."""
    vol = F.volume(kind, dims, 2)
    for sd in (None, F.BRICK_STEP):
        for mode, iso in _modes((77 / 255.0,)):
            cam, P = F.setup(O, dims, W, H, mode, F.CAMERAS[ci], sd, iso)
            raw, covered = check_frame(O, "%s cam %d step %s mode %d" % (kind, ci, sd, mode), vol, cam, P)
            assert covered.any()
            if F.CAMERAS[ci] is F.FAR:
                assert not covered[0, 0] and not covered[-1, -1] and covered[H // 2, W // 2]    # the corners miss


@pytest.mark.parametrize("iso", F.ISO_VALUES)
@pytest.mark.parametrize("kind,dims", [("sphere", (64, 64, 64)), ("noise", (32, 48, 16)), ("ramp_x", (32, 48, 16)),
                                       ("step", (64, 64, 64)), ("checker", (12, 6, 5)), ("const51", (12, 6, 5)),
                                       ("ramp_z", (1, 1, 8))])
def test_iso_values(O, iso, kind, dims):
    """Iso values on and off the grey levels, 0 (nothing is below it: no hit) and 1 (only a crossing into 255 hits)."""
    vol = F.volume(kind, dims, 3)
    for camera in (F.DEFAULT_CAM, F.OFF_AXIS[0]):
        for sd in (None, F.BRICK_STEP):
            cam, P = F.setup(O, dims, W, H, 1, camera, sd, iso)
            raw, covered = check_frame(O, "%s iso %.4f step %s" % (kind, iso, sd), vol, cam, P)
            if iso == 0.0:
                assert (raw[covered] == np.float32([255, 255, 255, 1])).all()       # the shader's start colour, raw


def test_shader_constants_and_raw_output(O):
    """MAX_SAMPLES of both shaders is the value the frames above use; the raw fragment keeps b = 255, which the
    oracle clamps, and the negative red of a bright volume, which the oracle hands on and only a framebuffer clamps."""
    assert O.RefShader(0).max_samples == 300 and O.RefShader(1).max_samples == 300
    assert O.default_params(8, 8).max_samples == 300
    vol = F.volume("const255", (12, 6, 5))
    cam, P = F.setup(O, (12, 6, 5), 32, 24, 0)
    raw, want, covered = F.shader_frame(O, vol, cam, P)
    assert (raw[covered][:, 2] == 255.0).all() and raw[covered][:, 0].min() < -0.5
    assert want.min() == 0.0 and want.max() == 1.0
    got = O.render(vol, cam, P)
    assert np.array_equal(got, np.minimum(raw, np.float32(1))) and got.min() < -0.5
    assert np.array_equal(O.RefShader(0).clamp(got), want)


def test_fragments_are_the_oracles_ray_setup(O):
    """vro_fragments is what vro_render marches from: vUV lies on the cube's surface, and a frame marched by the
    shader from it has the oracle's coverage."""
    cam, P = F.setup(O, (16, 16, 16), 64, 48, 0, F.OFF_AXIS[0])
    vuv, covered = O.fragments(cam, P)
    assert covered.any() and not covered.all()
    on_face = np.minimum(np.abs(vuv[covered]), np.abs(vuv[covered] - 1)).min(-1)
    assert on_face.max() <= 4e-7 and (vuv[covered] >= -4e-7).all() and (vuv[covered] <= 1 + 4e-7).all()
    assert (vuv[~covered] == 0).all()
    img = O.render(np.zeros((16, 16, 16), np.uint8), cam, P)
    assert np.array_equal(img[..., 3] == 0.0, covered)          # an empty volume: alpha 0 exactly where covered


def test_zero_gradient_is_the_oracles_choice(O):
    """Isolated 255 voxels in a 256^3 volume are narrower than the gradient's 2 * DELTA, so a hit on one reads 0 on
    both sides in x, y and z: the shader normalises a zero vector (NaN; GLSL: undefined), the oracle defines N = 0 and
    so the colour (0, 0, 0, 1).  Those pixels, and only those, are left out; a smooth blob behind the spikes gives
    the ordinary hits."""
    n = 256
    rng = np.random.default_rng(5)
    a = ((np.arange(n, dtype=np.float32) + 0.5) / n - 0.5) ** 2
    r = np.sqrt(a[:, None, None] + a[None, :, None] + a[None, None, :])
    vol = np.clip(255.0 * (1.0 - 3.0 * r), 0, 255).astype(np.uint8)
    idx = rng.integers(8, n - 8, (400, 3))
    idx = idx[vol[idx[:, 0], idx[:, 1], idx[:, 2]] == 0][:120]          # spikes in the empty space around the blob
    vol[idx[:, 0], idx[:, 1], idx[:, 2]] = 255
    cam, P = F.setup(O, (n, n, n), W, H, 1, F.OFF_AXIS[0], None, 0.3)
    raw, want, covered = F.shader_frame(O, vol, cam, P)
    got = O.render(vol, cam, P)
    out = ~np.isfinite(raw).all(-1)
    print("zero gradient: %d of %d covered pixels left out" % (int(out.sum()), int(covered.sum())))
    assert out.any() and not (out & ~covered).any()
    assert out.sum() < 0.01 * covered.sum()
    assert (got[out] == np.float32([0, 0, 0, 1])).all()
    assert np.isnan(raw[out][:, :3]).all() and (raw[out][:, 3] == 1.0).all()
    keep = covered & ~out
    assert np.array_equal(got[keep], np.minimum(raw, np.float32(1))[keep]) and np.array_equal(got[keep], want[keep]) and (got[~covered] == 1.0).all()
    assert (want[keep][:, 0] < 1.0).sum() > 1000                         # the ordinary hits beside them


# -- golden frames: recorded shader output, so a checkout without the reference keeps the pin (test_oracle_golden.py)

def golden_frames(O):
    out = {}
    for i in range(len(F.GOLDEN)):
        vol, cam, P = F.golden_inputs(O, i)
        raw, _, covered = F.shader_frame(O, vol, cam, P)
        assert np.isfinite(raw).all()
        out["frame_%d" % i] = raw
    out["inputs"] = np.array(json.dumps(F.GOLDEN))        # kind, dims, seed, camera, step, mode, iso of each frame
    return out


def test_golden_frames_are_the_shaders(O):
    """The committed generator of tests/golden/ref_frag_frames.npz (REGENERATE_GOLDEN=1 rewrites the file): the
    reference's shaders reproduce every recorded frame bit for bit from the inputs fragcases.GOLDEN names."""
    frames = golden_frames(O)
    if os.environ.get("REGENERATE_GOLDEN") == "1":
        np.savez_compressed(GOLD, **frames)
    gold = np.load(GOLD)
    assert sorted(gold.files) == sorted(frames)
    for k, v in frames.items():
        assert gold[k].dtype == v.dtype and gold[k].tobytes() == v.tobytes(), k
    assert {F.GOLDEN[i][5] for i in range(len(F.GOLDEN))} == {0, 1}
