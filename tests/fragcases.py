"""Inputs shared by the tests that pin the ray march to the reference's fragment shaders compiled in place
(oracle/_ref/libvkfrag.so): test_ref_shader_parity.py (the oracle against the shader), test_gpu_ref_shader_parity.py
(the kernels against the shader) and the golden-frame test of test_oracle_golden.py.

Volumes are uint8 [Z][Y][X], named by kind; `dims` is (X, Y, Z)."""
import numpy as np

KINDS = ("sphere", "noise", "ramp_x", "ramp_y", "ramp_z", "const0", "const51", "const255", "step", "checker")
DIMS = ((64, 64, 64), (32, 48, 16), (12, 6, 5), (1, 1, 8))

DEFAULT_CAM = ((0.0, 0.0, -0.75), (0.0, 0.0, 1.0))
# test_gpu_render.py::test_camera_positions: two off-axis cameras and one inside the cube
OFF_AXIS = [((0.9, 0.4, -0.9), (-0.6, -0.3, 0.7)), ((0.0, 1.2, 0.1), (0.0, -1.0, -0.05))]
INSIDE = ((0.1, 0.05, -0.2), (0.2, 0.1, 1.0))
# one camera on each side of the cube, a little off the axis (up stays (0, 1, 0), so the y sides look along a tilt)
SIDES = [((1.6, 0.1, 0.05), (-1.0, -0.05, 0.0)), ((-1.6, 0.1, 0.05), (1.0, -0.05, 0.0)),
         ((0.1, 1.6, 0.3), (0.0, -1.0, -0.2)), ((0.1, -1.6, 0.3), (0.0, 1.0, -0.2)),
         ((0.1, 0.05, 1.6), (-0.05, 0.0, -1.0)), ((0.1, 0.05, -1.6), (-0.05, 0.0, 1.0))]
FAR = ((0.0, 0.0, -3.0), (0.0, 0.0, 1.0))          # the cube is small on screen: the corners of the frame miss it
CAMERAS = [DEFAULT_CAM] + OFF_AXIS + [INSIDE] + SIDES + [FAR]

BRICK_STEP = (256, 256, 128)                       # the reference's BRICK_DIM style: step_size = 1 / these
ISO_VALUES = (0.0, 1 / 255.0, 77 / 255.0, 0.5, 1.0)


def volume(kind, dims, seed=0):
    X, Y, Z = dims
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    if kind == "sphere" and X == Y == Z:      # SURVEY 8d's generator, as test_gpu_render.py::test_sphere_matches_oracle
        from oracle import oracle as O
        return O.gen_sphere(X, 3, 12345 + seed)
    if kind == "sphere":      # other extents: a radial falloff about the centre plus two bits of noise
        r = np.sqrt(((x + 0.5) / X - 0.5) ** 2 + ((y + 0.5) / Y - 0.5) ** 2 + ((z + 0.5) / Z - 0.5) ** 2)
        v = 255.0 * np.clip(1.0 - 2.0 * r, 0.0, 1.0) + np.random.default_rng(seed).integers(0, 4, (Z, Y, X))
    elif kind == "noise":
        v = np.random.default_rng(seed).integers(0, 256, (Z, Y, X))
    elif kind.startswith("ramp_"):
        c, n = {"x": (x, X), "y": (y, Y), "z": (z, Z)}[kind[-1]]
        v = np.rint(255.0 * c / max(n - 1, 1)) if n > 1 else np.full((Z, Y, X), 128.0)
    elif kind.startswith("const"):
        v = np.full((Z, Y, X), int(kind[5:]))
    elif kind == "step":      # 0 | 255 across the longest axis
        a = int(np.argmax(dims))
        v = np.where((x, y, z)[a] * 2 >= dims[a], 255, 0)
    elif kind == "checker":
        v = ((x + y + z) & 1) * 255
    else:
        raise KeyError(kind)
    return np.ascontiguousarray(np.clip(v, 0, 255).astype(np.uint8))


def setup(O, dims, W, H, mode, cam=DEFAULT_CAM, step_dims=None, iso=0.5):
    """(camera, params) of the oracle's ctypes structs; the kernels' structs have the same layout."""
    c = O.default_camera()
    c.pos[:] = cam[0]
    c.front[:] = cam[1]
    P = O.default_params(W, H, step_dims or dims, mode, iso)
    return c, P


def shader_frame(O, vol, cam, P):
    """The shader's frame from the oracle's fragments: (raw float32 [H][W][4], clamped as the framebuffer clamps,
    covered bool [H][W]).  The marcher's mode 1 is isosurface.frag; modes 0 and 2 are raycaster.frag."""
    S = O.RefShader(1 if P.mode == 1 else 0)
    assert S.max_samples == P.max_samples, "MAX_SAMPLES is a constant of the shader"
    raw, covered = S.frame(vol, cam, P)
    return raw, S.clamp(raw), covered


# The frames of tests/golden/ref_frag_frames.npz: (kind, dims, seed, camera, step_dims or None (1 / dims), mode, iso).
GOLDEN_W, GOLDEN_H = 12, 9
GOLDEN = [("sphere", (64, 64, 64), 0, DEFAULT_CAM, None, 0, 0.5),
          ("sphere", (64, 64, 64), 0, OFF_AXIS[0], BRICK_STEP, 1, 77 / 255.0),
          ("noise", (32, 48, 16), 1, OFF_AXIS[1], BRICK_STEP, 0, 0.5),
          ("noise", (32, 48, 16), 1, INSIDE, None, 1, 0.5),
          ("const255", (12, 6, 5), 0, SIDES[0], None, 0, 0.5),
          ("checker", (12, 6, 5), 0, FAR, None, 1, 0.5),
          ("step", (1, 1, 8), 0, SIDES[5], BRICK_STEP, 1, 1 / 255.0),
          ("ramp_z", (1, 1, 8), 0, DEFAULT_CAM, None, 0, 0.5)]


def golden_inputs(O, i):
    kind, dims, seed, cam, sd, mode, iso = GOLDEN[i]
    c, P = setup(O, dims, GOLDEN_W, GOLDEN_H, mode, cam, sd, iso)
    return volume(kind, dims, seed), c, P
