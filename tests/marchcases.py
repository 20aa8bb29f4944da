"""The ray edge cases of the transfer-function, shaded, two-dimensional-table and projection marchers, shared by
test_marcher_edge_cases_cpu.py (the float64 references alone: the masked fractions and that the cases show something)
and test_gpu_marcher_edges.py (the kernels against them).  Data and small builders only: nothing here needs a GPU.

The case families are those of test_gpu_raymarch_edges.py, imported so that the numbers cannot drift: its image sizes,
volume cases 0 to 10, the six SIDES, the eleven CAMS, max_samples in {0, 1, 2, 300, 2000} with early exit on and off, and
three slabs per axis with halo and vol_origin.  A case is a dict:
  name, family, k (its index: the seed of its tables), vol (the global [Z][Y][X] volume), W, H, pos, front, up, fov,
  near, far, step_dims, ns, nee, box_min, box_max, sub = {halo: (local volume, vol_origin)} or None, shows (some ray is
  meant to take samples), fine (one of the two fine-step families).
Everything a kernel is handed as float32 (camera, planes, steps, box, table, background, lighting) is rounded to float32
here, so the references march the kernel's inputs."""
import functools

import numpy as np

import refproject as RP
from refshade import march_shaded_checked
from reftf import march_tf_checked
from reftf2d import march_tf2d_checked
from test_gpu_raymarch_edges import CAMS, SIDES, _sparse_volume, _vol_cases, smooth

TOL = 2e-3              # the project's tolerance for these kernels (test_gpu_raymarch_edges.TOL)
MASKED = 0.10           # at most this share of a frame may be masked (slack <= 1) ...
MASKED_FINE = 0.20      # ... or this in the two fine-step families: with tiny steps many rays pass T = 0.01 within EXIT_MARGIN
SIZES = [(1, 1), (1, 9), (9, 1), (7, 5), (65, 63)]
NS = [0, 1, 2, 300, 2000]
MARCHERS = ("tf", "shaded", "tf2d", "tf2d_lit", "max", "min", "mean")
COLOUR = MARCHERS[:4]
OPS = {"max": RP.MAX, "min": RP.MIN, "mean": RP.MEAN}
GRAD_SCALE = 40.0       # three rows over gradients of 0 to 6.4 grey levels per voxel
COUNT_STEP = 64         # the exact-count check marches steps of at least 1 / 64: at most 111 samples, T = 2^-n >= 2^-126


def f32(v):
    return tuple(float(np.float32(q)) for q in v)


BACKGROUND = f32((0.2, 0.4, 0.6))
PROJ_BACKGROUND = f32((0.1, 0.2, 0.3))
# (ambient, diffuse, specular, shininess, light_dir, grad_min): the head light, a directional light
SHADINGS = [f32((0.3, 0.6, 0.2, 8.0)) + ((0.0, 0.0, 0.0),) + f32((1 / 255,)),
            f32((0.25, 0.6, 0.3, 16.0)) + ((0.4, 1.0, -0.6),) + f32((1 / 255,))]
AMBIENT_ONLY = (1.0, 0.0, 0.0, 16.0, (0.0, 0.0, 0.0), 0.0)


def smooth_table(seed, alpha_max=0.5):
    """(256, 4) float32: control points every 51 grey levels, linear between them; each channel moves by at most 1 per
    51 levels (slope <= 5 per unit of scalar), alpha <= alpha_max."""
    rng = np.random.default_rng(seed)
    at = np.arange(0, 256, 51)
    pts = np.concatenate([rng.uniform(0, 1, (at.size, 3)), rng.uniform(0, alpha_max, (at.size, 1))], -1)
    return np.stack([np.interp(np.arange(256), at, pts[:, c]) for c in range(4)], -1).astype(np.float32)


def smooth_table2d(seed):
    """(3, 256, 4) float32: a smooth_table per row."""
    return np.stack([smooth_table(seed + 7919 * j) for j in range(3)])


def constant_alpha_table():
    """Alpha exactly 0.5, one colour: without opacity correction and early exit T = 2^-n after n samples, exactly."""
    return np.ascontiguousarray(np.broadcast_to(np.float32([0.25, 0.5, 0.75, 0.5]), (256, 4)))


def skip_tables():
    """(one-dimensional, three-row) tables transparent on a low range: the skip grid has something to skip."""
    lut, lut2 = smooth_table(5), smooth_table2d(6)
    lut[:, 3] = np.maximum(lut[:, 3], 0.02)
    lut2[:, :, 3] = np.maximum(lut2[:, :, 3], 0.02)
    lut[:90, 3] = 0.0
    lut2[:, :90, 3] = 0.0
    return lut, lut2


def sparse_volume():
    return _sparse_volume((37, 29, 23), 3)


def _case(family, name, vol, W, H, pos, front, up=(0.0, 1.0, 0.0), fov=50.0, near=0.1, far=100.0, step_dims=None, ns=300,
          nee=0, box=None, sub=None, shows=True, fine=False):
    Z, Y, X = vol.shape
    bmin, bmax = box if box is not None else ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    return dict(family=family, name=name, vol=vol, W=W, H=H, pos=f32(pos), front=f32(front), up=f32(up), fov=float(fov),
                near=f32((near,))[0], far=f32((far,))[0], step_dims=tuple(step_dims or (X, Y, Z)), ns=ns, nee=nee,
                box_min=f32(bmin), box_max=f32(bmax), sub=sub, shows=shows, fine=fine)


@functools.lru_cache(maxsize=None)
def cases():
    out = []
    for W, H in SIZES:
        out.append(_case("size", "size %dx%d" % (W, H), smooth((24, 20, 28), 1), W, H, (0.05, -0.03, -1.4), (-0.02, 0.01, 1.0)))
    for name, vol, sd in _vol_cases()[:11]:
        out.append(_case("dims", name, vol, 33, 27, (0.4, 0.3, -1.3), (-0.35, -0.25, 1.0), step_dims=sd,
                         ns=2 if name.startswith("noise") else 300, fine=sd == (256, 256, 128)))
    for side, (pos, front) in enumerate(SIDES):
        out.append(_case("side", "side %d" % side, smooth((21, 18, 15), 10 + side), 31, 23, pos, front,
                         up=(0.0, 0.0, 1.0) if side in (2, 3) else (0.0, 1.0, 0.0)))
    for i, (name, kw, _, cov) in enumerate(CAMS):
        out.append(_case("cam", name, smooth((19, 17, 23), 20 + i - (i > 5)), 29, 21, shows=cov, **kw))
    for ns in NS:
        for nee in (0, 1):
            vol = smooth((20, 18, 22), 30)
            vol[8:14] = 255                             # an opaque slab
            out.append(_case("ns", "ns %d nee %d" % (ns, nee), vol, 25, 19, (0.2, 0.1, -1.4), (-0.1, -0.05, 1.0),
                             step_dims=(256, 256, 256) if ns == 2000 else None, ns=ns, nee=nee, shows=ns > 0,
                             fine=ns == 2000 and nee == 0))
    dims = (22, 19, 25)
    for axis in (0, 1, 2):
        vol = smooth(dims, 50 + axis)
        n = dims[axis]
        for r in range(3):
            lo, hi = r * n // 3, (r + 1) * n // 3
            bmin, bmax = [0.0, 0.0, 0.0], [1.0, 1.0, 1.0]
            bmin[axis] = lo / n
            bmax[axis] = hi / n if r < 2 else 2.0
            sub = {}
            for halo in (1, 2):                         # lit and two-dimensional-table frames read one voxel further
                a0, a1 = max(0, lo - halo), min(n, hi + halo)
                sl, org = [slice(None)] * 3, [0, 0, 0]
                sl[2 - axis] = slice(a0, a1)
                org[axis] = a0
                sub[halo] = (np.ascontiguousarray(vol[tuple(sl)]), tuple(org))
            out.append(_case("slab", "slab axis %d rank %d" % (axis, r), vol, 31, 25, (0.45, 0.35, -1.3),
                             (-0.35, -0.25, 1.0), box=(bmin, bmax), sub=sub))
    for k, c in enumerate(out):
        c["k"] = k
    return tuple(out)


HD_ROWS = [0, 1, 137, 539, 540, 811, 1078, 1079]     # the rows of the 1920 x 1080 frame that are compared


def special(name, W=48, H=40):
    """The cases outside the table, numbered after it: "hd" (the edges module's 1920 x 1080 frame), "skip" (the sparse
    volume of the skip-grid checks at steps of 1 / 64), "hit" and "miss" (a camera that sees the cube and one that sees
    nothing, for the NaN-prefilled buffers)."""
    if name == "hd":
        c = _case("special", "1080p", smooth((20, 20, 20), 2), 1920, 1080, (0.3, 0.2, -2.2), (-0.12, -0.08, 1.0),
                  step_dims=(16, 16, 16))
    elif name == "skip":
        c = _case("special", "sparse 37x29x23", sparse_volume(), W, H, (0.5, 0.4, -1.2), (-0.4, -0.3, 1.0), step_dims=(64, 64, 64))
    else:
        pos, front = {"hit": ((0.0, 0.0, -1.5), (0.0, 0.0, 1.0)), "miss": ((3.0, 3.0, 3.0), (1.0, 1.0, 1.0))}[name]
        c = _case("special", name, smooth((12, 10, 9), 3), W, H, pos, front, shows=name == "hit")
    c["k"] = len(cases()) + ("hd", "skip", "hit", "miss").index(name)
    return c


def family(name):
    return [c["k"] for c in cases() if c["family"] == name]


def inputs(c):
    """The tables, opacity unit and lighting of a case: (lut, lut2d, opacity_unit, shading).  Odd cases correct the
    opacity for a unit of 1 / 40 and take the directional light, even ones do neither.  The fine-step families stay
    uncorrected: at a step of 1 / 256 a corrected alpha of 0.25 takes under 5e-4 off T per sample near the exit at 0.01,
    so almost half of the rays that reach it would pass within EXIT_MARGIN = 1e-4 and be masked."""
    k = c["k"]
    unit = f32((1 / 40,))[0] if k % 2 and not c["fine"] else 0.0
    return smooth_table(1000 + k), smooth_table2d(2000 + k), unit, SHADINGS[k % 2]


def step_of(step_dims):
    return f32(1.0 / d for d in step_dims)


def count_step_dims(c):
    return tuple(min(d, COUNT_STEP) for d in c["step_dims"])


def _geometry(c, rows=None):
    return dict(max_samples=c["ns"], box_min=c["box_min"], box_max=c["box_max"], near=c["near"], far=c["far"], rows=rows)


def camera(c):
    return (c["pos"], c["front"], c["up"], c["fov"])


def owned(c, step_dims=None, rows=None):
    """(n, slack): the samples each ray of the case owns at 1 / step_dims (default the case's own)."""
    return RP.owned_samples_checked(c["vol"], camera(c), c["W"], c["H"], step_of(step_dims or c["step_dims"]), **_geometry(c, rows))


def reference(c, marcher, rows=None):
    """(img, slack) of one marcher's frame of the case in float64."""
    lut, lut2, unit, shp = inputs(c)
    args = (c["vol"], camera(c), c["W"], c["H"], step_of(c["step_dims"]))
    early = dict(early_exit=not c["nee"], **_geometry(c, rows))
    lut, lut2 = lut.astype(np.float64), lut2.astype(np.float64)
    if marcher == "tf":
        return march_tf_checked(*args, lut, unit, BACKGROUND, **early)
    if marcher == "shaded":
        return march_shaded_checked(*args, lut, shp, unit, BACKGROUND, **early)
    if marcher in ("tf2d", "tf2d_lit"):
        return march_tf2d_checked(*args, lut2, GRAD_SCALE, shp if marcher == "tf2d_lit" else None, unit, BACKGROUND, **early)
    img, _, _, slack = RP.project_checked(*args, OPS[marcher], (0.0, 1.0), PROJ_BACKGROUND, None, **_geometry(c, rows))
    return img, slack


@functools.lru_cache(maxsize=None)
def references(k):
    """Every reference of case k, computed once per session: {marcher: (img, slack)}, "n": (n, slack) at the case's own
    step, "count": (n, slack) at count_step_dims."""
    c = cases()[k]
    out = {m: reference(c, m) for m in MARCHERS}
    out["n"] = owned(c)
    out["count"] = out["n"] if count_step_dims(c) == c["step_dims"] else owned(c, count_step_dims(c))
    return out


def masked_cap(c):
    return MASKED_FINE if c["fine"] else MASKED


def check_masked(c, what, slack):
    """The masked-fraction condition: a cap, not a measurement.  Returns the masked count."""
    n, total = int((~(slack > 1)).sum()), slack.size
    assert n < total, "%s %s: every pixel masked" % (c["name"], what)
    assert n <= masked_cap(c) * total, "%s %s: %d of %d pixels masked" % (c["name"], what, n, total)
    return n


def count_mismatches(n_got, n_ref, slack):
    """The unmasked pixels whose sample count is not the reference's: the exact-count checks assert that there are none."""
    return int(((np.asarray(n_got) != np.asarray(n_ref)) & (slack > 1)).sum())
