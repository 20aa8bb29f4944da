"""A float64 NumPy restatement of the transfer-function compositor (vr_raycast_tf; the rule is in include/vrhip.h),
on the ray set-up and sampler of refmarch.py.  Vectorised over rays; used by test_transfer_function_cpu.py and
test_gpu_transfer_function.py."""
import numpy as np

from refmarch import inside, march_checked, rays, tex3d


def lookup(lut, s):
    """Table lookup of samples s (any shape): x = clamp(s * 255, 0, 255), i = min(floor(x), 254), f = x - i,
    e = lut[i] + f (lut[i+1] - lut[i]).  Returns (..., 4) float64 with alpha clamped to [0, 1]."""
    lut = np.asarray(lut, np.float64)
    x = np.clip(np.asarray(s, np.float64) * 255.0, 0.0, 255.0)
    i = np.minimum(np.floor(x).astype(np.int64), 254)
    f = (x - i)[..., None]
    e = lut[i] + f * (lut[i + 1] - lut[i])
    e[..., 3] = np.clip(e[..., 3], 0.0, 1.0)
    return e


def ray_samples(vol, covered, vuv, g, step, max_samples=300, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
    """The samples of vr_raycast's march, step by step: yields (take, s) per step -- take = the rays whose position is
    inside the cube and in [box_min, box_max), s their fetched values (0 elsewhere).  A ray that has left the cube stays
    out.  `vol` is the global [Z][Y][X] volume."""
    st = g * np.asarray(step, float)
    bmin, bmax = np.asarray(box_min, float), np.asarray(box_max, float)
    pos = vuv.copy()
    live = covered.copy()
    for _ in range(max_samples):
        pos = pos + st
        live = live & inside(pos)
        if not live.any():
            return
        take = live & ((pos >= bmin) & (pos < bmax)).all(-1)
        s = np.where(take, tex3d(vol, np.where(take[..., None], pos, 0.5)), 0.0)
        yield take, s


def march_tf(vol, covered, vuv, g, step, lut, opacity_unit=0.0, background=(1.0, 1.0, 1.0), max_samples=300,
             early_exit=True, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
    """The frame of vr_raycast_tf in float64.  Returns (img, exit_margin): img (..., 4) = (C + T * background, 1 - T),
    exit_margin per ray = min over its samples of |T - 0.01| while early exit is on (inf where it never applied)."""
    L = np.linalg.norm(g * np.asarray(step, float), axis=-1)
    ex = L / opacity_unit if opacity_unit > 0 else None
    C = np.zeros(covered.shape + (3,))
    T = np.ones(covered.shape)
    margin = np.full(covered.shape, np.inf)
    done = np.zeros(covered.shape, bool)
    for take, s in ray_samples(vol, covered, vuv, g, step, max_samples, box_min, box_max):
        take = take & ~done
        e = lookup(lut, s)
        a = e[..., 3] if ex is None else 1.0 - (1.0 - e[..., 3]) ** ex
        a = np.where(take, a, 0.0)
        C = C + (T * a)[..., None] * e[..., :3]
        T = T * (1.0 - a)
        if early_exit:
            margin = np.where(take, np.minimum(margin, np.abs(T - 0.01)), margin)
            done = done | (take & (T < 0.01))
            if done[covered].all():
                break
    img = np.empty(covered.shape + (4,))
    img[..., :3] = C + T[..., None] * np.asarray(background, float)
    img[..., 3] = 1.0 - T
    return img, margin


# T's float32 drift over a ray, for the smooth tables the tests use (channel slopes of a few units per unit of scalar),
# stays orders of magnitude below this: a ray whose T passes 0.01 closer than that is not compared
EXIT_MARGIN = 1e-4


def march_tf_checked(vol, cam, W, H, step, lut, opacity_unit=0.0, background=(1.0, 1.0, 1.0), max_samples=300,
                     early_exit=True, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), near=0.1, far=100.0, rows=None):
    """march_tf on the camera cam = (pos, front, up, fov_deg) with a per-pixel slack: refmarch.march_checked's for the
    ray's geometric decisions (cube entry, near / far, inside, the clip box: its partial mode marches the same
    positions), and |T - 0.01| / EXIT_MARGIN for the early exit.  slack > 1: no decision can flip in float32.
    near / far are the camera's planes, `rows` the frame rows to march (default all)."""
    pos, front, up, fov = cam
    covered, vuv, g = rays(pos, front, up, fov, W, H, rows, near, far)
    img, margin = march_tf(vol, covered, vuv, g, step, lut, opacity_unit, background, max_samples, early_exit, box_min,
                           box_max)
    _, slack, _ = march_checked(vol, pos, front, up, fov, W, H, step, mode=2, max_samples=max_samples, box_min=box_min,
                                box_max=box_max, near=near, far=far, rows=rows)
    return img, np.minimum(slack, margin / EXIT_MARGIN)
