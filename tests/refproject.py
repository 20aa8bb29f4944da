"""A float64 NumPy restatement of the intensity projections (vr_raycast_projection; the rule is in include/vrhip.h), on
the ray set-up and sampler of refmarch.py and the owned samples of reftf.ray_samples.  Vectorised over rays; used by
test_projection_cpu.py and test_gpu_projection.py."""
import numpy as np

from refmarch import march_checked, rays
from reftf import lookup, ray_samples

MAX, MIN, MEAN = 0, 1, 2
OPS = (MAX, MIN, MEAN)


def project(vol, covered, vuv, g, step, op, max_samples=300, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
    """The projection partial of the box: (v, n) per ray -- n the owned samples, v their maximum, minimum or sum; (0, 0)
    where n = 0."""
    n = np.zeros(covered.shape)
    v = np.full(covered.shape, {MAX: 0.0, MIN: np.inf, MEAN: 0.0}[op])
    for take, s in ray_samples(vol, covered, vuv, g, step, max_samples, box_min, box_max):
        n = n + take
        if op == MAX:
            v = np.where(take, np.maximum(v, s), v)
        elif op == MIN:
            v = np.where(take, np.minimum(v, s), v)
        else:
            v = v + np.where(take, s, 0.0)
    return np.where(n > 0, v, 0.0), n


def combine(parts, op):
    """The combine of stacked partials [slabs][...][2] = (v, n), in ascending slab index: partials with n = 0 are
    ignored, n adds, v is the max, the min or the sum."""
    parts = np.asarray(parts, np.float64)
    v = np.zeros(parts.shape[1:-1])
    n = np.zeros(parts.shape[1:-1])
    for p in parts:
        has, first = p[..., 1] > 0, n == 0
        both = {MAX: np.maximum(v, p[..., 0]), MIN: np.minimum(v, p[..., 0]), MEAN: v + p[..., 0]}[op]
        v = np.where(has, np.where(first, p[..., 0], both), v)
        n = n + np.where(has, p[..., 1], 0.0)
    return np.stack([v, n], -1)


def finish(v, n, op, window=(0.0, 1.0), background=(0.0, 0.0, 0.0), lut=None):
    """Partial to pixel: n = 0: (background, 0); else m = v (MAX, MIN) or v / n (MEAN), w = clamp((m - lo) / (hi - lo),
    0, 1); grey: (w, w, w, 1); with a table: e = reftf.lookup(lut, w), (e.a e.rgb + (1 - e.a) background, e.a)."""
    lo, hi = window
    bg = np.asarray(background, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        m = np.where(n > 0, v / np.maximum(n, 1), 0.0) if op == MEAN else v
    w = np.clip((m - lo) / (hi - lo), 0.0, 1.0)
    out = np.empty(np.shape(v) + (4,))
    if lut is None:
        out[..., :3] = w[..., None]
        out[..., 3] = 1.0
    else:
        e = lookup(lut, w)
        out[..., :3] = e[..., 3:] * e[..., :3] + (1.0 - e[..., 3:]) * bg
        out[..., 3] = e[..., 3]
    empty = n == 0
    out[empty, :3] = bg
    out[empty, 3] = 0.0
    return out


def project_checked(vol, cam, W, H, step, op, window=(0.0, 1.0), background=(0.0, 0.0, 0.0), lut=None, max_samples=300,
                    box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), near=0.1, far=100.0, rows=None):
    """The frame and the partial on the camera cam = (pos, front, up, fov_deg), with refmarch.march_checked's per-pixel
    slack of the partial mode (the same positions: cube entry, near / far, inside, the clip box -- the geometric
    decisions; a projection has no exit margin).  Returns (img, v, n, slack); slack > 1: no decision can flip in
    float32.  near / far are the camera's planes, `rows` the frame rows to march (default all)."""
    pos, front, up, fov = cam
    covered, vuv, g = rays(pos, front, up, fov, W, H, rows, near, far)
    v, n = project(vol, covered, vuv, g, step, op, max_samples, box_min, box_max)
    _, slack, _ = march_checked(vol, pos, front, up, fov, W, H, step, mode=2, max_samples=max_samples, box_min=box_min,
                                box_max=box_max, near=near, far=far, rows=rows)
    return finish(v, n, op, window, background, lut), v, n, slack.reshape(covered.shape)


def owned_samples_checked(vol, cam, W, H, step, max_samples=300, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), near=0.1,
                          far=100.0, rows=None):
    """(n, slack): the number of samples each ray owns -- inside the cube and in [box_min, box_max), among its first
    max_samples steps; 0 where the cube does not cover the pixel -- and project_checked's slack.  Every marcher that has
    no early exit takes exactly these samples, whatever it does with them."""
    _, _, n, slack = project_checked(vol, cam, W, H, step, MAX, max_samples=max_samples, box_min=box_min, box_max=box_max,
                                     near=near, far=far, rows=rows)
    return n, slack
