"""A float64 NumPy restatement of the two-dimensional transfer-function compositor (vr_raycast_tf2d; the rule is in
include/vrhip.h), on the ray set-up and sampler of refmarch.py, the value lookup of reftf.py and the lattice gradient and
lighting of refshade.py.  Vectorised over rays; used by test_transfer_function2d_cpu.py and
test_gpu_transfer_function2d.py."""
import numpy as np

from refmarch import inside, march_checked, rays, tex3d
from refshade import GRAD_SMALL, LIT_MARGIN, lattice_gradient, shade
from reftf import EXIT_MARGIN, lookup


def row_coordinate(m, grad_scale, rows):
    """y = clamp(m * grad_scale, 0, rows - 1), j = min(floor(y), rows - 2), h = y - j."""
    y = np.clip(np.asarray(m, np.float64) * grad_scale, 0.0, rows - 1.0)
    j = np.minimum(np.floor(y).astype(np.int64), rows - 2)
    return y, j, y - j


def lookup2d(lut, s, m, grad_scale):
    """The table entry of samples s with gradient magnitudes m (same shape): reftf.lookup in rows j and j + 1, blended by
    h.  lut: (rows, 256, 4).  Returns (..., 4) float64 with alpha clamped to [0, 1]."""
    lut = np.asarray(lut, np.float64)
    rows = lut.shape[0]
    _, j, h = row_coordinate(m, grad_scale, rows)
    x = np.clip(np.asarray(s, np.float64) * 255.0, 0.0, 255.0)
    i = np.minimum(np.floor(x).astype(np.int64), 254)
    f = (x - i)[..., None]
    eA = lut[j, i] + f * (lut[j, i + 1] - lut[j, i])
    eB = lut[j + 1, i] + f * (lut[j + 1, i + 1] - lut[j + 1, i])
    e = eA + h[..., None] * (eB - eA)
    e[..., 3] = np.clip(e[..., 3], 0.0, 1.0)
    return e


def march_tf2d(vol, covered, vuv, g, step, lut, grad_scale, shading=None, opacity_unit=0.0, background=(1.0, 1.0, 1.0),
               max_samples=300, early_exit=True, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), rows_seen=None):
    """The frame of vr_raycast_tf2d in float64; `shading` = None (unlit) or refshade's (ambient, diffuse, specular,
    shininess, light_dir, grad_min).  Returns (img, exit_margin, lit_margin, grad_size) as refshade.march_shaded does
    (the last two inf when unlit).  rows_seen: a list that receives the y of every taken sample (closed-form tests)."""
    vol = np.asarray(vol)
    Z, Y, X = vol.shape
    st = g * np.asarray(step, float)
    L = np.linalg.norm(st, axis=-1)
    ex = L / opacity_unit if opacity_unit > 0 else None
    bmin, bmax = np.asarray(box_min, float), np.asarray(box_max, float)
    rows = np.asarray(lut).shape[0]
    C = np.zeros(covered.shape + (3,))
    T = np.ones(covered.shape)
    exit_m = np.full(covered.shape, np.inf)
    lit_m = np.full(covered.shape, np.inf)
    gsize = np.full(covered.shape, np.inf)
    done = np.zeros(covered.shape, bool)
    pos = vuv.copy()
    live = covered.copy()
    for _ in range(max_samples):
        pos = pos + st
        live = live & inside(pos)
        if not live.any():
            break
        take = live & ((pos >= bmin) & (pos < bmax)).all(-1) & ~done
        q = np.where(take[..., None], pos, 0.5)
        grad = lattice_gradient(vol, q)
        m = np.sqrt((grad * grad).sum(-1))
        if rows_seen is not None:
            rows_seen.append(row_coordinate(m, grad_scale, rows)[0][take])
        e = lookup2d(lut, np.where(take, tex3d(vol, q), 0.0), m, grad_scale)
        a = e[..., 3] if ex is None else 1.0 - (1.0 - e[..., 3]) ** ex
        a = np.where(take, a, 0.0)
        contrib = take & (a > 0)
        c = e[..., :3]
        if shading is not None:
            c, _ = shade(c, grad, (X, Y, Z), g, *shading)
            lit_m = np.where(contrib, np.minimum(lit_m, np.abs(m - shading[5])), lit_m)
            gsize = np.where(contrib & (m > shading[5]), np.minimum(gsize, m), gsize)
        C = C + (T * a)[..., None] * np.where(contrib[..., None], c, 0.0)
        T = T * (1.0 - a)
        if early_exit:
            exit_m = np.where(take, np.minimum(exit_m, np.abs(T - 0.01)), exit_m)
            done = done | (take & (T < 0.01))
            if done[covered].all():
                break
    img = np.empty(covered.shape + (4,))
    img[..., :3] = C + T[..., None] * np.asarray(background, float)
    img[..., 3] = 1.0 - T
    return img, exit_m, lit_m, gsize


def march_tf2d_checked(vol, cam, W, H, step, lut, grad_scale, shading=None, opacity_unit=0.0, background=(1.0, 1.0, 1.0),
                       max_samples=300, early_exit=True, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), near=0.1, far=100.0,
                       rows=None):
    """march_tf2d on the camera cam = (pos, front, up, fov_deg) with refshade's per-pixel slack: refmarch.march_checked's
    for the ray's geometric decisions, |T - 0.01| / EXIT_MARGIN for the early exit and, lit, |m - grad_min| / LIT_MARGIN
    and m / GRAD_SMALL.  The row lookup adds no decision: e is continuous in y, also across rows and at the clamp.
    near / far are the camera's planes, `rows` the frame rows to march (default all; not the table's rows)."""
    pos, front, up, fov = cam
    covered, vuv, g = rays(pos, front, up, fov, W, H, rows, near, far)
    img, exit_m, lit_m, gsize = march_tf2d(vol, covered, vuv, g, step, lut, grad_scale, shading, opacity_unit, background,
                                           max_samples, early_exit, box_min, box_max)
    _, slack, _ = march_checked(vol, pos, front, up, fov, W, H, step, mode=2, max_samples=max_samples, box_min=box_min,
                                box_max=box_max, near=near, far=far, rows=rows)
    slack = np.minimum(slack, exit_m / EXIT_MARGIN)
    slack = np.minimum(slack, lit_m / LIT_MARGIN)
    slack = np.minimum(slack, gsize / GRAD_SMALL)
    return img, slack
