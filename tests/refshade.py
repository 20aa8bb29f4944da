"""A float64 NumPy restatement of the gradient-shaded compositor (vr_raycast_tf_shaded; the rule is in include/vrhip.h),
on the ray set-up and sampler of refmarch.py and the lookup of reftf.py.  Vectorised over rays; used by
test_shading_cpu.py and test_gpu_shading.py."""
import numpy as np

from refmarch import inside, march_checked, rays, tex3d
from reftf import EXIT_MARGIN, lookup


def lattice_gradient(vol, p):
    """The lattice gradient at texture positions p (..., 3) of the [Z][Y][X] volume: per corner (x0+i, y0+j, z0+k) of
    the trilinear fetch the integer central differences v(x0+i+1) - v(x0+i-1) (and y, z), every index clamped to the
    volume, interpolated with the fetch's weights and divided by 2 * 255.  Returns (..., 3)."""
    Z, Y, X = vol.shape
    G = (X, Y, Z)
    c = [p[..., k] * G[k] - 0.5 for k in range(3)]
    i0 = [np.floor(v).astype(np.int64) for v in c]
    fr = [v - i for v, i in zip(c, i0)]
    v = np.asarray(vol, np.int64)

    def V(ix, iy, iz):
        return v[np.clip(iz, 0, Z - 1), np.clip(iy, 0, Y - 1), np.clip(ix, 0, X - 1)]

    g = np.zeros(p.shape, np.float64)
    for k in (0, 1):
        for j in (0, 1):
            for i in (0, 1):
                w = (fr[0] if i else 1 - fr[0]) * (fr[1] if j else 1 - fr[1]) * (fr[2] if k else 1 - fr[2])
                x, y, z = i0[0] + i, i0[1] + j, i0[2] + k
                g[..., 0] += w * (V(x + 1, y, z) - V(x - 1, y, z))
                g[..., 1] += w * (V(x, y + 1, z) - V(x, y - 1, z))
                g[..., 2] += w * (V(x, y, z + 1) - V(x, y, z - 1))
    return g / 510.0


def shade(e_rgb, g, G, gd, ambient, diffuse, specular, shininess, light_dir, grad_min):
    """The lit colour c of the rule for table colours e_rgb (..., 3), gradients g (..., 3) of a volume of extents
    G = (X, Y, Z) and normalized ray directions gd (..., 3).  Returns (c, m): m = |g|."""
    m = np.linalg.norm(g, axis=-1)
    n = g * np.asarray(G, float)
    with np.errstate(invalid="ignore", divide="ignore"):
        N = n / np.linalg.norm(n, axis=-1, keepdims=True)
    Vv = -gd
    ld = np.asarray(light_dir, float)
    L = Vv if not np.any(ld != 0) else np.broadcast_to(ld / np.linalg.norm(ld), Vv.shape)
    Hs = L + Vv
    hn = np.linalg.norm(Hs, axis=-1, keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        Hn = Hs / hn
    ks = np.where(hn[..., 0] > 0, specular, 0.0)
    cd = np.abs((N * L).sum(-1))
    ch = np.clip(np.abs((N * Hn).sum(-1)), 1e-5, 1.0)
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.minimum(1.0, e_rgb * (ambient + diffuse * cd)[..., None] + (ks * ch ** shininess)[..., None])
    lit = m > grad_min
    return np.where(lit[..., None], c, e_rgb), m


def march_shaded(vol, covered, vuv, g, step, lut, shading, opacity_unit=0.0, background=(1.0, 1.0, 1.0), max_samples=300,
                 early_exit=True, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0)):
    """The frame of vr_raycast_tf_shaded in float64; `shading` = (ambient, diffuse, specular, shininess, light_dir,
    grad_min).  Returns (img, exit_margin, lit_margin, grad_size): per ray the min over its contributing samples of
    |T - 0.01| (early exit on; inf otherwise), of |m - grad_min|, and of m over the lit ones (inf where none)."""
    vol = np.asarray(vol)
    Z, Y, X = vol.shape
    st = g * np.asarray(step, float)
    L = np.linalg.norm(st, axis=-1)
    ex = L / opacity_unit if opacity_unit > 0 else None
    bmin, bmax = np.asarray(box_min, float), np.asarray(box_max, float)
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
        e = lookup(lut, np.where(take, tex3d(vol, q), 0.0))
        a = e[..., 3] if ex is None else 1.0 - (1.0 - e[..., 3]) ** ex
        a = np.where(take, a, 0.0)
        c, m = shade(e[..., :3], lattice_gradient(vol, q), (X, Y, Z), g, *shading)
        contrib = take & (a > 0)
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


# float32 error of m stays near 1e-7 (differences of at most 255 levels, weights in [0, 1]): a ray with a contributing
# sample closer than this to the lit / unlit decision is not compared
LIT_MARGIN = 1e-5
# below this gradient size the normal's direction is ill-conditioned in float32 (its error grows like 1e-7 / m)
GRAD_SMALL = 1e-3


def march_shaded_checked(vol, cam, W, H, step, lut, shading, opacity_unit=0.0, background=(1.0, 1.0, 1.0),
                         max_samples=300, early_exit=True, box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), near=0.1,
                         far=100.0, rows=None):
    """march_shaded on the camera cam = (pos, front, up, fov_deg) with a per-pixel slack: refmarch.march_checked's for
    the ray's geometric decisions, |T - 0.01| / EXIT_MARGIN for the early exit, |m - grad_min| / LIT_MARGIN for the
    lit / unlit choice and m / GRAD_SMALL for the normal.  slack > 1: the pixel is decidable in float32.  near / far
    are the camera's planes, `rows` the frame rows to march (default all)."""
    pos, front, up, fov = cam
    covered, vuv, g = rays(pos, front, up, fov, W, H, rows, near, far)
    img, exit_m, lit_m, gsize = march_shaded(vol, covered, vuv, g, step, lut, shading, opacity_unit, background,
                                             max_samples, early_exit, box_min, box_max)
    _, slack, _ = march_checked(vol, pos, front, up, fov, W, H, step, mode=2, max_samples=max_samples, box_min=box_min,
                                box_max=box_max, near=near, far=far, rows=rows)
    slack = np.minimum(slack, exit_m / EXIT_MARGIN)
    slack = np.minimum(slack, lit_m / LIT_MARGIN)
    slack = np.minimum(slack, gsize / GRAD_SMALL)
    return img, slack
