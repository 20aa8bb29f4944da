"""A float64 NumPy restatement of the ray marchers, written from the GLSL text (raycaster.vert:10-21,
raycaster.frag:18-86, isosurface.frag:23-159, main.cpp:396-397 for the matrices) and, for the sort-last partial mode,
from the partial branch of k_raycast (csrc/raymarch.hip).  Vectorised over rays; shared by the tests that pin the GPU
kernels against it (test_gpu_render_pins.py, test_gpu_compositor.py)."""
import math

import numpy as np


def rays(pos, front, up, fov_deg, W, H, rows=None, near=0.1, far=100.0):
    """Per pixel centre: (covered, vUV, dir).  gl_Position = P*V*M*v with M = identity, V = lookAt, P = perspectiveFov
    (main.cpp:396-397): a pixel's ray through the unit cube [-0.5, 0.5]^3; the nearest cube-surface point in front of
    the near plane wins (depth test LESS, no culling, main.cpp:367-369); vUV = vertex + 0.5 (raycaster.vert:17)."""
    f = np.asarray(front, float); f /= np.linalg.norm(f)
    s = np.cross(f, np.asarray(up, float)); s /= np.linalg.norm(s)
    u = np.cross(s, f)
    ty = math.tan(math.radians(fov_deg) / 2); tx = ty * W / H
    ys = np.arange(H) if rows is None else np.asarray(rows)
    px, py = np.meshgrid(np.arange(W), ys)
    nx = 2 * (px + 0.5) / W - 1
    ny = 1 - 2 * (py + 0.5) / H
    d = f[None, None, :] + nx[..., None] * tx * s + ny[..., None] * ty * u          # view-space z = 1 along f
    cp = np.asarray(pos, float)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = (-0.5 - cp) / d
        hi = (0.5 - cp) / d
    t0 = np.minimum(lo, hi); t1 = np.maximum(lo, hi)
    par = d == 0
    t0 = np.where(par, -np.inf, t0); t1 = np.where(par, np.inf, t1)
    miss = (par & ((cp < -0.5) | (cp > 0.5))).any(-1)
    tn, tf = t0.max(-1), t1.min(-1)
    th = np.where(tn >= near, tn, tf)
    covered = ~miss & (tn <= tf) & (th >= near) & (th <= far)
    vuv = cp + th[..., None] * d + 0.5
    g = vuv - 0.5 - cp
    g /= np.linalg.norm(g, axis=-1, keepdims=True)
    return covered, vuv, g


def tex3d(vol, p):
    """texture(volume, p).r: R8 normalised, GL_LINEAR, clamp to edge (VolumeReader.h:120-127)."""
    Z, Y, X = vol.shape
    out = None
    c = [p[..., 0] * X - 0.5, p[..., 1] * Y - 0.5, p[..., 2] * Z - 0.5]
    i0 = [np.floor(v).astype(np.int64) for v in c]
    fr = [v - i for v, i in zip(c, i0)]
    n = [X, Y, Z]
    a = [np.clip(i, 0, m - 1) for i, m in zip(i0, n)]
    b = [np.clip(i + 1, 0, m - 1) for i, m in zip(i0, n)]
    v = vol.astype(np.float64) / 255.0
    def at(ix, iy, iz): return v[iz, iy, ix]
    c00 = at(a[0], a[1], a[2]) * (1 - fr[0]) + at(b[0], a[1], a[2]) * fr[0]
    c10 = at(a[0], b[1], a[2]) * (1 - fr[0]) + at(b[0], b[1], a[2]) * fr[0]
    c01 = at(a[0], a[1], b[2]) * (1 - fr[0]) + at(b[0], a[1], b[2]) * fr[0]
    c11 = at(a[0], b[1], b[2]) * (1 - fr[0]) + at(b[0], b[1], b[2]) * fr[0]
    c0 = c00 * (1 - fr[1]) + c10 * fr[1]
    c1 = c01 * (1 - fr[1]) + c11 * fr[1]
    return c0 * (1 - fr[2]) + c1 * fr[2]


def inside(p):
    """stop = dot(sign(p - 0), sign(1 - p)) < 3 (raycaster.frag:51): strictly inside on every axis."""
    return ((p > 0) & (p < 1)).all(-1)


def march_composite(vol, covered, vuv, g, step, max_samples=300, early_exit=True):
    """raycaster.frag:33-85 per ray.  early_exit=False ignores the alpha > 0.99 exit (:76-77), as
    vr_render_params.no_early_exit = 1 does: then the result does not depend on the order in which the samples'
    (c, tau) pairs are combined, only on the samples."""
    st = g * np.asarray(step, float)
    pos = vuv.copy()
    rgb = np.zeros(covered.shape); A = np.zeros(covered.shape)
    live = covered.copy()
    for _ in range(max_samples):
        pos = pos + st
        live = live & inside(pos)
        if not live.any():
            break
        s = tex3d(vol, np.where(live[..., None], pos, 0.5))
        pa = s - s * A
        rgb = np.where(live, rgb + pa * s, rgb)
        A = np.where(live, A + 0.6 * pa, A)
        if early_exit:
            live = live & ~(A > 0.99)
    out = np.ones(covered.shape + (4,))
    out[..., 0] = np.where(covered, 1 - rgb, 1.0)
    out[..., 1] = out[..., 0]
    out[..., 3] = np.where(covered, A, 1.0)
    return out


def march_iso(vol, covered, vuv, g, step, iso, max_samples=300):
    """isosurface.frag:77-159 per ray (Bisection :23-42, GetGradient :47-62, PhongLighting :64-75)."""
    st = g * np.asarray(step, float)
    pos = vuv.copy()
    col = np.ones(covered.shape + (4,))
    live = covered.copy()
    for _ in range(max_samples):
        pos = pos + st
        live = live & inside(pos)
        if not live.any():
            break
        safe = np.where(live[..., None], pos, 0.5)
        s1, s2 = tex3d(vol, safe), tex3d(vol, safe + st)
        hit = live & (s1 - iso < 0) & (s2 - iso >= 0)
        if hit.any():
            l, r = pos.copy(), pos + st
            for _b in range(4):
                m = (l + r) / 2
                below = tex3d(vol, np.where(hit[..., None], m, 0.5)) < iso
                l = np.where(below[..., None], m, l)
                r = np.where(below[..., None], r, m)
            tc = np.where(hit[..., None], (l + r) / 2, 0.5)
            D = 0.01
            N = np.stack([(tex3d(vol, tc - [D, 0, 0]) - tex3d(vol, tc + [D, 0, 0])) / 2,
                          (tex3d(vol, tc - [0, D, 0]) - tex3d(vol, tc + [0, D, 0])) / 2,
                          (tex3d(vol, tc - [0, 0, D]) - tex3d(vol, tc + [0, 0, D])) / 2], -1)
            nl = np.linalg.norm(N, axis=-1, keepdims=True)
            N = np.where(nl > 0, N / np.where(nl > 0, nl, 1), 0.0)
            V = -g
            diff = np.maximum((V * N).sum(-1), 0)
            Hh = V + V
            Hh = Hh / np.linalg.norm(Hh, axis=-1, keepdims=True)
            spec = np.maximum(1e-5, (Hh * N).sum(-1)) ** 250
            shade = np.minimum(1.0, diff[..., None] * np.array([0.39, 0.58, 0.93]) + spec[..., None])
            col[..., :3] = np.where(hit[..., None], shade, col[..., :3])
            live = live & ~hit
    return col


def march_partial(vol, covered, vuv, g, step, box_min, box_max, max_samples=300):
    """VR_RENDER_PARTIAL (the partial branch of k_raycast): the ray marches the whole cube with the composite shader's
    steps, but only a sample at a position p with box_min <= p < box_max on every axis is taken:
    c += tau * s^2, tau *= 1 - 0.6 s; no early exit.  `vol` is the GLOBAL volume -- a slab with a correct halo and
    vol_origin fetches the same values.  Returns (c, tau, 1, 0) per covered ray, (0, 1, 0, 0) elsewhere."""
    st = g * np.asarray(step, float)
    bmin, bmax = np.asarray(box_min, float), np.asarray(box_max, float)
    pos = vuv.copy()
    c = np.zeros(covered.shape); tau = np.ones(covered.shape)
    live = covered.copy()
    for _ in range(max_samples):
        pos = pos + st
        live = live & inside(pos)
        if not live.any():
            break
        own = live & ((pos >= bmin) & (pos < bmax)).all(-1)
        if not own.any():
            continue
        s = tex3d(vol, np.where(own[..., None], pos, 0.5))
        c = np.where(own, c + tau * s * s, c)
        tau = np.where(own, tau * (1 - 0.6 * s), tau)
    out = np.zeros(covered.shape + (4,))
    out[..., 0] = np.where(covered, c, 0.0)
    out[..., 1] = np.where(covered, tau, 1.0)
    out[..., 2] = np.where(covered, 1.0, 0.0)
    return out
