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


def view_dir(cam, w, h, axis):
    """dir[axis] per pixel exactly as the kernels compute it (float32 basis, float32 pixel arithmetic)."""
    front, up, fov = cam[2], cam[3], cam[4]
    f = np.asarray(front, np.float32)
    f = f / np.float32(np.sqrt(np.sum(f * f, dtype=np.float32)))
    s = np.cross(f, np.asarray(up, np.float32)).astype(np.float32)
    s = s / np.float32(np.sqrt(np.sum(s * s, dtype=np.float32)))
    u = np.cross(s, f).astype(np.float32)
    ty = np.float32(math.tan(np.float32(0.5) * np.float32(fov) * np.float32(0.01745329251994329576923690768489)))
    tx = ty * np.float32(w) / np.float32(h)
    px, py = np.meshgrid(np.arange(w, dtype=np.float32), np.arange(h, dtype=np.float32))
    nx = np.float32(2) * (px + np.float32(0.5)) / np.float32(w) - np.float32(1)
    ny = np.float32(1) - np.float32(2) * (py + np.float32(0.5)) / np.float32(h)
    return f[axis] + nx * tx * s[axis] + ny * ty * u[axis]


# ---- margins: how close each ray came to a discrete decision ---------------------------------------------------------
# k_raycast runs the same arithmetic in float32.  Where every discrete decision of a ray (cube hit, near / far plane,
# the strict inside test, the partial box, alpha > 0.99, the iso crossings, the bisection, a zero gradient) is taken with
# more room than float32 rounding can eat, the kernel's pixel differs from this float64 one only by the propagated
# rounding, bounded below per pixel.  march_checked() returns the pixel, `slack` = min over the ray's decisions of
# (distance to the decision) / (bound on the float32 error of that distance) -- > 1 means no decision can flip -- and
# `tol`, the bound on |float32 - float64| per channel given that no decision flipped.
#
# Derivation (EPS = 2^-24 is the float32 unit roundoff, half an ulp of 1):
#  * direction: f, s, u are unit vectors normalised in float32 and tanY = tanf(...): a few roundings on terms of size
#    <= 1 + tanX + tanY, so e_dir = 8 EPS (1 + tanX + tanY) per component.  An exact zero of the float64 direction
#    arises only from exact cancellations (centre column / row of an odd W / H, zero basis components) that float32
#    reproduces; a component 0 < |d_k| < e_dir has an uncertain sign, and its slab planes matter within the longest ray
#    (z_far): margin min|cp_k +- 0.5| against e_dir * z_far.
#  * t = (+-0.5 - cp) / d: relative error 4 EPS + e_dir / |d| (two roundings, the direction's error); t0, t1, th take
#    that of the axis that sets them.  Margins |t0 - z_near|, |th - z_near|, |th - z_far|, t1 - t0.
#  * vUV = cp + th d + 0.5: e0 = 8 EPS (2 + max|cp|) + |th| (e_dir + max|d| rel(th)).  gd = vUV - 0.5 - cp has absolute
#    error e0 + 4 EPS (1 + max|cp|) on a vector of length th |d|: direction error dg = that / (th |d|) + 4 EPS.
#  * pos_k = pos_{k-1} + st in float32: each addition rounds by at most EPS (|pos| < 2), st = gd * step carries
#    |st| (dg + 2 EPS) per step, so e_pos(k) = e0 + k (EPS + max|st| (dg + 2 EPS)).  Margins: distance of pos to the
#    cube faces (inside) and, in partial mode, to box_min / box_max.
#  * a fetch moves by at most G_a * dmax_a per unit of texture position along axis a (dmax_a = the volume's largest
#    voxel-to-voxel step along a, in [0, 1]); tex3d rounds p G - 0.5 (<= EPS in texture units) and does 7 lerps on
#    values <= 1 (<= 32 EPS), so e_val(k) = sum_a G_a dmax_a (e_pos(k) + EPS) + 32 EPS.
#  * composite: A' = A + 0.6 s (1 - A), rgb' = rgb + s^2 (1 - A): eA' = eA (1 - 0.6 s) + 0.6 (1 - A) e_val + 4 EPS,
#    eR' = eR + 2 s (1 - A) e_val + s^2 eA + 4 EPS.  Margin |A - 0.99| / eA for the early exit.
#  * partial: tau' = tau (1 - 0.6 s), c' = c + tau s^2: et' = et (1 - 0.6 s) + 0.6 tau e_val + 4 EPS,
#    ec' = ec + 2 tau s e_val + s^2 et + 4 EPS.
#  * iso: margins |s1 - iso|, |s2 - iso| per step and |cm - iso| per bisection step, against e_val.  The colour bound
#    is sharper than e_val, because the specular term x^250 would multiply a loose one by 250:
#    - the six gradient fetches at tc +- 0.01 e_a sit within e_f = e_pos(k+1) + 10 EPS of the kernel's (five midpoint
#      roundings of the bisection, the 0.01f offset and its addition, the p G - 0.5 of tex3d).  While e_f is under a
#      voxel, a fetch moves by at most L(q) e_f with L(q) = sum_a G_a M_a(q), M_a(q) the largest step along a among the
#      voxels within one of q's base voxel (local_steps) -- not the volume's largest step;
#    - tex3d's own arithmetic: the eight taps q k carry 2 EPS (k = 1/255 and the product), each of the three lerp levels
#      a + f (b - a) adds EPS |result| + 2 EPS |b - a| <= 3 EPS: 11 EPS;
#    - a gradient component (s- - s+) / 2 then errs by e_c = (e(s-) + e(s+)) / 2 + EPS |N_a|, |dN| = |e_c|, and the
#      unit normal turns by at most dth_N = |dN| / (|N| - |dN|) (margin |N| / (2 |dN|));
#    - V = -gd turns by dg, the two normalisations add 8 EPS: the angle between H = V and N errs by dth = dth_N + dg +
#      8 EPS, and x = H.N = cos th by |cos(th + a) - cos th| <= sin th dth + dth^2 / 2 (+ 4 EPS for the dot product):
#      near the specular peak sin th -> 0, which is where 250 x^249 is large;
#    - the colour min(1, c_j max(x, 0) + max(1e-5, x)^250) then moves by (0.93 + 250 min(1, x + dx)^249) dx, + 16 EPS
#      for powf, the sum and the min.
#  * every output: + 2 EPS for the float32 rounding of the result itself.
EPS = 2.0 ** -24


def max_steps(vol):
    """dmax_a: the largest voxel-to-voxel step of a [Z][Y][X] uint8 volume along x, y, z, in [0, 1]."""
    v = np.asarray(vol, np.int16)
    out = []
    for ax in (2, 1, 0):
        out.append(float(np.abs(np.diff(v, axis=ax)).max()) / 255.0 if v.shape[ax] > 1 else 0.0)
    return out


def local_steps(vol):
    """M_a[z, y, x]: the largest voxel-to-voxel step along axis a (x, y, z; in [0, 1]) between voxels whose indices lie
    within [i - 1, i + 2] on every axis of (x, y, z) = i -- every step a trilinear fetch whose base voxel is within one
    voxel of i can use.  Float64 arrays shaped like vol."""
    v = np.asarray(vol, np.int16)
    out = []
    for ax in (2, 1, 0):
        d = np.zeros(v.shape)
        if v.shape[ax] > 1:
            sl = [slice(None)] * 3
            sl[ax] = slice(0, v.shape[ax] - 1)
            d[tuple(sl)] = np.abs(np.diff(v, axis=ax)) / 255.0
        for bx in range(3):                                   # max over the window [i - 1, i + 2] along each axis
            n = d.shape[bx]
            m = d.copy()
            for sh in (-1, 1, 2):
                src = [slice(None)] * 3; dst = [slice(None)] * 3
                if sh > 0:
                    if sh >= n:
                        continue
                    src[bx] = slice(sh, n); dst[bx] = slice(0, n - sh)
                else:
                    if -sh >= n:
                        continue
                    src[bx] = slice(0, n + sh); dst[bx] = slice(-sh, n)
                m[tuple(dst)] = np.maximum(m[tuple(dst)], d[tuple(src)])
            d = m
        out.append(d)
    return out


def march_checked(vol, pos, front, up, fov_deg, W, H, step, mode=0, iso=0.0, max_samples=300, early_exit=True,
                  box_min=(0.0, 0.0, 0.0), box_max=(1.0, 1.0, 1.0), near=0.1, far=100.0, rows=None):
    """The frame k_raycast draws (mode 0 composite, 1 iso, 2 partial) on the rows `rows` (default all), in float64,
    with per-pixel `slack` and `tol` (see above).  `vol` is the global [Z][Y][X] volume.  Returns (img, slack, tol):
    img and tol shaped (rows, W, 4), slack (rows, W)."""
    vol = np.asarray(vol)
    Z, Y, X = vol.shape
    f = np.asarray(front, float); f = f / np.linalg.norm(f)
    s = np.cross(f, np.asarray(up, float)); s = s / np.linalg.norm(s)
    u = np.cross(s, f)
    ty = math.tan(math.radians(fov_deg) / 2); tx = ty * W / H
    ys = np.arange(H) if rows is None else np.asarray(rows)
    px, py = np.meshgrid(np.arange(W), ys)
    shape = px.shape
    nx = (2 * (px + 0.5) / W - 1).ravel(); ny = (1 - 2 * (py + 0.5) / H).ravel()
    d = f[None, :] + nx[:, None] * tx * s + ny[:, None] * ty * u
    cp = np.asarray(pos, float)
    n = d.shape[0]
    e_dir = 8 * EPS * (1 + tx + ty)
    ad = np.abs(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        lo = (-0.5 - cp) / d; hi = (0.5 - cp) / d
        rel = 4 * EPS + e_dir / ad
    par = d == 0
    t0a = np.where(par, -np.inf, np.minimum(lo, hi)); t1a = np.where(par, np.inf, np.maximum(lo, hi))
    miss = (par & ((cp < -0.5) | (cp > 0.5))).any(-1)
    k0 = t0a.argmax(-1); k1 = t1a.argmin(-1)
    tn = t0a[np.arange(n), k0]; tf = t1a[np.arange(n), k1]
    with np.errstate(invalid="ignore"):
        etn = np.abs(tn) * rel[np.arange(n), k0] + EPS; etf = np.abs(tf) * rel[np.arange(n), k1] + EPS
    th = np.where(tn >= near, tn, tf); eth = np.where(tn >= near, etn, etf)
    covered = ~miss & (tn <= tf) & (th >= near) & (th <= far)
    slack = np.full(n, np.inf)

    def upd(idx, margin, err):
        with np.errstate(divide="ignore", invalid="ignore"):
            r = np.where(err > 0, np.abs(margin) / err, np.inf)
        np.minimum.at(slack, idx, np.nan_to_num(r, nan=0.0))

    allr = np.arange(n)
    fin = np.isfinite(tn) & np.isfinite(tf)
    upd(allr[fin], (tn - near)[fin], etn[fin])
    upd(allr[fin], (tf - tn)[fin], (etn + etf)[fin])
    okth = np.isfinite(th)
    upd(allr[okth], (th - near)[okth], eth[okth])
    upd(allr[okth], (th - far)[okth], eth[okth])
    tiny = (ad > 0) & (ad < e_dir)
    for k in range(3):
        r = allr[tiny[:, k]]
        upd(r, np.full(r.size, min(abs(cp[k] + 0.5), abs(cp[k] - 0.5))), np.full(r.size, e_dir * far))

    img = np.zeros((n, 4))
    tol = np.zeros((n, 4))
    if mode == 2:
        img[:, 1] = 1.0
    else:
        img[:] = 1.0
    idx = allr[covered]
    thc = th[idx]; dc = d[idx]
    vuv = cp + thc[:, None] * dc + 0.5
    e0 = 8 * EPS * (2 + np.abs(cp).max()) + np.abs(thc) * (e_dir + ad[idx].max(-1) * rel[idx, np.where(tn[idx] >= near, k0[idx], k1[idx])])
    gl = np.abs(thc) * np.linalg.norm(dc, axis=-1)
    with np.errstate(divide="ignore", invalid="ignore"):
        g = (vuv - 0.5 - cp) / np.linalg.norm(vuv - 0.5 - cp, axis=-1, keepdims=True)
        dg = np.where(gl > 0, (e0 + 4 * EPS * (1 + np.abs(cp).max())) / gl, np.inf) + 4 * EPS
    upd(idx, np.zeros(idx.size), np.where(gl > 0, 0.0, 1.0))               # th |d| == 0: no direction at all
    g = np.nan_to_num(g)
    st = g * np.asarray(step, float)
    dpos = EPS + np.abs(st).max(-1) * (dg + 2 * EPS)
    G = np.array([X, Y, Z], float)
    Gd = float((G * np.array(max_steps(vol))).sum())
    Mloc = local_steps(vol) if mode == 1 else None
    bmin, bmax = np.asarray(box_min, float), np.asarray(box_max, float)
    m = idx.size
    p = vuv.copy()
    rgb = np.zeros(m); A = np.zeros(m); eR = np.zeros(m); eA = np.zeros(m)
    c = np.zeros(m); tau = np.ones(m); ec = np.zeros(m); et = np.zeros(m)
    col = np.ones((m, 3)); ecol = np.zeros(m)
    live = np.arange(m)
    for k in range(1, max_samples + 1):
        if live.size == 0:
            break
        p[live] = p[live] + st[live]
        pl = p[live]
        epos = e0[live] + k * dpos[live]
        upd(idx[live], np.minimum(np.abs(pl), np.abs(1 - pl)).min(-1), epos)
        ins = ((pl > 0) & (pl < 1)).all(-1)
        live = live[ins]; pl = pl[ins]; epos = epos[ins]
        if live.size == 0:
            break
        ev = Gd * (epos + EPS) + 32 * EPS
        if mode == 0:
            sm = tex3d(vol, pl)
            a = A[live]
            eA[live] = eA[live] * (1 - 0.6 * sm) + 0.6 * (1 - a) * ev + 4 * EPS
            eR[live] = eR[live] + 2 * sm * (1 - a) * ev + sm * sm * eA[live] + 4 * EPS
            pa = sm - sm * a
            rgb[live] += pa * sm
            A[live] = a + 0.6 * pa
            if early_exit:
                upd(idx[live], A[live] - 0.99, eA[live])
                live = live[~(A[live] > 0.99)]
        elif mode == 2:
            upd(idx[live], np.minimum(np.abs(pl - bmin), np.abs(pl - bmax)).min(-1), epos)
            own = ((pl >= bmin) & (pl < bmax)).all(-1)
            o = live[own]; sm = tex3d(vol, pl[own]); evo = ev[own]
            et[o] = et[o] * (1 - 0.6 * sm) + 0.6 * tau[o] * evo + 4 * EPS
            ec[o] = ec[o] + 2 * tau[o] * sm * evo + sm * sm * et[o] + 4 * EPS
            c[o] += tau[o] * sm * sm
            tau[o] *= 1 - 0.6 * sm
        else:
            ev2 = Gd * (epos + dpos[live] + EPS) + 32 * EPS
            s1 = tex3d(vol, pl); s2 = tex3d(vol, pl + st[live])
            if iso > 0:     # (s1 < iso <= 0 is impossible for samples >= 0 in either precision: no decision)
                upd(idx[live], s1 - iso, ev); upd(idx[live], s2 - iso, ev2)
            hit = (s1 - iso < 0) & (s2 - iso >= 0)
            if hit.any():
                h = live[hit]; evh = ev2[hit]
                l, r = p[h].copy(), p[h] + st[h]
                for _b in range(4):
                    mid = (l + r) / 2
                    cm = tex3d(vol, mid)
                    upd(idx[h], cm - iso, evh)
                    below = cm < iso
                    l = np.where(below[:, None], mid, l)
                    r = np.where(below[:, None], r, mid)
                tc = (l + r) / 2
                D = 0.01
                N = np.stack([(tex3d(vol, tc - [D, 0, 0]) - tex3d(vol, tc + [D, 0, 0])) / 2,
                              (tex3d(vol, tc - [0, D, 0]) - tex3d(vol, tc + [0, D, 0])) / 2,
                              (tex3d(vol, tc - [0, 0, D]) - tex3d(vol, tc + [0, 0, D])) / 2], -1)
                nl = np.linalg.norm(N, axis=-1)
                ef = epos[hit] + dpos[h] + 10 * EPS
                ec = np.zeros_like(N)
                for a in range(3):
                    for sg in (-D, D):
                        q = tc.copy(); q[:, a] += sg
                        i0 = [np.clip(np.floor(q[:, b] * G[b] - 0.5).astype(np.int64), 0, int(G[b]) - 1) for b in range(3)]
                        L = sum(G[b] * Mloc[b][i0[2], i0[1], i0[0]] for b in range(3))
                        L = np.where(ef * G.max() < 1, L, Gd)        # (the window holds for a shift under a voxel)
                        ec[:, a] += (L * ef + 11 * EPS) / 2
                    ec[:, a] += EPS * np.abs(N[:, a])
                dN = np.linalg.norm(ec, axis=-1)
                upd(idx[h], nl, 2 * dN)
                Nn = np.where(nl[:, None] > 0, N / np.where(nl > 0, nl, 1)[:, None], 0.0)
                V = -g[h]
                diff = np.maximum((V * Nn).sum(-1), 0)
                Hh = V / np.linalg.norm(V, axis=-1, keepdims=True)
                x = (Hh * Nn).sum(-1)
                with np.errstate(divide="ignore", invalid="ignore"):
                    dth = np.where(nl > dN, dN / (nl - dN), np.inf) + dg[h] + 8 * EPS
                dx = np.sqrt(np.maximum(0.0, 1 - x * x)) * dth + dth * dth / 2 + 4 * EPS
                spec = np.maximum(1e-5, x) ** 250
                col[h] = np.minimum(1.0, diff[:, None] * np.array([0.39, 0.58, 0.93]) + spec[:, None])
                with np.errstate(invalid="ignore", over="ignore"):
                    ecol[h] = np.nan_to_num((0.93 + 250 * np.minimum(1.0, np.maximum(x, 0) + dx) ** 249) * dx,
                                            nan=np.inf) + 16 * EPS
                live = live[~hit]
    if mode == 0:
        img[idx, 0] = 1 - rgb; img[idx, 1] = 1 - rgb; img[idx, 3] = A
        tol[idx, 0] = eR; tol[idx, 1] = eR; tol[idx, 3] = eA
    elif mode == 2:
        img[idx, 0] = c; img[idx, 1] = tau; img[idx, 2] = 1.0
        tol[idx, 0] = ec; tol[idx, 1] = et
    else:
        img[idx, :3] = col
        tol[idx, :3] = ecol[:, None]
    tol = np.where(tol > 0, tol + 2 * EPS, 0.0)
    return img.reshape(shape + (4,)), slack.reshape(shape), tol.reshape(shape + (4,))
