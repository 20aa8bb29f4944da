// raymarch.hip -- gfx950 kernels for the front-to-back ray-marching compositor
// (reference volume_renderer/raycaster.frag:18-86), the iso-surface marcher
// (volume_renderer/isosurface.frag:23-159), the vertex stage / proxy cube they run on
// (raycaster.vert:10-21, UnitBrick.h:54-100, main.cpp:396-402), plus the small
// data-parallel helpers of the path: brick assembly (VolumeReader.h:151-223), error
// metrics (VolumeKdTree_recover.cpp:386-411) and sort-last compositing: the three kinds of partial image (grey,
// colour, projection) as small structs and one fold, one finish and one slab kernel over the kind.  raymarch.h
// declares what the other units call.
//
// One thread per pixel; a 64-lane wave covers an 8x8 pixel tile so neighbouring rays
// touch neighbouring voxels (L1/L2 locality of the 8 trilinear taps).  The cube
// rasteriser is replaced by its per-pixel equivalent: nearest cube-surface point along
// the view ray inside [near, far] (GL_LESS, no culling: main.cpp:367-369).
#include "raymarch.h"
#include "kd_common.h"
#include <math.h>
#include <stdlib.h>

namespace vr {

struct Tex {
    const uint8_t *v;
    int X, Y, Z;       // local extents
    int GX, GY, GZ;    // global extents (== local on the single-GPU path)
    int ox, oy, oz;    // global index of local voxel 0
};

__device__ __forceinline__ int clampi(int v, int lo, int hi) { return v < lo ? lo : (v > hi ? hi : v); }
// a 16-bit word at any byte address (gfx950: still one global_load_ushort)
typedef uint16_t __attribute__((aligned(1))) u16u;

// texture(volume, p).r : R8 normalised, GL_LINEAR, clamp-to-edge, float32 weights
__device__ __forceinline__ float tex3d(const Tex &t, float px, float py, float pz)
{
    float x = px * (float)t.GX - 0.5f, y = py * (float)t.GY - 0.5f, z = pz * (float)t.GZ - 0.5f;
    float fx0 = floorf(x), fy0 = floorf(y), fz0 = floorf(z);
    float fx = x - fx0, fy = y - fy0, fz = z - fz0;
    int x0 = (int)fx0, y0 = (int)fy0, z0 = (int)fz0;
    int xa = clampi(clampi(x0, 0, t.GX - 1) - t.ox, 0, t.X - 1), xb = clampi(clampi(x0 + 1, 0, t.GX - 1) - t.ox, 0, t.X - 1);
    int ya = clampi(clampi(y0, 0, t.GY - 1) - t.oy, 0, t.Y - 1), yb = clampi(clampi(y0 + 1, 0, t.GY - 1) - t.oy, 0, t.Y - 1);
    int za = clampi(clampi(z0, 0, t.GZ - 1) - t.oz, 0, t.Z - 1), zb = clampi(clampi(z0 + 1, 0, t.GZ - 1) - t.oz, 0, t.Z - 1);
    const float k = 1.0f / 255.0f;
    const int64_t sy = t.X, sz = (int64_t)t.X * t.Y;
    const uint8_t *r0 = t.v + sy * ya + sz * za, *r1 = t.v + sy * yb + sz * za;
    const uint8_t *r2 = t.v + sy * ya + sz * zb, *r3 = t.v + sy * yb + sz * zb;
    // the two x taps of a row are neighbouring bytes except at a clamped edge: one (unaligned) 16-bit load
    // per row instead of two byte loads; at an edge both taps are the same voxel
    const bool pairx = xb == xa + 1;
    const int xl = pairx ? xa : (xa < xb ? xa : xb);
    uint32_t q0, q1, q2, q3;
    if (pairx) { q0 = *(const u16u *)(r0 + xl); q1 = *(const u16u *)(r1 + xl); q2 = *(const u16u *)(r2 + xl); q3 = *(const u16u *)(r3 + xl); }
    else { q0 = r0[xa] | (r0[xb] << 8); q1 = r1[xa] | (r1[xb] << 8); q2 = r2[xa] | (r2[xb] << 8); q3 = r3[xa] | (r3[xb] << 8); }
    float c000 = (float)(q0 & 255u) * k, c100 = (float)(q0 >> 8) * k, c010 = (float)(q1 & 255u) * k, c110 = (float)(q1 >> 8) * k;
    float c001 = (float)(q2 & 255u) * k, c101 = (float)(q2 >> 8) * k, c011 = (float)(q3 & 255u) * k, c111 = (float)(q3 >> 8) * k;
    float c00 = c000 + fx * (c100 - c000), c10 = c010 + fx * (c110 - c010);
    float c01 = c001 + fx * (c101 - c001), c11 = c011 + fx * (c111 - c011);
    float c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    return c0 + fz * (c1 - c0);
}

// ---- the level-of-detail pool (vr_raycast_pool): a virtual volume of grid * brick_dims voxels, brick cell c stored at
// pool + tab[c].offset with one byte per 2^shift box (vrhip.h).  Brick extents are powers of two.
struct PoolTex {
    const uint8_t *pool;
    const vr_pool_entry *tab;
    int lx, ly, lz;        // log2 of the brick extents
    int gx, gy;            // grid cells along x, y
};

struct PoolCell { int64_t off; int sx, sy, sz; };

// the table entry of brick cell (cx, cy, cz): one 16-byte load
__device__ __forceinline__ PoolCell pool_cell(const PoolTex &p, int cx, int cy, int cz)
{
    const uint4 e = *(const uint4 *)(p.tab + (cx + (int64_t)p.gx * (cy + (int64_t)p.gy * cz)));
    PoolCell c;
    c.off = (int64_t)((uint64_t)e.x | ((uint64_t)e.y << 32));
    c.sx = e.z & 255u; c.sy = (e.z >> 8) & 255u; c.sz = (e.z >> 16) & 255u;
    return c;
}
// byte offset in the pool of the stored voxel that virtual voxel (x, y, z) of cell c reads
__device__ __forceinline__ int64_t pool_at(const PoolTex &p, const PoolCell &c, int x, int y, int z)
{
    const int lx = (x & ((1 << p.lx) - 1)) >> c.sx, ly = (y & ((1 << p.ly) - 1)) >> c.sy, lz = (z & ((1 << p.lz) - 1)) >> c.sz;
    return c.off + lx + ((int64_t)1 << (p.lx - c.sx)) * (ly + ((int64_t)1 << (p.ly - c.sy)) * lz);
}
__device__ __forceinline__ uint32_t pool_voxel(const PoolTex &p, int x, int y, int z)
{
    const PoolCell c = pool_cell(p, x >> p.lx, y >> p.ly, z >> p.lz);
    return c.off < 0 ? 0u : (uint32_t)p.pool[pool_at(p, c, x, y, z)];
}

// tex3d of the virtual volume (GX, GY, GZ its extents): the same tap indices, weights and interpolation, only the
// byte fetch differs.  Taps in one brick (the common case): one table load; the two x taps of a row as one 16-bit load
// where the brick is stored at full x resolution.  Taps across a brick face: a table load per tap.
__device__ __forceinline__ float tex3d_pool(const PoolTex &t, int GX, int GY, int GZ, float px, float py, float pz)
{
    float x = px * (float)GX - 0.5f, y = py * (float)GY - 0.5f, z = pz * (float)GZ - 0.5f;
    float fx0 = floorf(x), fy0 = floorf(y), fz0 = floorf(z);
    float fx = x - fx0, fy = y - fy0, fz = z - fz0;
    int x0 = (int)fx0, y0 = (int)fy0, z0 = (int)fz0;
    int xa = clampi(x0, 0, GX - 1), xb = clampi(x0 + 1, 0, GX - 1);
    int ya = clampi(y0, 0, GY - 1), yb = clampi(y0 + 1, 0, GY - 1);
    int za = clampi(z0, 0, GZ - 1), zb = clampi(z0 + 1, 0, GZ - 1);
    const float k = 1.0f / 255.0f;
    uint32_t q0, q1, q2, q3;
    const int cx = xa >> t.lx, cy = ya >> t.ly, cz = za >> t.lz;
    if (cx == (xb >> t.lx) && cy == (yb >> t.ly) && cz == (zb >> t.lz)) {
        const PoolCell c = pool_cell(t, cx, cy, cz);
        if (c.off < 0) { q0 = q1 = q2 = q3 = 0u; }
        else {
            const int64_t sy = (int64_t)1 << (t.lx - c.sx), sz = sy << (t.ly - c.sy);
            const int mx = (1 << t.lx) - 1, my = (1 << t.ly) - 1, mz = (1 << t.lz) - 1;
            const int la = (xa & mx) >> c.sx, lb = (xb & mx) >> c.sx;
            const int64_t ra = sy * ((ya & my) >> c.sy), rb = sy * ((yb & my) >> c.sy);
            const int64_t pa = sz * ((za & mz) >> c.sz), pb = sz * ((zb & mz) >> c.sz);
            const uint8_t *r0 = t.pool + c.off + ra + pa, *r1 = t.pool + c.off + rb + pa;
            const uint8_t *r2 = t.pool + c.off + ra + pb, *r3 = t.pool + c.off + rb + pb;
            if (lb == la + 1) { q0 = *(const u16u *)(r0 + la); q1 = *(const u16u *)(r1 + la); q2 = *(const u16u *)(r2 + la); q3 = *(const u16u *)(r3 + la); }
            else { q0 = r0[la] | (r0[lb] << 8); q1 = r1[la] | (r1[lb] << 8); q2 = r2[la] | (r2[lb] << 8); q3 = r3[la] | (r3[lb] << 8); }
        }
    } else {
        q0 = pool_voxel(t, xa, ya, za) | (pool_voxel(t, xb, ya, za) << 8);
        q1 = pool_voxel(t, xa, yb, za) | (pool_voxel(t, xb, yb, za) << 8);
        q2 = pool_voxel(t, xa, ya, zb) | (pool_voxel(t, xb, ya, zb) << 8);
        q3 = pool_voxel(t, xa, yb, zb) | (pool_voxel(t, xb, yb, zb) << 8);
    }
    float c000 = (float)(q0 & 255u) * k, c100 = (float)(q0 >> 8) * k, c010 = (float)(q1 & 255u) * k, c110 = (float)(q1 >> 8) * k;
    float c001 = (float)(q2 & 255u) * k, c101 = (float)(q2 >> 8) * k, c011 = (float)(q3 & 255u) * k, c111 = (float)(q3 >> 8) * k;
    float c00 = c000 + fx * (c100 - c000), c10 = c010 + fx * (c110 - c010);
    float c01 = c001 + fx * (c101 - c001), c11 = c011 + fx * (c111 - c011);
    float c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    return c0 + fz * (c1 - c0);
}

__device__ __forceinline__ void norm3(float &a, float &b, float &c)
{
    float l = sqrtf(a * a + b * b + c * c);
    if (l > 0.0f) { a /= l; b /= l; c /= l; } else { a = b = c = 0.0f; }
}
__device__ __forceinline__ float sgn(float v) { return v > 0.0f ? 1.0f : (v < 0.0f ? -1.0f : 0.0f); }
__device__ __forceinline__ bool inside(float x, float y, float z)
{   // stop = dot(sign(p - texMin), sign(texMax - p)) < 3.0  (raycaster.frag:51)
    float d = sgn(x) * sgn(1.0f - x) + sgn(y) * sgn(1.0f - y) + sgn(z) * sgn(1.0f - z);
    return !(d < 3.0f);
}

// ---- empty-space skipping (new; isosurface_compressed.frag:23-29 only declares the intent) ---------------------
// grid[2 * cell] = min, [2 * cell + 1] = max over the voxels [c * S, c * S + S] per axis (S = cell size; the + 1 is the
// second tap of a trilinear fetch whose base voxel lies in the cell), clamped to the volume.  A fetch at texture position
// p has its base voxel at floor(p * G - 0.5), clamped like the taps themselves, so its eight taps lie inside that cell's
// bounds.
struct SkipGrid { const uint8_t *g; int S, nx, ny, nz; };

__global__ void __launch_bounds__(256)
k_skip_grid(const uint8_t *__restrict__ vol, int X, int Y, int Z, int S, int nx, int ny, int nz, uint8_t *__restrict__ grid,
            bool volAligned8)
{
    // one wave per cell: a lane takes whole x-rows of the cell's (S+1)^2 (y, z) columns -- S + 1 consecutive bytes,
    // fetched as aligned 8-byte pieces where the row allows it -- then a wave min / max
    const int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (cell >= (int64_t)nx * ny * nz) return;
    const int cx = (int)(cell % nx), cy = (int)((cell / nx) % ny), cz = (int)(cell / ((int64_t)nx * ny));
    const int x0 = cx * S, y0 = cy * S, z0 = cz * S;
    const int ex = min(S + 1, X - x0), ey = min(S + 1, Y - y0), ez = min(S + 1, Z - z0);
    uint32_t mn = 255, mx = 0;
    const bool wide = volAligned8 && (S & 7) == 0 && (X & 7) == 0;          // rows start 8-byte aligned
    for (int r = lane; r < ey * ez; r += 64) {
        const uint8_t *row = vol + (int64_t)x0 + (int64_t)X * ((y0 + r % ey) + (int64_t)Y * (z0 + r / ey));
        int i = 0;
        if (wide)
            for (; i + 8 <= ex; i += 8) {
                const uint2 q = *(const uint2 *)(row + i);
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const uint32_t a = (q.x >> (8 * k)) & 255u, b = (q.y >> (8 * k)) & 255u;
                    mn = min(mn, min(a, b)); mx = max(mx, max(a, b));
                }
            }
        for (; i < ex; ++i) { const uint32_t v = row[i]; mn = min(mn, v); mx = max(mx, v); }
    }
    for (int o = 32; o > 0; o >>= 1) { mn = min(mn, (uint32_t)__shfl_xor((int)mn, o)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, o)); }
    if (lane == 0) { grid[2 * cell] = (uint8_t)mn; grid[2 * cell + 1] = (uint8_t)mx; }
}

// The same grid for 8-voxel cells of a volume whose rows are multiples of 128 voxels (the assembled bench volume):
// one wave per strip of 16 cells along x.  A lane owns a 16-byte piece of a row (two cells) and every eighth of the
// strip's 9 x 9 (y, z) rows; bytes are reduced as packed 16-bit pairs, the + 1 voxel in x comes from the neighbour
// lane's first byte (the last piece reads one byte of the next strip).  Reads each voxel 1.27 times in whole
// 128-byte lines instead of 9-byte row ends by one wave per cell: 17 ms -> 3 ms for the 8 GB volume.
__global__ void __launch_bounds__(256)
k_skip_grid8(const uint8_t *__restrict__ vol, int X, int Y, int Z, int nx, int ny, int nz, uint8_t *__restrict__ grid)
{
    const int nsx = X >> 7;
    const int64_t strip = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (strip >= (int64_t)nsx * ny * nz) return;
    const int lane = threadIdx.x & 63, c = lane & 7, rr = lane >> 3;
    const int sx = (int)(strip % nsx), cy = (int)((strip / nsx) % ny), cz = (int)(strip / ((int64_t)nsx * ny));
    const int x = sx * 128 + c * 16, y0 = cy * 8, z0 = cz * 8;
    const int ey = min(9, Y - y0), ez = min(9, Z - z0), nrows = ey * ez;
    const bool more = c == 7 && x + 16 < X;            // my second cell's last voxel lies in the next strip
    vr_s16x2 mnA = pk_s(0x00FF00FFu), mxA = pk_s(0u), mnB = pk_s(0x00FF00FFu), mxB = pk_s(0u);
    uint32_t fmnA = 255, fmxA = 0, fmnB = 255, fmxB = 0, nmn = 255, nmx = 0;      // first bytes of my cells; the next strip's
    for (int r = rr; r < nrows; r += 8) {
        const uint8_t *row = vol + (int64_t)x + (int64_t)X * ((y0 + r % ey) + (int64_t)Y * (z0 + r / ey));
        const uint4 q = *(const uint4 *)row;
        const vr_s16x2 a0 = pk_s(q.x & 0x00FF00FFu), a1 = pk_s((q.x >> 8) & 0x00FF00FFu), a2 = pk_s(q.y & 0x00FF00FFu),
                       a3 = pk_s((q.y >> 8) & 0x00FF00FFu);
        const vr_s16x2 b0 = pk_s(q.z & 0x00FF00FFu), b1 = pk_s((q.z >> 8) & 0x00FF00FFu), b2 = pk_s(q.w & 0x00FF00FFu),
                       b3 = pk_s((q.w >> 8) & 0x00FF00FFu);
        mnA = __builtin_elementwise_min(mnA, __builtin_elementwise_min(__builtin_elementwise_min(a0, a1), __builtin_elementwise_min(a2, a3)));
        mxA = __builtin_elementwise_max(mxA, __builtin_elementwise_max(__builtin_elementwise_max(a0, a1), __builtin_elementwise_max(a2, a3)));
        mnB = __builtin_elementwise_min(mnB, __builtin_elementwise_min(__builtin_elementwise_min(b0, b1), __builtin_elementwise_min(b2, b3)));
        mxB = __builtin_elementwise_max(mxB, __builtin_elementwise_max(__builtin_elementwise_max(b0, b1), __builtin_elementwise_max(b2, b3)));
        const uint32_t fa = q.x & 255u, fb = q.z & 255u;
        fmnA = min(fmnA, fa); fmxA = max(fmxA, fa);
        fmnB = min(fmnB, fb); fmxB = max(fmxB, fb);
        if (more) { const uint32_t v = row[16]; nmn = min(nmn, v); nmx = max(nmx, v); }
    }
    // cell A = bytes 0..7 plus the first byte of B; cell B = bytes 8..15 plus the first byte of the next piece
    uint32_t cmnA = min(min((uint32_t)(uint16_t)mnA.x, (uint32_t)(uint16_t)mnA.y), fmnB);
    uint32_t cmxA = max(max((uint32_t)(uint16_t)mxA.x, (uint32_t)(uint16_t)mxA.y), fmxB);
    // (shuffles outside the select: a lane that sits out of a cross-lane read hands zeros to the lanes that read it)
    const uint32_t dnMn = (uint32_t)__shfl_down((int)fmnA, 1), dnMx = (uint32_t)__shfl_down((int)fmxA, 1);
    const uint32_t nbMn = c == 7 ? nmn : dnMn, nbMx = c == 7 ? nmx : dnMx;
    uint32_t cmnB = min(min((uint32_t)(uint16_t)mnB.x, (uint32_t)(uint16_t)mnB.y), nbMn);
    uint32_t cmxB = max(max((uint32_t)(uint16_t)mxB.x, (uint32_t)(uint16_t)mxB.y), nbMx);
    for (int o = 8; o < 64; o <<= 1) {
        cmnA = min(cmnA, (uint32_t)__shfl_xor((int)cmnA, o)); cmxA = max(cmxA, (uint32_t)__shfl_xor((int)cmxA, o));
        cmnB = min(cmnB, (uint32_t)__shfl_xor((int)cmnB, o)); cmxB = max(cmxB, (uint32_t)__shfl_xor((int)cmxB, o));
    }
    if (rr == 0) {
        const int64_t cell = (int64_t)(sx * 16 + 2 * c) + (int64_t)nx * (cy + (int64_t)ny * cz);
        *(uint32_t *)(grid + 2 * cell) = cmnA | (cmxA << 8) | (cmnB << 16) | (cmxB << 24);
    }
}

// bounds of the eight taps of tex3d(t, px, py, pz): (min | max << 8)
__device__ __forceinline__ uint32_t skip_bounds(const SkipGrid &sg, const Tex &t, float px, float py, float pz)
{
    const int x0 = clampi((int)floorf(px * (float)t.GX - 0.5f), 0, t.GX - 1), y0 = clampi((int)floorf(py * (float)t.GY - 0.5f), 0, t.GY - 1),
              z0 = clampi((int)floorf(pz * (float)t.GZ - 0.5f), 0, t.GZ - 1);
    const int64_t c = (x0 / sg.S) + (int64_t)sg.nx * ((y0 / sg.S) + (int64_t)sg.ny * (z0 / sg.S));
    return *(const u16u *)(sg.g + 2 * c);       // the grid may start at any byte of a caller's allocation
}

struct RayArgs {
    Tex t;
    SkipGrid sg;
    vr_camera cam;
    vr_render_params P;
    float f[3], s[3], u[3];
    float tanX, tanY;
    float *out;
};

// k_raycast's fetch: the dense volume a.t (vr_raycast) or a pool (vr_raycast_pool) whose virtual extents are a.t's
struct DenseSampler {};
__device__ __forceinline__ float sample3d(const DenseSampler &, const RayArgs &a, float x, float y, float z) { return tex3d(a.t, x, y, z); }
__device__ __forceinline__ float sample3d(const PoolTex &p, const RayArgs &a, float x, float y, float z)
{
    return tex3d_pool(p, a.t.GX, a.t.GY, a.t.GZ, x, y, z);
}

template <class SAMPLER>
__global__ void __launch_bounds__(64)
k_raycast(RayArgs a, SAMPLER tex)
{
    // 8x8 pixel tile per wave
    const int px = blockIdx.x * 8 + (threadIdx.x & 7), py = blockIdx.y * 8 + (threadIdx.x >> 3);
    const int W = a.P.width, H = a.P.height;
    if (px >= W || py >= H) return;
    float *o = a.out + 4 * ((size_t)py * W + px);
    const float nx = 2.0f * ((float)px + 0.5f) / (float)W - 1.0f;
    const float ny = 1.0f - 2.0f * ((float)py + 0.5f) / (float)H;
    float dir[3], cp[3] = {a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) dir[k] = a.f[k] + nx * a.tanX * a.s[k] + ny * a.tanY * a.u[k];
    float t0 = -INFINITY, t1 = INFINITY;
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (dir[k] != 0.0f) {
            float lo = (-0.5f - cp[k]) / dir[k], hi = (0.5f - cp[k]) / dir[k];
            if (lo > hi) { float q = lo; lo = hi; hi = q; }
            if (lo > t0) t0 = lo;
            if (hi < t1) t1 = hi;
        } else if (cp[k] < -0.5f || cp[k] > 0.5f) miss = true;
    }
    const float th = t0 >= a.cam.z_near ? t0 : t1;
    const int mode = a.P.mode;
    if (miss || t0 > t1 || th < a.cam.z_near || th > a.cam.z_far) {
        if (mode == VR_RENDER_PARTIAL) { o[0] = 0.0f; o[1] = 1.0f; o[2] = 0.0f; o[3] = 0.0f; }
        else { o[0] = o[1] = o[2] = o[3] = 1.0f; }   // clear colour (main.cpp:392)
        return;
    }
    float vuv[3], gd[3], st[3], pos[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vuv[k] = (cp[k] + th * dir[k]) + 0.5f;      // vUV = vVertex + 0.5
#pragma unroll
    for (int k = 0; k < 3; ++k) gd[k] = (vuv[k] - 0.5f) - cp[k];            // raycaster.frag:27
    norm3(gd[0], gd[1], gd[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) { st[k] = gd[k] * a.P.step_size[k]; pos[k] = vuv[k]; }
    const int ns = a.P.max_samples;
    if (mode == VR_RENDER_COMPOSITE) {
        float rgb = 0.0f, A = 0.0f;
        bool probe = true;      // ask the grid only while the ray is in empty space (the last fetch, if any, was 0)
        for (int i = 0; i < ns; ++i) {
            pos[0] = pos[0] + st[0]; pos[1] = pos[1] + st[1]; pos[2] = pos[2] + st[2];
            if (!inside(pos[0], pos[1], pos[2])) break;
            // all eight taps zero: the sample is exactly 0 and the three updates below are exact no-ops
            if (a.sg.g && probe && (skip_bounds(a.sg, a.t, pos[0], pos[1], pos[2]) >> 8) == 0u) continue;
            float smp = sample3d(tex, a, pos[0], pos[1], pos[2]);
            probe = smp == 0.0f;
            float pa = smp - (smp * A);          // raycaster.frag:69
            rgb = pa * smp + rgb;                // :70
            A += pa * 0.6f;                      // :72
            if (!a.P.no_early_exit && A > 0.99f) break; // :77
        }
        o[0] = 1.0f - rgb; o[1] = 1.0f - rgb; o[2] = 1.0f; o[3] = A;   // :82-85 (b = 255 clamps)
    } else if (mode == VR_RENDER_PARTIAL) {
        float c = 0.0f, tau = 1.0f;
        for (int i = 0; i < ns; ++i) {
            pos[0] = pos[0] + st[0]; pos[1] = pos[1] + st[1]; pos[2] = pos[2] + st[2];
            if (!inside(pos[0], pos[1], pos[2])) break;
            bool own = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) own = own && (pos[k] >= a.P.box_min[k] && pos[k] < a.P.box_max[k]);
            if (!own) continue;
            float smp = sample3d(tex, a, pos[0], pos[1], pos[2]);
            c = c + tau * (smp * smp);
            tau = tau * (1.0f - 0.6f * smp);
        }
        o[0] = c; o[1] = tau; o[2] = 1.0f; o[3] = 0.0f;
    } else {
        float col[4] = {1.0f, 1.0f, 1.0f, 1.0f};         // vec4(255,255,255,1) clamped (isosurface.frag:79)
        const float iso = a.P.iso_value;
        // A step's second fetch is at dataPos + dirStep, which IS the next step's dataPos (the same float addition of
        // the same operands): the shader fetches it twice (isosurface.frag:120-121), here the value is carried over.
        float carried = 0.0f;
        bool haveCarried = false, haveBounds = false;
        uint32_t carriedBounds = 0;
        for (int i = 0; i < ns; ++i) {
            pos[0] = pos[0] + st[0]; pos[1] = pos[1] + st[1]; pos[2] = pos[2] + st[2];
            if (!inside(pos[0], pos[1], pos[2])) break;
            if (a.sg.g) {
                // the test below needs s1 < iso <= s2.  Interpolation in float can leave the taps' range by rounding only,
                // so a whole grey level of margin decides safely: every tap of s1 above iso, or every tap of s2 below it
                // (the second position's bounds are the next step's first, like the fetch itself)
                const uint32_t b1 = haveBounds ? carriedBounds : skip_bounds(a.sg, a.t, pos[0], pos[1], pos[2]);
                haveBounds = false;
                if ((float)((int)(b1 & 255u) - 1) * (1.0f / 255.0f) >= iso) { haveCarried = false; continue; }
                const uint32_t b2 = skip_bounds(a.sg, a.t, pos[0] + st[0], pos[1] + st[1], pos[2] + st[2]);
                carriedBounds = b2; haveBounds = true;
                if ((float)((int)(b2 >> 8) + 1) * (1.0f / 255.0f) < iso) { haveCarried = false; continue; }
            }
            float s1 = haveCarried ? carried : sample3d(tex, a, pos[0], pos[1], pos[2]);
            float s2 = sample3d(tex, a, pos[0] + st[0], pos[1] + st[1], pos[2] + st[2]);
            carried = s2; haveCarried = true;
            if ((s1 - iso) < 0.0f && (s2 - iso) >= 0.0f) {                     // :126
                float l[3] = {pos[0], pos[1], pos[2]}, r[3] = {pos[0] + st[0], pos[1] + st[1], pos[2] + st[2]};
                for (int b = 0; b < 4; ++b) {                                  // Bisection :23-42
                    float m0 = (r[0] + l[0]) * 0.5f, m1 = (r[1] + l[1]) * 0.5f, m2 = (r[2] + l[2]) * 0.5f;
                    float cm = sample3d(tex, a, m0, m1, m2);
                    if (cm < iso) { l[0] = m0; l[1] = m1; l[2] = m2; } else { r[0] = m0; r[1] = m1; r[2] = m2; }
                }
                float tc0 = (r[0] + l[0]) * 0.5f, tc1 = (r[1] + l[1]) * 0.5f, tc2 = (r[2] + l[2]) * 0.5f;
                const float DELTA = 0.01f;                                     // GetGradient :47-62
                float N0 = (sample3d(tex, a, tc0 - DELTA, tc1, tc2) - sample3d(tex, a, tc0 + DELTA, tc1, tc2)) / 2.0f;
                float N1 = (sample3d(tex, a, tc0, tc1 - DELTA, tc2) - sample3d(tex, a, tc0, tc1 + DELTA, tc2)) / 2.0f;
                float N2 = (sample3d(tex, a, tc0, tc1, tc2 - DELTA) - sample3d(tex, a, tc0, tc1, tc2 + DELTA)) / 2.0f;
                norm3(N0, N1, N2);
                float V0 = -gd[0], V1 = -gd[1], V2 = -gd[2];                   // head light: L = V (:142-146)
                float diffuse = fmaxf(V0 * N0 + V1 * N1 + V2 * N2, 0.0f);
                float h0 = V0 + V0, h1 = V1 + V1, h2 = V2 + V2;
                norm3(h0, h1, h2);
                float spec = powf(fmaxf(0.00001f, h0 * N0 + h1 * N1 + h2 * N2), 250.0f); // :73
                col[0] = fminf(1.0f, diffuse * 0.39f + spec);
                col[1] = fminf(1.0f, diffuse * 0.58f + spec);
                col[2] = fminf(1.0f, diffuse * 0.93f + spec);
                col[3] = 1.0f;
                break;
            }
        }
        o[0] = col[0]; o[1] = col[1]; o[2] = col[2]; o[3] = col[3];
    }
}

// ---- direct volume rendering through a user transfer function (vr_raycast_tf; the rule is in vrhip.h) --------------
struct TfArgs {
    const float4 *lut;      // 256 (r, g, b, a), 16-byte aligned
    float unit;             // opacity_unit (0: no correction)
    float bg[3];
};

// The workgroup's table in LDS (four float4 per lane) with next_opaque[k] = the first j >= k whose alpha is not 0 (256:
// none), found by one wave-wide suffix min.  The workgroup is one wave.
__device__ __forceinline__ void tf_stage(const TfArgs &tf, float4 *lut, uint16_t *nextOpaque, int lane)
{
    float4 e[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) { e[j] = tf.lut[4 * lane + j]; lut[4 * lane + j] = e[j]; }
    int first = 256;                                    // my four entries' first non-zero alpha
#pragma unroll
    for (int j = 3; j >= 0; --j) if (e[j].w != 0.0f) first = 4 * lane + j;
    int suffix = first;                                 // min over lanes >= mine
    for (int o = 1; o < 64; o <<= 1) {
        const int u = __shfl_down(suffix, o);
        if (lane + o < 64) suffix = min(suffix, u);
    }
    const int after = __shfl_down(suffix, 1);           // min over lanes > mine
    int carry = lane == 63 ? 256 : after;
#pragma unroll
    for (int j = 3; j >= 0; --j) {
        if (e[j].w != 0.0f) carry = 4 * lane + j;
        nextOpaque[4 * lane + j] = (uint16_t)carry;
    }
}

// ---- gradient-shaded DVR (vr_raycast_tf_shaded; the rule is in vrhip.h) ---------------------------------------------
// a 32-bit word at any byte address (one global_load_dword: gfx950 takes unaligned global loads)
typedef uint32_t __attribute__((aligned(1))) u32u;

// the base voxel and weights of a trilinear fetch at texture position p of a volume of extents G (tex3d's arithmetic)
struct Lattice { int x0, y0, z0; float fx, fy, fz; };
__device__ __forceinline__ Lattice lattice(int GX, int GY, int GZ, float px, float py, float pz)
{
    float x = px * (float)GX - 0.5f, y = py * (float)GY - 0.5f, z = pz * (float)GZ - 0.5f;
    float fx0 = floorf(x), fy0 = floorf(y), fz0 = floorf(z);
    Lattice l;
    l.fx = x - fx0; l.fy = y - fy0; l.fz = z - fz0;
    l.x0 = (int)fx0; l.y0 = (int)fy0; l.z0 = (int)fz0;
    return l;
}

// The 32 voxels a lattice gradient reads, a plus-shaped set around the eight taps (indices clamped as the fetch's):
// r[j + 2k] = v(x0-1 .. x0+2, y0+j, z0+k) in bytes 0..3; ym[k] / yp[k] = v(x0 .. x0+1, y0-1 / y0+2, z0+k) and
// zm[j] / zp[j] = v(x0 .. x0+1, y0+j, z0-1 / z0+2) in bytes 0..1.
struct Nbhd { uint32_t r[4], ym[2], yp[2], zm[2], zp[2]; };

// the same 32 voxels through an accessor V(a, b, c) = the voxel at x slot a, y slot b, z slot c (slot q = offset q - 1)
template <class F>
__device__ __forceinline__ void nbhd_fill(Nbhd &n, F V)
{
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k)
            n.r[j + 2 * k] = V(0, 1 + j, 1 + k) | (V(1, 1 + j, 1 + k) << 8) | (V(2, 1 + j, 1 + k) << 16) | (V(3, 1 + j, 1 + k) << 24);
#pragma unroll
    for (int k = 0; k < 2; ++k) { n.ym[k] = V(1, 0, 1 + k) | (V(2, 0, 1 + k) << 8); n.yp[k] = V(1, 3, 1 + k) | (V(2, 3, 1 + k) << 8); }
#pragma unroll
    for (int j = 0; j < 2; ++j) { n.zm[j] = V(1, 1 + j, 0) | (V(2, 1 + j, 0) << 8); n.zp[j] = V(1, 1 + j, 3) | (V(2, 1 + j, 3) << 8); }
}

// dense: whole rows where the indices are consecutive -- one dword per x-row, one 16-bit word per y- or z-row pair --
// and byte loads at a clamped edge
__device__ __forceinline__ Nbhd gather(const DenseSampler &, const RayArgs &a, const Lattice &l)
{
    const Tex &t = a.t;
    int xi[4], yi[4], zi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        xi[q] = clampi(clampi(l.x0 + q - 1, 0, t.GX - 1) - t.ox, 0, t.X - 1);
        yi[q] = clampi(clampi(l.y0 + q - 1, 0, t.GY - 1) - t.oy, 0, t.Y - 1);
        zi[q] = clampi(clampi(l.z0 + q - 1, 0, t.GZ - 1) - t.oz, 0, t.Z - 1);
    }
    const int64_t sy = t.X, sz = (int64_t)t.X * t.Y;
    const bool row4 = xi[3] == xi[0] + 3, pair = xi[2] == xi[1] + 1;     // clamped indices step by 0 or 1
    auto row = [&](int b, int c) -> uint32_t {
        const uint8_t *r = t.v + sy * yi[b] + sz * zi[c];
        return row4 ? *(const u32u *)(r + xi[0]) : (r[xi[0]] | (r[xi[1]] << 8) | (r[xi[2]] << 16) | ((uint32_t)r[xi[3]] << 24));
    };
    auto two = [&](int b, int c) -> uint32_t {
        const uint8_t *r = t.v + sy * yi[b] + sz * zi[c];
        return pair ? (uint32_t)*(const u16u *)(r + xi[1]) : (r[xi[1]] | (r[xi[2]] << 8));
    };
    Nbhd n;
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
        for (int k = 0; k < 2; ++k) n.r[j + 2 * k] = row(1 + j, 1 + k);
#pragma unroll
    for (int k = 0; k < 2; ++k) { n.ym[k] = two(0, 1 + k); n.yp[k] = two(3, 1 + k); }
#pragma unroll
    for (int j = 0; j < 2; ++j) { n.zm[j] = two(1 + j, 0); n.zp[j] = two(1 + j, 3); }
    return n;
}

// pool: the brick cell resolved once where the 4 x 4 x 4 box of the indices lies in one cell, per voxel otherwise
__device__ __forceinline__ Nbhd gather(const PoolTex &p, const RayArgs &a, const Lattice &l)
{
    int xi[4], yi[4], zi[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        xi[q] = clampi(l.x0 + q - 1, 0, a.t.GX - 1);
        yi[q] = clampi(l.y0 + q - 1, 0, a.t.GY - 1);
        zi[q] = clampi(l.z0 + q - 1, 0, a.t.GZ - 1);
    }
    Nbhd n;
    const int cx = xi[0] >> p.lx, cy = yi[0] >> p.ly, cz = zi[0] >> p.lz;
    if (cx == (xi[3] >> p.lx) && cy == (yi[3] >> p.ly) && cz == (zi[3] >> p.lz)) {
        const PoolCell c = pool_cell(p, cx, cy, cz);
        if (c.off < 0) {
            nbhd_fill(n, [](int, int, int) -> uint32_t { return 0u; });
        } else {
            const int64_t sy = (int64_t)1 << (p.lx - c.sx), sz = sy << (p.ly - c.sy);
            const int mx = (1 << p.lx) - 1, my = (1 << p.ly) - 1, mz = (1 << p.lz) - 1;
            int64_t ox[4], oy[4], oz[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ox[q] = (xi[q] & mx) >> c.sx; oy[q] = sy * ((yi[q] & my) >> c.sy); oz[q] = sz * ((zi[q] & mz) >> c.sz);
            }
            const uint8_t *b = p.pool + c.off;
            nbhd_fill(n, [&](int u, int v, int w) -> uint32_t { return b[ox[u] + oy[v] + oz[w]]; });
        }
    } else {
        nbhd_fill(n, [&](int u, int v, int w) -> uint32_t { return pool_voxel(p, xi[u], yi[v], zi[w]); });
    }
    return n;
}

// tex3d's interpolation of eight corner values c[i + 2j + 4k]
__device__ __forceinline__ float trilerp(const float c[8], float fx, float fy, float fz)
{
    float c00 = c[0] + fx * (c[1] - c[0]), c10 = c[2] + fx * (c[3] - c[2]);
    float c01 = c[4] + fx * (c[5] - c[4]), c11 = c[6] + fx * (c[7] - c[6]);
    float c0 = c00 + fy * (c10 - c00), c1 = c01 + fy * (c11 - c01);
    return c0 + fz * (c1 - c0);
}

// the lattice gradient (vrhip.h): integer central differences at the eight corners, interpolated, scaled once
__device__ __forceinline__ void lattice_gradient(const Nbhd &n, const Lattice &l, float g[3])
{
    auto B = [](uint32_t w, int q) -> int { return (int)((w >> (8 * q)) & 255u); };
    float dx[8], dy[8], dz[8];
#pragma unroll
    for (int k = 0; k < 2; ++k)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                const int c = i + 2 * j + 4 * k;
                dx[c] = (float)(B(n.r[j + 2 * k], 2 + i) - B(n.r[j + 2 * k], i));
                dy[c] = (float)(j == 0 ? B(n.r[1 + 2 * k], 1 + i) - B(n.ym[k], i) : B(n.yp[k], i) - B(n.r[2 * k], 1 + i));
                dz[c] = (float)(k == 0 ? B(n.r[j + 2], 1 + i) - B(n.zm[j], i) : B(n.zp[j], i) - B(n.r[j], 1 + i));
            }
    const float k = 1.0f / 510.0f;
    g[0] = trilerp(dx, l.fx, l.fy, l.fz) * k;
    g[1] = trilerp(dy, l.fx, l.fy, l.fz) * k;
    g[2] = trilerp(dz, l.fx, l.fy, l.fz) * k;
}

struct ShadeArgs {
    float ka, kd, ks, shininess, gmin;
    float L[3];             // normalized light direction; head: L = V per ray
    int head;
};

// k_raycast's ray set-up and fetch, a table lookup per sample and "over" into (C, T).  The workgroup stages the table
// (tf_stage).  A sample the skip grid bounds by (mn, mx) is skippable when next_opaque[max(mn - 1, 0)] > min(mx + 1, 255).
// LIT (vr_raycast_tf_shaded; the rule is in vrhip.h): a sample with a > 0 gathers the 32 voxels of its lattice gradient
// (gather) and takes the head-light / directional Blinn-Phong of the iso-surface shader, two-sided, as its colour;
// transparent samples and empty stretches cost what they cost unlit.  The ray set-up is an inline copy of k_raycast's,
// and the lit and unlit "over" are written out apart: a shared function or a shared update schedules the code differently.
// PARTIAL (vr_raycast_tf_partial): the same march; the pixel is (C, T) as the loop leaves them, for sort-last compositing.
template <class SAMPLER, bool LIT, bool PARTIAL>
__global__ void __launch_bounds__(64)
k_raycast_tf(RayArgs a, SAMPLER tex, TfArgs tf, ShadeArgs sh)
{
    __shared__ float4 lut[256];
    __shared__ uint16_t nextOpaque[256];
    const int lane = threadIdx.x;
    tf_stage(tf, lut, nextOpaque, lane);
    __syncthreads();
    // 8x8 pixel tile per wave
    const int px = blockIdx.x * 8 + (lane & 7), py = blockIdx.y * 8 + (lane >> 3);
    const int W = a.P.width, H = a.P.height;
    if (px >= W || py >= H) return;
    float *o = a.out + 4 * ((size_t)py * W + px);
    const float nx = 2.0f * ((float)px + 0.5f) / (float)W - 1.0f;
    const float ny = 1.0f - 2.0f * ((float)py + 0.5f) / (float)H;
    float dir[3], cp[3] = {a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) dir[k] = a.f[k] + nx * a.tanX * a.s[k] + ny * a.tanY * a.u[k];
    float t0 = -INFINITY, t1 = INFINITY;
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (dir[k] != 0.0f) {
            float lo = (-0.5f - cp[k]) / dir[k], hi = (0.5f - cp[k]) / dir[k];
            if (lo > hi) { float q = lo; lo = hi; hi = q; }
            if (lo > t0) t0 = lo;
            if (hi < t1) t1 = hi;
        } else if (cp[k] < -0.5f || cp[k] > 0.5f) miss = true;
    }
    const float th = t0 >= a.cam.z_near ? t0 : t1;
    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, T = 1.0f;
    if (!(miss || t0 > t1 || th < a.cam.z_near || th > a.cam.z_far)) {
        float vuv[3], gd[3], st[3], pos[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) vuv[k] = (cp[k] + th * dir[k]) + 0.5f;
#pragma unroll
        for (int k = 0; k < 3; ++k) gd[k] = (vuv[k] - 0.5f) - cp[k];
        norm3(gd[0], gd[1], gd[2]);
#pragma unroll
        for (int k = 0; k < 3; ++k) { st[k] = gd[k] * a.P.step_size[k]; pos[k] = vuv[k]; }
        // opacity correction exponent L / opacity_unit (0 = none, or L = 0: a = 1 - t^0 = 0)
        const float L = sqrtf(st[0] * st[0] + st[1] * st[1] + st[2] * st[2]);
        const bool correct = tf.unit > 0.0f;
        const float ex = correct ? L / tf.unit : 0.0f;
        // LIT, per ray: V, the light and the half vector; no specular term where L + V = 0
        const float V0 = -gd[0], V1 = -gd[1], V2 = -gd[2];
        const float L0 = sh.head ? V0 : sh.L[0], L1 = sh.head ? V1 : sh.L[1], L2 = sh.head ? V2 : sh.L[2];
        float H0 = L0 + V0, H1 = L1 + V1, H2 = L2 + V2;
        const float ks = (H0 != 0.0f || H1 != 0.0f || H2 != 0.0f) ? sh.ks : 0.0f;
        norm3(H0, H1, H2);
        const int ns = a.P.max_samples;
        bool probe = true;      // ask the grid only while the ray is in empty space (the last sample's a was 0)
        for (int i = 0; i < ns; ++i) {
            pos[0] = pos[0] + st[0]; pos[1] = pos[1] + st[1]; pos[2] = pos[2] + st[2];
            if (!inside(pos[0], pos[1], pos[2])) break;
            bool own = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) own = own && (pos[k] >= a.P.box_min[k] && pos[k] < a.P.box_max[k]);
            if (!own) continue;
            if (a.sg.g && probe) {
                const uint32_t b = skip_bounds(a.sg, a.t, pos[0], pos[1], pos[2]);
                const int lo = max((int)(b & 255u) - 1, 0), hi = min((int)(b >> 8) + 1, 255);
                if ((int)nextOpaque[lo] > hi) continue;        // every entry the lookup can touch is transparent
            }
            const float smp = sample3d(tex, a, pos[0], pos[1], pos[2]);
            const float x = fminf(fmaxf(smp * 255.0f, 0.0f), 255.0f);
            const int li = min((int)x, 254);
            const float f = x - (float)li;
            const float4 e0 = lut[li], e1 = lut[li + 1];
            float ea = e0.w + f * (e1.w - e0.w);
            ea = fminf(fmaxf(ea, 0.0f), 1.0f);
            float al = ea;
            if (correct) {
                // 1 - (1 - ea)^ex: ea = 0 -> log2(1) = 0 -> exactly 0; ea = 1 -> log2(0) = -inf -> exp2(-inf) = 0 -> 1
                const float p = ex == 0.0f ? 1.0f : exp2f(ex * log2f(1.0f - ea));
                al = 1.0f - p;
            }
            probe = al == 0.0f;
            if (LIT) {
                if (probe) continue;        // a = 0: both updates would be exact no-ops
                float c0 = e0.x + f * (e1.x - e0.x), c1 = e0.y + f * (e1.y - e0.y), c2 = e0.z + f * (e1.z - e0.z);
                const Lattice l = lattice(a.t.GX, a.t.GY, a.t.GZ, pos[0], pos[1], pos[2]);
                float g[3];
                lattice_gradient(gather(tex, a, l), l, g);
                const float m = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
                if (m > sh.gmin) {
                    float N0 = (float)a.t.GX * g[0], N1 = (float)a.t.GY * g[1], N2 = (float)a.t.GZ * g[2];
                    norm3(N0, N1, N2);
                    const float cd = fabsf(N0 * L0 + N1 * L1 + N2 * L2);
                    const float ch = fminf(fmaxf(fabsf(N0 * H0 + N1 * H1 + N2 * H2), 0.00001f), 1.0f);
                    const float kl = sh.ka + sh.kd * cd, sp = ks * powf(ch, sh.shininess);
                    c0 = fminf(1.0f, c0 * kl + sp); c1 = fminf(1.0f, c1 * kl + sp); c2 = fminf(1.0f, c2 * kl + sp);
                }
                const float w = T * al;
                C0 = C0 + w * c0;
                C1 = C1 + w * c1;
                C2 = C2 + w * c2;
            } else {
                const float w = T * al;
                C0 = C0 + w * (e0.x + f * (e1.x - e0.x));
                C1 = C1 + w * (e0.y + f * (e1.y - e0.y));
                C2 = C2 + w * (e0.z + f * (e1.z - e0.z));
            }
            T = T * (1.0f - al);
            if (!a.P.no_early_exit && T < 0.01f) break;
        }
    }
    if (PARTIAL) { o[0] = C0; o[1] = C1; o[2] = C2; o[3] = T; }
    else { o[0] = C0 + T * tf.bg[0]; o[1] = C1 + T * tf.bg[1]; o[2] = C2 + T * tf.bg[2]; o[3] = 1.0f - T; }
}

// ---- two-dimensional transfer functions (vr_raycast_tf2d; the rule is in vrhip.h) ------------------------------------
struct Tf2dArgs {
    const float4 *lut;          // rows x 256 (r, g, b, a), 16-byte aligned, row-major
    const uint16_t *columns;    // vr_tf2d_columns_build of the same table; read only where a skip grid is attached
    int rows;
    float gscale;               // grad_scale
    float unit;
    float bg[3];
};

// columns[k] = the first j >= k at which any row has alpha != 0 at entry j (256: none).  One workgroup of 256 lanes: lane k
// ORs column k over the rows, then walks forward to the first flagged column.
__global__ void __launch_bounds__(256)
k_tf2d_columns(const float4 *__restrict__ lut, int rows, uint16_t *__restrict__ columns)
{
    __shared__ uint8_t opaque[256];
    const int k = threadIdx.x;
    bool any = false;
    for (int j = 0; j < rows; ++j) any = any || lut[(size_t)j * 256 + k].w != 0.0f;
    opaque[k] = any ? 1 : 0;
    __syncthreads();
    int first = k;
    while (first < 256 && !opaque[first]) ++first;
    columns[k] = (uint16_t)first;
}

// k_raycast_tf's march with a table indexed by value and gradient magnitude: a sibling kernel, so k_raycast_tf's
// instantiations keep their registers.  Every fetched sample gathers its lattice gradient (the row needs |g|); the table
// stays in global memory (two 32-byte reads per sample: entries i, i + 1 of rows j, j + 1), only the 512-byte column
// summary is staged, and only when a grid is attached.  A sample the grid bounds by (mn, mx) is skippable when
// columns[max(mn - 1, 0)] > min(mx + 1, 255): every entry of every row the lookup can touch is transparent.
__device__ __forceinline__ bool ray_setup(const RayArgs &a, int px, int py, float pos[3], float st[3]);     // below

template <class SAMPLER, bool LIT, bool PARTIAL>
__global__ void __launch_bounds__(64)
k_raycast_tf2d(RayArgs a, SAMPLER tex, Tf2dArgs tf, ShadeArgs sh)
{
    __shared__ alignas(8) uint16_t columns[256];      // staged as one 8-byte piece per lane
    const int lane = threadIdx.x;
    if (a.sg.g) ((uint2 *)columns)[lane] = ((const uint2 *)tf.columns)[lane];
    __syncthreads();
    // 8x8 pixel tile per wave
    const int px = blockIdx.x * 8 + (lane & 7), py = blockIdx.y * 8 + (lane >> 3);
    const int W = a.P.width, H = a.P.height;
    if (px >= W || py >= H) return;
    float *o = a.out + 4 * ((size_t)py * W + px);
    float C0 = 0.0f, C1 = 0.0f, C2 = 0.0f, T = 1.0f;
    float st[3], pos[3];
    if (ray_setup(a, px, py, pos, st)) {
        // opacity correction exponent L / opacity_unit (0 = none, or L = 0: a = 1 - t^0 = 0)
        const float L = sqrtf(st[0] * st[0] + st[1] * st[1] + st[2] * st[2]);
        const bool correct = tf.unit > 0.0f;
        const float ex = correct ? L / tf.unit : 0.0f;
        // LIT, per ray: V, the light and the half vector; no specular term where L + V = 0.  gd is ray_setup's, formed
        // again from the same operands (pos is still vUV here)
        float gd[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) gd[k] = (pos[k] - 0.5f) - a.cam.pos[k];
        norm3(gd[0], gd[1], gd[2]);
        const float V0 = -gd[0], V1 = -gd[1], V2 = -gd[2];
        const float L0 = sh.head ? V0 : sh.L[0], L1 = sh.head ? V1 : sh.L[1], L2 = sh.head ? V2 : sh.L[2];
        float H0 = L0 + V0, H1 = L1 + V1, H2 = L2 + V2;
        const float ks = (H0 != 0.0f || H1 != 0.0f || H2 != 0.0f) ? sh.ks : 0.0f;
        norm3(H0, H1, H2);
        const float top = (float)(tf.rows - 1);
        const int ns = a.P.max_samples;
        bool probe = true;      // ask the grid only while the ray is in empty space (the last sample's a was 0)
        for (int i = 0; i < ns; ++i) {
            pos[0] = pos[0] + st[0]; pos[1] = pos[1] + st[1]; pos[2] = pos[2] + st[2];
            if (!inside(pos[0], pos[1], pos[2])) break;
            bool own = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) own = own && (pos[k] >= a.P.box_min[k] && pos[k] < a.P.box_max[k]);
            if (!own) continue;
            if (a.sg.g && probe) {
                const uint32_t b = skip_bounds(a.sg, a.t, pos[0], pos[1], pos[2]);
                const int lo = max((int)(b & 255u) - 1, 0), hi = min((int)(b >> 8) + 1, 255);
                if ((int)columns[lo] > hi) continue;        // every entry of every row the lookup can touch is transparent
            }
            const float smp = sample3d(tex, a, pos[0], pos[1], pos[2]);
            const float x = fminf(fmaxf(smp * 255.0f, 0.0f), 255.0f);
            const int li = min((int)x, 254);
            const float f = x - (float)li;
            const Lattice l = lattice(a.t.GX, a.t.GY, a.t.GZ, pos[0], pos[1], pos[2]);
            float g[3];
            lattice_gradient(gather(tex, a, l), l, g);
            const float m = sqrtf(g[0] * g[0] + g[1] * g[1] + g[2] * g[2]);
            const float y = fminf(fmaxf(m * tf.gscale, 0.0f), top);
            const int lj = min((int)y, tf.rows - 2);
            const float h = y - (float)lj;
            const float4 *row = tf.lut + ((size_t)lj * 256 + li);
            const float4 a0 = row[0], a1 = row[1], b0 = row[256], b1 = row[257];
            const float eAa = a0.w + f * (a1.w - a0.w), eBa = b0.w + f * (b1.w - b0.w);
            float ea = eAa + h * (eBa - eAa);
            ea = fminf(fmaxf(ea, 0.0f), 1.0f);
            float al = ea;
            if (correct) {
                // 1 - (1 - ea)^ex: ea = 0 -> log2(1) = 0 -> exactly 0; ea = 1 -> log2(0) = -inf -> exp2(-inf) = 0 -> 1
                const float p = ex == 0.0f ? 1.0f : exp2f(ex * log2f(1.0f - ea));
                al = 1.0f - p;
            }
            probe = al == 0.0f;
            if (probe) continue;        // a = 0: both updates would be exact no-ops
            const float eA0 = a0.x + f * (a1.x - a0.x), eB0 = b0.x + f * (b1.x - b0.x);
            const float eA1 = a0.y + f * (a1.y - a0.y), eB1 = b0.y + f * (b1.y - b0.y);
            const float eA2 = a0.z + f * (a1.z - a0.z), eB2 = b0.z + f * (b1.z - b0.z);
            float c0 = eA0 + h * (eB0 - eA0), c1 = eA1 + h * (eB1 - eA1), c2 = eA2 + h * (eB2 - eA2);
            if (LIT) {
                if (m > sh.gmin) {
                    float N0 = (float)a.t.GX * g[0], N1 = (float)a.t.GY * g[1], N2 = (float)a.t.GZ * g[2];
                    norm3(N0, N1, N2);
                    const float cd = fabsf(N0 * L0 + N1 * L1 + N2 * L2);
                    const float ch = fminf(fmaxf(fabsf(N0 * H0 + N1 * H1 + N2 * H2), 0.00001f), 1.0f);
                    const float kl = sh.ka + sh.kd * cd, sp = ks * powf(ch, sh.shininess);
                    c0 = fminf(1.0f, c0 * kl + sp); c1 = fminf(1.0f, c1 * kl + sp); c2 = fminf(1.0f, c2 * kl + sp);
                }
            }
            const float w = T * al;
            C0 = C0 + w * c0;
            C1 = C1 + w * c1;
            C2 = C2 + w * c2;
            T = T * (1.0f - al);
            if (!a.P.no_early_exit && T < 0.01f) break;
        }
    }
    if (PARTIAL) { o[0] = C0; o[1] = C1; o[2] = C2; o[3] = T; }
    else { o[0] = C0 + T * tf.bg[0]; o[1] = C1 + T * tf.bg[1]; o[2] = C2 + T * tf.bg[2]; o[3] = 1.0f - T; }
}

// ---- colour partials (vr_raycast_tf_partial): one float4 (C.r, C.g, C.b, T) per pixel.  "Over" and the finish are
// written with the marcher's own expressions (C + w c, T t; C + T bg, 1 - T), so a fold of slabs rounds like one march.
struct Bg { float c[3]; };

__device__ __forceinline__ void over_tf(float4 &f, const float4 &b)
{
    f.x = f.x + f.w * b.x;       // (C1 + T1*C2, T1*T2)
    f.y = f.y + f.w * b.y;
    f.z = f.z + f.w * b.z;
    f.w = f.w * b.w;
}
__device__ __forceinline__ float4 finish_tf(const float4 &p, const Bg &bg)
{
    float4 o;
    o.x = p.x + p.w * bg.c[0]; o.y = p.y + p.w * bg.c[1]; o.z = p.z + p.w * bg.c[2]; o.w = 1.0f - p.w;
    return o;
}

// ---- intensity projections (vr_raycast_projection; the rule is in vrhip.h) -------------------------------------------
// A projection partial is (v, n, 0, 0): n owned samples, v their maximum, minimum or float32 sum.  One combine and one
// finish serve the marchers' final store and the compositing kernels (ProjKind), so finish(partial) == frame and
// pairwise folds == the slab call hold by construction.
struct ProjArgs {
    const float4 *lut;      // NULL = grey; else 256 (r, g, b, a), 16-byte aligned
    int op;                 // VR_PROJECT_*
    float lo, hi;           // the window
    float bg[3];
};

__device__ __forceinline__ void combine_proj(float4 &f, const float4 &b, int op)
{
    if (b.y == 0.0f) return;            // a partial that owns no sample
    if (f.y == 0.0f) { f = b; return; }
    f.x = op == VR_PROJECT_MAX ? fmaxf(f.x, b.x) : (op == VR_PROJECT_MIN ? fminf(f.x, b.x) : f.x + b.x);
    f.y = f.y + b.y;
}

__device__ __forceinline__ float4 finish_proj(const float4 &p, const ProjArgs &A)
{
    if (p.y == 0.0f) return make_float4(A.bg[0], A.bg[1], A.bg[2], 0.0f);
    const float m = A.op == VR_PROJECT_MEAN ? p.x / p.y : p.x;
    const float w = fminf(fmaxf((m - A.lo) / (A.hi - A.lo), 0.0f), 1.0f);
    if (!A.lut) return make_float4(w, w, w, 1.0f);
    // step 3 of vr_raycast_tf's rule, with k_raycast_tf's expressions
    const float x = fminf(fmaxf(w * 255.0f, 0.0f), 255.0f);
    const int li = min((int)x, 254);
    const float f = x - (float)li;
    const float4 e0 = A.lut[li], e1 = A.lut[li + 1];
    const float ea = fminf(fmaxf(e0.w + f * (e1.w - e0.w), 0.0f), 1.0f);
    const float c0 = e0.x + f * (e1.x - e0.x), c1 = e0.y + f * (e1.y - e0.y), c2 = e0.z + f * (e1.z - e0.z);
    const float tb = 1.0f - ea;
    return make_float4(ea * c0 + tb * A.bg[0], ea * c1 + tb * A.bg[1], ea * c2 + tb * A.bg[2], ea);
}

// k_raycast's per-pixel ray set-up (the same expressions in the same order): false where the cube does not cover the
// pixel, else pos = vUV and st = the step
__device__ __forceinline__ bool ray_setup(const RayArgs &a, int px, int py, float pos[3], float st[3])
{
    const int W = a.P.width, H = a.P.height;
    const float nx = 2.0f * ((float)px + 0.5f) / (float)W - 1.0f;
    const float ny = 1.0f - 2.0f * ((float)py + 0.5f) / (float)H;
    float dir[3], cp[3] = {a.cam.pos[0], a.cam.pos[1], a.cam.pos[2]};
#pragma unroll
    for (int k = 0; k < 3; ++k) dir[k] = a.f[k] + nx * a.tanX * a.s[k] + ny * a.tanY * a.u[k];
    float t0 = -INFINITY, t1 = INFINITY;
    bool miss = false;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (dir[k] != 0.0f) {
            float lo = (-0.5f - cp[k]) / dir[k], hi = (0.5f - cp[k]) / dir[k];
            if (lo > hi) { float q = lo; lo = hi; hi = q; }
            if (lo > t0) t0 = lo;
            if (hi < t1) t1 = hi;
        } else if (cp[k] < -0.5f || cp[k] > 0.5f) miss = true;
    }
    const float th = t0 >= a.cam.z_near ? t0 : t1;
    if (miss || t0 > t1 || th < a.cam.z_near || th > a.cam.z_far) return false;
    float vuv[3], gd[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) vuv[k] = (cp[k] + th * dir[k]) + 0.5f;
#pragma unroll
    for (int k = 0; k < 3; ++k) gd[k] = (vuv[k] - 0.5f) - cp[k];
    norm3(gd[0], gd[1], gd[2]);
#pragma unroll
    for (int k = 0; k < 3; ++k) { st[k] = gd[k] * a.P.step_size[k]; pos[k] = vuv[k]; }
    return true;
}

// may the fetch at a position whose taps the grid bounds by b = (mn | mx << 8) be dropped?  (the proof is in vrhip.h)
template <int OP>
__device__ __forceinline__ bool proj_skippable(uint32_t b, float cur)
{
    const int mn = (int)(b & 255u), mx = (int)(b >> 8);
    const float k = 1.0f / 255.0f;
    if (OP == VR_PROJECT_MAX) return (float)(mn == mx ? mx : mx + 1) * k <= cur;
    if (OP == VR_PROJECT_MIN) return (float)(mn == mx ? mn : mn - 1) * k >= cur;
    return mx == 0;
}

// One thread per pixel, 8x8 tile per wave; one fetch per iteration (keeping 2 or 4 in flight was tried and measured: no
// gain without the grid, fewer skips with it -- DESIGN.md 3.5f).  The grid is asked while the ray's value stands still
// (after a skip, or a fetch that did not change it; MEAN: a fetch of 0), like k_raycast's probe.
template <class SAMPLER, int OP, bool PARTIAL>
__global__ void __launch_bounds__(64)
k_raycast_proj(RayArgs a, SAMPLER tex, ProjArgs A)
{
    const int px = blockIdx.x * 8 + (threadIdx.x & 7), py = blockIdx.y * 8 + (threadIdx.x >> 3);
    if (px >= a.P.width || py >= a.P.height) return;
    float *o = a.out + 4 * ((size_t)py * a.P.width + px);
    float pos[3], st[3];
    float cur = OP == VR_PROJECT_MIN ? INFINITY : 0.0f;
    int n = 0;
    if (ray_setup(a, px, py, pos, st)) {
        const int ns = a.P.max_samples;
        bool probe = true;
        for (int i = 0; i < ns; ++i) {
            pos[0] = pos[0] + st[0]; pos[1] = pos[1] + st[1]; pos[2] = pos[2] + st[2];
            if (!inside(pos[0], pos[1], pos[2])) break;
            bool own = true;
#pragma unroll
            for (int k = 0; k < 3; ++k) own = own && (pos[k] >= a.P.box_min[k] && pos[k] < a.P.box_max[k]);
            if (!own) continue;
            ++n;
            if (a.sg.g && probe && proj_skippable<OP>(skip_bounds(a.sg, a.t, pos[0], pos[1], pos[2]), cur)) continue;
            const float smp = sample3d(tex, a, pos[0], pos[1], pos[2]);
            if (OP == VR_PROJECT_MEAN) { cur = cur + smp; probe = smp == 0.0f; }
            else {
                const float nv = OP == VR_PROJECT_MAX ? fmaxf(cur, smp) : fminf(cur, smp);
                probe = nv == cur;
                cur = nv;
            }
        }
    }
    const float4 part = n > 0 ? make_float4(cur, (float)n, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 r = PARTIAL ? part : finish_proj(part, A);
    o[0] = r.x; o[1] = r.y; o[2] = r.z; o[3] = r.w;
}

// ---- the three kinds of partial image: identity, fold (front = front then back), finish into a frame, and whether slabs
// fold in the pixel's view order.  A kind carries what its finish needs.
struct GreyKind {       // (c, tau, covered, 0)
    static constexpr bool ordered = true;
    __device__ static float4 identity() { return make_float4(0.0f, 1.0f, 0.0f, 0.0f); }
    __device__ void fold(float4 &f, const float4 &b) const
    {
        f.x = f.x + f.y * b.x;       // (c1 + t1*c2, t1*t2)
        f.y = f.y * b.y;
        f.z = fmaxf(f.z, b.z);
    }
    __device__ float4 finish(const float4 &p) const
    {
        if (p.z > 0.0f) return make_float4(1.0f - p.x, 1.0f - p.x, 1.0f, 1.0f - p.y);      // raycaster.frag:82-85
        return make_float4(1.0f, 1.0f, 1.0f, 1.0f);
    }
};
struct ColourKind {     // (C.r, C.g, C.b, T)
    Bg bg;
    static constexpr bool ordered = true;
    __device__ static float4 identity() { return make_float4(0.0f, 0.0f, 0.0f, 1.0f); }
    __device__ void fold(float4 &f, const float4 &b) const { over_tf(f, b); }
    __device__ float4 finish(const float4 &p) const { return finish_tf(p, bg); }
};
struct ProjKind {       // (v, n, 0, 0); the order only matters to MEAN's rounding
    ProjArgs A;
    static constexpr bool ordered = false;
    __device__ static float4 identity() { return make_float4(0.0f, 0.0f, 0.0f, 0.0f); }
    __device__ void fold(float4 &f, const float4 &b) const { combine_proj(f, b, A.op); }
    __device__ float4 finish(const float4 &p) const { return finish_proj(p, A); }
};

template <class KIND>
__global__ void __launch_bounds__(256)
k_composite_over(KIND kind, float4 *front, const float4 *back, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float4 f = front[i];
    kind.fold(f, back[i]);
    front[i] = f;
}

template <class KIND>
__global__ void __launch_bounds__(256)
k_composite_finish(KIND kind, const float4 *partial, float4 *rgba, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    rgba[i] = kind.finish(partial[i]);
}

struct SlabArgs {
    const float4 *partials;
    int num_slabs;
    int64_t npix, first;
    float4 *out;
    int axis, W, H;         // an ordered kind's frame: pixel i of the call is pixel first + i of W x H
    ViewBasis b;
};

// Pixel i of num_slabs partial images folded front to back and finished: a streaming kernel -- num_slabs 16-byte loads
// and one 16-byte store per lane, consecutive lanes on consecutive pixels.  An ordered kind walks the slabs in the
// order the pixel's ray crosses them: ascending where its direction's component d along the axis is >= 0.
template <class KIND>
__global__ void __launch_bounds__(256)
k_composite_slabs(SlabArgs a, KIND kind)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.npix) return;
    bool ascending = true;
    if constexpr (KIND::ordered) {
        const int64_t gp = a.first + i;
        const int px = (int)(gp % a.W), py = (int)(gp / a.W);
        const float nx = 2.0f * ((float)px + 0.5f) / (float)a.W - 1.0f;
        const float ny = 1.0f - 2.0f * ((float)py + 0.5f) / (float)a.H;
        const float d = a.b.f[a.axis] + nx * a.b.tanX * a.b.s[a.axis] + ny * a.b.tanY * a.b.u[a.axis];
        ascending = d >= 0.0f;
    }
    float4 acc = KIND::identity();
    for (int k = 0; k < a.num_slabs; ++k) {
        const int sidx = ascending ? k : a.num_slabs - 1 - k;
        kind.fold(acc, a.partials[(int64_t)sidx * a.npix + i]);
    }
    a.out[i] = kind.finish(acc);
}

// ---- slice views (vr_reslice; the rule is in vrhip.h) ------------------------------------------------------------------
// a pixel at any float address: four floats stored as one 16-byte word (gfx950 takes unaligned global stores)
struct __attribute__((aligned(4))) Pixel4 { float x, y, z, w; };

#define RESLICE_TILE_LOG2 4    // the wave's tile is 16 x 4 pixels (measured: DESIGN.md 3.5g)
struct SliceArgs {
    Tex t;                  // the dense volume
    int W, H, layers;
    int ltw;                // log2 of the wave's tile width: lane l is pixel (l & (tw - 1), l >> ltw) of a tw x 64 / tw tile
    float o[3], du[3], dv[3], dw[3], bmin[3], bmax[3];
    float *out;
};

// the voxel a position falls into, as a float: global index clamped, then located like a tap of tex3d
__device__ __forceinline__ float nearest3d(const DenseSampler &, const Tex &t, float px, float py, float pz)
{
    const int gx = clampi((int)floorf(px * (float)t.GX), 0, t.GX - 1), gy = clampi((int)floorf(py * (float)t.GY), 0, t.GY - 1),
              gz = clampi((int)floorf(pz * (float)t.GZ), 0, t.GZ - 1);
    const int x = clampi(gx - t.ox, 0, t.X - 1), y = clampi(gy - t.oy, 0, t.Y - 1), z = clampi(gz - t.oz, 0, t.Z - 1);
    return (float)t.v[x + (int64_t)t.X * (y + (int64_t)t.Y * z)] * (1.0f / 255.0f);
}
__device__ __forceinline__ float linear3d(const DenseSampler &, const Tex &t, float x, float y, float z) { return tex3d(t, x, y, z); }

// One thread per pixel, the layers looped inside the thread; every position is formed from the pixel and layer indices
// alone.  The wave's footprint is a launch parameter (slice_launch picks it; DESIGN.md 3.5g has the measurements).
template <class SAMPLER, int OP, int FILTER, bool PARTIAL>
__global__ void __launch_bounds__(64)
k_reslice(SliceArgs a, SAMPLER tex, ProjArgs A)
{
    const int lane = threadIdx.x;
    const int px = (int)(blockIdx.x << a.ltw) + (lane & ((1 << a.ltw) - 1)), py = (int)(blockIdx.y << (6 - a.ltw)) + (lane >> a.ltw);
    if (px >= a.W || py >= a.H) return;
    float base[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) base[k] = (a.o[k] + (float)px * a.du[k]) + (float)py * a.dv[k];
    float cur = OP == VR_PROJECT_MIN ? INFINITY : 0.0f;
    int n = 0;
    for (int l = 0; l < a.layers; ++l) {
        float pos[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) pos[k] = base[k] + (float)l * a.dw[k];
        if (!inside(pos[0], pos[1], pos[2])) continue;
        bool own = true;
#pragma unroll
        for (int k = 0; k < 3; ++k) own = own && (pos[k] >= a.bmin[k] && pos[k] < a.bmax[k]);
        if (!own) continue;
        ++n;
        const float smp = FILTER == VR_SLICE_LINEAR ? linear3d(tex, a.t, pos[0], pos[1], pos[2])
                                                    : nearest3d(tex, a.t, pos[0], pos[1], pos[2]);
        cur = OP == VR_PROJECT_MEAN ? cur + smp : (OP == VR_PROJECT_MAX ? fmaxf(cur, smp) : fminf(cur, smp));
    }
    const float4 part = n > 0 ? make_float4(cur, (float)n, 0.0f, 0.0f) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float4 r = PARTIAL ? part : finish_proj(part, A);
    *(Pixel4 *)(a.out + 4 * ((size_t)py * a.W + px)) = Pixel4{r.x, r.y, r.z, r.w};
}

// Brick <-> global volume placement (VolumeReader.h:172-211), 16-byte rows segments: one vector copy each where both
// buffers start 16-byte aligned, sixteen byte copies otherwise (offset views of a caller's allocation).
template <bool TO_VOLUME, bool ALIGNED>
__global__ void __launch_bounds__(256)
k_assemble(const uint8_t *src, uint8_t *dst, int nbricks, int64_t X, int64_t Y, int64_t Z, const int64_t *ijk,
           int64_t I, int64_t J)
{
    const int b = blockIdx.y;
    const int64_t xv = X / 16;                     // 16-byte vectors per row
    const int64_t total = xv * Y * Z;
    const int64_t i = ijk[3 * b], j = ijk[3 * b + 1], k = ijk[3 * b + 2];
    const int64_t GX = X * I, GY = Y * J;
    for (int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < total; q += (int64_t)gridDim.x * blockDim.x) {
        int64_t xq = q % xv, y = (q / xv) % Y, z = q / (xv * Y);
        int64_t bo = (int64_t)b * X * Y * Z + xq * 16 + X * (y + Y * z);
        int64_t go = (i * X + xq * 16) + GX * ((j * Y + y) + GY * (k * Z + z));
        const int64_t so = TO_VOLUME ? bo : go, doff = TO_VOLUME ? go : bo;
        if (ALIGNED) *(uint4 *)(dst + doff) = *(const uint4 *)(src + so);
        else {
#pragma unroll
            for (int c = 0; c < 16; ++c) dst[doff + c] = src[so + c];
        }
    }
}

__global__ void __launch_bounds__(256)
k_measure_error(const uint8_t *a, const uint8_t *b, int64_t n, int *maxErr, unsigned long long *sumErr)
{
    int m = 0;
    unsigned long long s = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int e = (int)a[i] - (int)b[i];
        e = e < 0 ? -e : e;
        m = e > m ? e : m;
        s += (unsigned)e;
    }
    for (int o = 32; o > 0; o >>= 1) { int u = __shfl_xor(m, o); m = u > m ? u : m; s += __shfl_xor(s, o); }
    if ((threadIdx.x & 63) == 0) { if (m) atomicMax(maxErr, m); if (s) atomicAdd(sumErr, s); }
}

__global__ void __launch_bounds__(256)
k_query_error(const uint8_t *a, const uint8_t *b, int64_t n, uint8_t *out)
{
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        int e = (int)a[i] - (int)b[i];
        out[i] = (uint8_t)(e < 0 ? -e : e);
    }
}

static void cross3(const float *a, const float *b, float *o)
{
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}
static void hnorm3(float *v)
{
    float l = sqrtf(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
    if (l > 0.0f) { v[0] /= l; v[1] /= l; v[2] /= l; } else { v[0] = v[1] = v[2] = 0.0f; }
}

// the frame's basis (raymarch.h): these float operations, in this order, for everything that needs it
ViewBasis view_basis(const vr_camera *cam, int width, int height)
{
    ViewBasis b;
    for (int k = 0; k < 3; ++k) b.f[k] = cam->front[k];
    hnorm3(b.f);
    cross3(b.f, cam->up, b.s);
    hnorm3(b.s);
    cross3(b.s, b.f, b.u);
    const float rad = cam->fov_deg * 0.01745329251994329576923690768489f;
    b.tanY = tanf(0.5f * rad);
    b.tanX = b.tanY * (float)width / (float)height;
    return b;
}

// the camera, the parameters, the frame's basis and the output
static void ray_frame(RayArgs &a, const vr_camera *cam, const vr_render_params *P, float *rgba)
{
    a.cam = *cam;
    a.P = *P;
    const ViewBasis b = view_basis(cam, P->width, P->height);
    for (int k = 0; k < 3; ++k) { a.f[k] = b.f[k]; a.s[k] = b.s[k]; a.u[k] = b.u[k]; }
    a.tanX = b.tanX; a.tanY = b.tanY;
    a.out = rgba;
}

// the dense volume's texture and skip grid
static void dense_args(RayArgs &a, const uint8_t *vol, const int64_t dims[3], const vr_render_params *P)
{
    a.t.v = vol;
    a.t.X = (int)dims[0]; a.t.Y = (int)dims[1]; a.t.Z = (int)dims[2];
    a.t.GX = P->global_dims[0] > 0 ? (int)P->global_dims[0] : a.t.X;
    a.t.GY = P->global_dims[1] > 0 ? (int)P->global_dims[1] : a.t.Y;
    a.t.GZ = P->global_dims[2] > 0 ? (int)P->global_dims[2] : a.t.Z;
    a.t.ox = (int)P->vol_origin[0]; a.t.oy = (int)P->vol_origin[1]; a.t.oz = (int)P->vol_origin[2];
    a.sg.g = nullptr; a.sg.S = 1; a.sg.nx = a.sg.ny = a.sg.nz = 0;
    // the grid describes volume_dev as a whole: only used where the local volume IS the texture (single-GPU path)
    if (P->skip_grid_dev && P->skip_cell > 0 && a.t.GX == a.t.X && a.t.GY == a.t.Y && a.t.GZ == a.t.Z && a.t.ox == 0 && a.t.oy == 0 && a.t.oz == 0) {
        a.sg.g = P->skip_grid_dev; a.sg.S = P->skip_cell;
        a.sg.nx = (a.t.X + a.sg.S - 1) / a.sg.S; a.sg.ny = (a.t.Y + a.sg.S - 1) / a.sg.S; a.sg.nz = (a.t.Z + a.sg.S - 1) / a.sg.S;
    }
}

static int ilog2(int64_t v) { int n = 0; while (((int64_t)1 << n) < v) ++n; return n; }

// a pool's virtual volume (its extents in a.t), sampler and skip grid
static PoolTex pool_args(RayArgs &a, const uint8_t *pool, const vr_pool_entry *tab, const int64_t bd[3], const int64_t grid[3],
                         const vr_render_params *P)
{
    a.t.v = nullptr;
    a.t.X = a.t.GX = (int)(grid[0] * bd[0]); a.t.Y = a.t.GY = (int)(grid[1] * bd[1]); a.t.Z = a.t.GZ = (int)(grid[2] * bd[2]);
    a.t.ox = a.t.oy = a.t.oz = 0;
    a.sg.g = nullptr; a.sg.S = 1; a.sg.nx = a.sg.ny = a.sg.nz = 0;
    if (P->skip_grid_dev && P->skip_cell > 0) {     // a grid of the whole virtual volume
        a.sg.g = P->skip_grid_dev; a.sg.S = P->skip_cell;
        a.sg.nx = (a.t.X + a.sg.S - 1) / a.sg.S; a.sg.ny = (a.t.Y + a.sg.S - 1) / a.sg.S; a.sg.nz = (a.t.Z + a.sg.S - 1) / a.sg.S;
    }
    PoolTex pt;
    pt.pool = pool; pt.tab = tab;
    pt.lx = ilog2(bd[0]); pt.ly = ilog2(bd[1]); pt.lz = ilog2(bd[2]);
    pt.gx = (int)grid[0]; pt.gy = (int)grid[1];
    return pt;
}

static TfArgs tf_args(const vr_transfer_function *tf)
{
    TfArgs t;
    t.lut = (const float4 *)tf->lut_dev;
    t.unit = tf->opacity_unit;
    for (int k = 0; k < 3; ++k) t.bg[k] = tf->background[k];
    return t;
}

// the lighting constants; a non-zero light_dir is normalized in double (a tiny one stays a direction)
static ShadeArgs shade_args(const vr_shading *sh)
{
    ShadeArgs s;
    s.ka = sh->ambient; s.kd = sh->diffuse; s.ks = sh->specular; s.shininess = sh->shininess; s.gmin = sh->grad_min;
    const double l[3] = {sh->light_dir[0], sh->light_dir[1], sh->light_dir[2]};
    const double n = sqrt(l[0] * l[0] + l[1] * l[1] + l[2] * l[2]);
    s.head = n > 0.0 ? 0 : 1;
    for (int k = 0; k < 3; ++k) s.L[k] = n > 0.0 ? (float)(l[k] / n) : 0.0f;
    return s;
}

// The frame of a through k_raycast (no table), k_raycast_tf (a table) or its lit instantiation (a table and lighting);
// label[style] names the launch in errors.  partial (a table only): the colour partial instead of the frame.
template <class SAMPLER>
static int march_launch(const RayArgs &a, const SAMPLER &tex, const vr_transfer_function *tf, const vr_shading *sh,
                        bool partial, const char *const label[3], hipStream_t st)
{
    const dim3 grid((a.P.width + 7) / 8, (a.P.height + 7) / 8);
    if (!tf) hipLaunchKernelGGL(k_raycast<SAMPLER>, grid, dim3(64), 0, st, a, tex);
    else if (!sh) {
        auto kern = partial ? k_raycast_tf<SAMPLER, false, true> : k_raycast_tf<SAMPLER, false, false>;
        hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, a, tex, tf_args(tf), ShadeArgs());
    } else {
        auto kern = partial ? k_raycast_tf<SAMPLER, true, true> : k_raycast_tf<SAMPLER, true, false>;
        hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, a, tex, tf_args(tf), shade_args(sh));
    }
    return launch_status(label[!tf ? 0 : (!sh ? 1 : 2)]);
}

int raycast_launch(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                   const vr_transfer_function *tf, const vr_shading *sh, bool partial, float *rgba, hipStream_t st)
{
    static const char *const label[3] = {"raymarch", "raymarch_tf", "raymarch_tf_shaded"};
    RayArgs a;
    dense_args(a, vol, dims, P);
    ray_frame(a, cam, P, rgba);
    return march_launch(a, DenseSampler(), tf, sh, partial, label, st);
}

int raycast_pool_launch(const uint8_t *pool, const vr_pool_entry *tab, const int64_t bd[3], const int64_t grid[3],
                        const vr_camera *cam, const vr_render_params *P, const vr_transfer_function *tf, const vr_shading *sh,
                        bool partial, float *rgba, hipStream_t st)
{
    static const char *const label[3] = {"raymarch_pool", "raymarch_pool_tf", "raymarch_pool_tf_shaded"};
    RayArgs a;
    const PoolTex pt = pool_args(a, pool, tab, bd, grid, P);
    ray_frame(a, cam, P, rgba);
    return march_launch(a, pt, tf, sh, partial, label, st);
}

// the frame (or colour partial) of a through k_raycast_tf2d, lit where sh is given
template <class SAMPLER>
static int march2d_launch(const RayArgs &a, const SAMPLER &tex, const vr_transfer_function2d *tf, const vr_shading *sh,
                          bool partial, const char *label, hipStream_t st)
{
    Tf2dArgs t;
    t.lut = (const float4 *)tf->lut_dev;
    t.columns = tf->columns_dev;
    t.rows = tf->rows;
    t.gscale = tf->grad_scale;
    t.unit = tf->opacity_unit;
    for (int k = 0; k < 3; ++k) t.bg[k] = tf->background[k];
    const dim3 grid((a.P.width + 7) / 8, (a.P.height + 7) / 8);
    if (!sh) {
        auto kern = partial ? k_raycast_tf2d<SAMPLER, false, true> : k_raycast_tf2d<SAMPLER, false, false>;
        hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, a, tex, t, ShadeArgs());
    } else {
        auto kern = partial ? k_raycast_tf2d<SAMPLER, true, true> : k_raycast_tf2d<SAMPLER, true, false>;
        hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, a, tex, t, shade_args(sh));
    }
    return launch_status(label);
}

int raycast_tf2d_launch(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                        const vr_transfer_function2d *tf, const vr_shading *sh, bool partial, float *rgba, hipStream_t st)
{
    RayArgs a;
    dense_args(a, vol, dims, P);
    ray_frame(a, cam, P, rgba);
    return march2d_launch(a, DenseSampler(), tf, sh, partial, "raymarch_tf2d", st);
}

int raycast_pool_tf2d_launch(const uint8_t *pool, const vr_pool_entry *tab, const int64_t bd[3], const int64_t grid[3],
                             const vr_camera *cam, const vr_render_params *P, const vr_transfer_function2d *tf,
                             const vr_shading *sh, bool partial, float *rgba, hipStream_t st)
{
    RayArgs a;
    const PoolTex pt = pool_args(a, pool, tab, bd, grid, P);
    ray_frame(a, cam, P, rgba);
    return march2d_launch(a, pt, tf, sh, partial, "raymarch_pool_tf2d", st);
}

int tf2d_columns_launch(const float *lut, int rows, uint16_t *columns, hipStream_t st)
{
    hipLaunchKernelGGL(k_tf2d_columns, dim3(1), dim3(256), 0, st, (const float4 *)lut, rows, columns);
    return launch_status("tf2d_columns");
}

// k_skip_grid over a pool's virtual volume: the same cells, rows and bounds; a row's voxels come from the stored voxels of
// the bricks it crosses (a table load where it enters one)
__global__ void __launch_bounds__(256)
k_skip_grid_pool(PoolTex p, int X, int Y, int Z, int S, int nx, int ny, int nz, uint8_t *__restrict__ grid)
{
    const int64_t cell = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (cell >= (int64_t)nx * ny * nz) return;
    const int cx = (int)(cell % nx), cy = (int)((cell / nx) % ny), cz = (int)(cell / ((int64_t)nx * ny));
    const int x0 = cx * S, y0 = cy * S, z0 = cz * S;
    const int ex = min(S + 1, X - x0), ey = min(S + 1, Y - y0), ez = min(S + 1, Z - z0);
    uint32_t mn = 255, mx = 0;
    for (int r = lane; r < ey * ez; r += 64) {
        const int y = y0 + r % ey, z = z0 + r / ey;
        int i = 0;
        while (i < ex) {
            const int x = x0 + i, bx = x >> p.lx;
            const int end = min(ex, ((bx + 1) << p.lx) - x0);       // the row's voxels in this brick
            const PoolCell c = pool_cell(p, bx, y >> p.ly, z >> p.lz);
            if (c.off < 0) { mn = 0; i = end; continue; }
            const uint8_t *row = p.pool + pool_at(p, c, x, y, z) - ((x & ((1 << p.lx) - 1)) >> c.sx);
            for (; i < end; ++i) {
                const uint32_t v = row[((x0 + i) & ((1 << p.lx) - 1)) >> c.sx];
                mn = min(mn, v); mx = max(mx, v);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { mn = min(mn, (uint32_t)__shfl_xor((int)mn, o)); mx = max(mx, (uint32_t)__shfl_xor((int)mx, o)); }
    if (lane == 0) { grid[2 * cell] = (uint8_t)mn; grid[2 * cell + 1] = (uint8_t)mx; }
}

int skip_grid_pool_launch(const uint8_t *pool, const vr_pool_entry *tab, const int64_t bd[3], const int64_t grid[3], int S,
                          uint8_t *out, hipStream_t st)
{
    PoolTex pt;
    pt.pool = pool; pt.tab = tab;
    pt.lx = ilog2(bd[0]); pt.ly = ilog2(bd[1]); pt.lz = ilog2(bd[2]);
    pt.gx = (int)grid[0]; pt.gy = (int)grid[1];
    const int X = (int)(grid[0] * bd[0]), Y = (int)(grid[1] * bd[1]), Z = (int)(grid[2] * bd[2]);
    const int nx = (X + S - 1) / S, ny = (Y + S - 1) / S, nz = (Z + S - 1) / S;
    const int64_t cells = (int64_t)nx * ny * nz;
    hipLaunchKernelGGL(k_skip_grid_pool, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, st, pt, X, Y, Z, S, nx, ny, nz, out);
    return launch_status("skip_grid_pool");
}

// process-wide debugging switch (vr_debug_set("skip_grid_v1", 1), or VRHIP_SKIP_GRID_V1 in the environment when the
// library is first used): the one-wave-per-cell kernel for every grid
std::atomic<int> g_skipGridV1{-1};

int skip_grid_launch(const uint8_t *vol, const int64_t dims[3], int S, uint8_t *grid, hipStream_t st)
{
    int v1 = g_skipGridV1.load(std::memory_order_relaxed);
    if (v1 < 0) { v1 = getenv("VRHIP_SKIP_GRID_V1") ? 1 : 0; g_skipGridV1.store(v1, std::memory_order_relaxed); }
    // k_skip_grid8 loads 16 bytes per lane and stores (min, max) pairs as 32-bit words: an offset sub-buffer of a
    // caller's allocation goes through the byte-wise kernel
    const int nx = (int)((dims[0] + S - 1) / S), ny = (int)((dims[1] + S - 1) / S), nz = (int)((dims[2] + S - 1) / S);
    const int64_t cells = (int64_t)nx * ny * nz;
    const bool aligned = (((uintptr_t)vol & 15u) == 0u) && (((uintptr_t)grid & 3u) == 0u);
    if (S == 8 && (dims[0] & 127) == 0 && !v1 && aligned) {
        const int64_t strips = (dims[0] >> 7) * (int64_t)ny * nz;
        hipLaunchKernelGGL(k_skip_grid8, dim3((unsigned)((strips + 3) / 4)), dim3(256), 0, st, vol, (int)dims[0], (int)dims[1],
                           (int)dims[2], nx, ny, nz, grid);
        return launch_status("skip_grid");
    }
    hipLaunchKernelGGL(k_skip_grid, dim3((unsigned)((cells + 3) / 4)), dim3(256), 0, st, vol, (int)dims[0], (int)dims[1], (int)dims[2], S,
                       nx, ny, nz, grid, ((uintptr_t)vol & 7u) == 0u);
    return launch_status("skip_grid");
}

static ProjArgs proj_args(const vr_projection *pj)
{
    ProjArgs A;
    A.lut = (const float4 *)pj->lut_dev;
    A.op = pj->op;
    A.lo = pj->window_lo; A.hi = pj->window_hi;
    for (int k = 0; k < 3; ++k) A.bg[k] = pj->background[k];
    return A;
}

template <class SAMPLER, int OP>
static void proj_launch_op(const RayArgs &a, const SAMPLER &tex, const ProjArgs &A, bool partial, hipStream_t st)
{
    const dim3 grid((a.P.width + 7) / 8, (a.P.height + 7) / 8);
    auto kern = partial ? k_raycast_proj<SAMPLER, OP, true> : k_raycast_proj<SAMPLER, OP, false>;
    hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, a, tex, A);
}
template <class SAMPLER>
static int proj_launch(const RayArgs &a, const SAMPLER &tex, const vr_projection *pj, bool partial, const char *label, hipStream_t st)
{
    const ProjArgs A = proj_args(pj);
    if (pj->op == VR_PROJECT_MAX) proj_launch_op<SAMPLER, VR_PROJECT_MAX>(a, tex, A, partial, st);
    else if (pj->op == VR_PROJECT_MIN) proj_launch_op<SAMPLER, VR_PROJECT_MIN>(a, tex, A, partial, st);
    else proj_launch_op<SAMPLER, VR_PROJECT_MEAN>(a, tex, A, partial, st);
    return launch_status(label);
}

int raycast_proj_launch(const uint8_t *vol, const int64_t dims[3], const vr_camera *cam, const vr_render_params *P,
                        const vr_projection *pj, bool partial, float *rgba, hipStream_t st)
{
    RayArgs a;
    dense_args(a, vol, dims, P);
    ray_frame(a, cam, P, rgba);
    return proj_launch(a, DenseSampler(), pj, partial, "raymarch_proj", st);
}

int raycast_pool_proj_launch(const uint8_t *pool, const vr_pool_entry *tab, const int64_t bd[3], const int64_t grid[3],
                             const vr_camera *cam, const vr_render_params *P, const vr_projection *pj, bool partial, float *rgba,
                             hipStream_t st)
{
    RayArgs a;
    const PoolTex pt = pool_args(a, pool, tab, bd, grid, P);
    ray_frame(a, cam, P, rgba);
    return proj_launch(a, pt, pj, partial, "raymarch_pool_proj", st);
}

// ---- the compositing launches: a PartialKind (raymarch.h) picks the instantiation
static const char *const kCompositeLabel[3][3] = {{"raymarch", "raymarch", "composite_slabs"},
                                                  {"composite_over_tf", "composite_finish_tf", "composite_slabs_tf"},
                                                  {"composite_combine_proj", "composite_finish_proj", "composite_slabs_proj"}};

// launch(kind) with the device struct of k
template <class F>
static void with_kind(const PartialKind &k, F &&launch)
{
    if (k.which == PartialKind::GREY) launch(GreyKind());
    else if (k.which == PartialKind::COLOUR) {
        ColourKind c = {};      // a fold comes without tf: it does not read the background
        if (k.tf) for (int q = 0; q < 3; ++q) c.bg.c[q] = k.tf->background[q];
        launch(c);
    } else launch(ProjKind{proj_args(k.proj)});
}

int composite_over_launch(const PartialKind &k, float *front, const float *back, int64_t n, hipStream_t st)
{
    with_kind(k, [&](auto kind) {
        hipLaunchKernelGGL(k_composite_over<decltype(kind)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kind,
                           (float4 *)front, (const float4 *)back, n);
    });
    return launch_status(kCompositeLabel[k.which][0]);
}
int composite_finish_launch(const PartialKind &k, const float *partial, float *rgba, int64_t n, hipStream_t st)
{
    with_kind(k, [&](auto kind) {
        hipLaunchKernelGGL(k_composite_finish<decltype(kind)>, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, kind,
                           (const float4 *)partial, (float4 *)rgba, n);
    });
    return launch_status(kCompositeLabel[k.which][1]);
}
int composite_slabs_launch(const PartialKind &k, const float *partials, int nslabs, int64_t npix, int64_t first, int axis,
                           const vr_camera *cam, const vr_render_params *P, float *rgba, hipStream_t st)
{
    with_kind(k, [&](auto kind) {
        SlabArgs a = {(const float4 *)partials, nslabs, npix, first, (float4 *)rgba};
        if (decltype(kind)::ordered) {
            a.axis = axis; a.W = P->width; a.H = P->height;
            a.b = view_basis(cam, P->width, P->height);
        }
        hipLaunchKernelGGL(k_composite_slabs<decltype(kind)>, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, a, kind);
    });
    return launch_status(kCompositeLabel[k.which][2]);
}

// process-wide debugging switch (vr_debug_set("reslice_tile_w", 8 | 16 | 64)): the width of the wave's pixel tile in
// k_reslice, for profiles/tools/slice_bench.py; results do not depend on it
std::atomic<int> g_resliceTileLog2{RESLICE_TILE_LOG2};

static void slice_args(SliceArgs &a, const vr_slice_plane *pl, float *out)
{
    a.W = pl->width; a.H = pl->height; a.layers = pl->layers;
    a.ltw = g_resliceTileLog2.load(std::memory_order_relaxed);
    for (int k = 0; k < 3; ++k) {
        a.o[k] = pl->origin[k]; a.du[k] = pl->du[k]; a.dv[k] = pl->dv[k]; a.dw[k] = pl->dw[k];
        a.bmin[k] = pl->box_min[k]; a.bmax[k] = pl->box_max[k];
    }
    a.out = out;
}

template <class SAMPLER, int OP, int FILTER>
static void slice_launch_of(const SliceArgs &a, const SAMPLER &tex, const ProjArgs &A, bool partial, hipStream_t st)
{
    const int tw = 1 << a.ltw, th = 64 >> a.ltw;
    const dim3 grid((a.W + tw - 1) / tw, (a.H + th - 1) / th);
    auto kern = partial ? k_reslice<SAMPLER, OP, FILTER, true> : k_reslice<SAMPLER, OP, FILTER, false>;
    hipLaunchKernelGGL(kern, grid, dim3(64), 0, st, a, tex, A);
}
template <class SAMPLER, int OP>
static void slice_launch_op(const SliceArgs &a, const SAMPLER &tex, const ProjArgs &A, int filter, bool partial, hipStream_t st)
{
    if (filter == VR_SLICE_LINEAR) slice_launch_of<SAMPLER, OP, VR_SLICE_LINEAR>(a, tex, A, partial, st);
    else slice_launch_of<SAMPLER, OP, VR_SLICE_NEAREST>(a, tex, A, partial, st);
}
template <class SAMPLER>
static int slice_launch(const SliceArgs &a, const SAMPLER &tex, const vr_slice_plane *pl, const vr_projection *pj, bool partial,
                        const char *label, hipStream_t st)
{
    const ProjArgs A = proj_args(pj);
    if (pj->op == VR_PROJECT_MAX) slice_launch_op<SAMPLER, VR_PROJECT_MAX>(a, tex, A, pl->filter, partial, st);
    else if (pj->op == VR_PROJECT_MIN) slice_launch_op<SAMPLER, VR_PROJECT_MIN>(a, tex, A, pl->filter, partial, st);
    else slice_launch_op<SAMPLER, VR_PROJECT_MEAN>(a, tex, A, pl->filter, partial, st);
    return launch_status(label);
}

// the texture of a slice: dense_args lays it out from render params; a plane carries the same two fields
static vr_render_params plane_params(const vr_slice_plane *pl)
{
    vr_render_params P = {};
    for (int k = 0; k < 3; ++k) { P.global_dims[k] = pl->global_dims[k]; P.vol_origin[k] = pl->vol_origin[k]; }
    return P;
}

int reslice_launch(const uint8_t *vol, const int64_t dims[3], const vr_slice_plane *pl, const vr_projection *pj, bool partial,
                   float *out, hipStream_t st)
{
    RayArgs r;
    const vr_render_params P = plane_params(pl);
    dense_args(r, vol, dims, &P);
    SliceArgs a;
    a.t = r.t;
    slice_args(a, pl, out);
    return slice_launch(a, DenseSampler(), pl, pj, partial, "reslice", st);
}

int assemble_launch(bool toVolume, const uint8_t *src, uint8_t *dst, int nb, const int64_t bd[3], const int64_t *ijkDev,
                    const int64_t grid[3], hipStream_t st)
{
    int64_t total = bd[0] / 16 * bd[1] * bd[2];
    unsigned gx = (unsigned)((total + 255) / 256);
    if (gx > 4096) gx = 4096;
    const bool aligned = (((uintptr_t)src | (uintptr_t)dst) & 15u) == 0u;
    auto kern = toVolume ? (aligned ? k_assemble<true, true> : k_assemble<true, false>)
                         : (aligned ? k_assemble<false, true> : k_assemble<false, false>);
    hipLaunchKernelGGL(kern, dim3(gx, nb), dim3(256), 0, st, src, dst, nb, bd[0], bd[1], bd[2], ijkDev, grid[0], grid[1]);
    return launch_status("raymarch");
}
int measure_error_launch(const uint8_t *a, const uint8_t *b, int64_t n, int *maxErrDev, unsigned long long *sumDev,
                         hipStream_t st)
{
    unsigned g = (unsigned)((n + 255) / 256);
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(k_measure_error, dim3(g), dim3(256), 0, st, a, b, n, maxErrDev, sumDev);
    return launch_status("raymarch");
}
int query_error_launch(const uint8_t *a, const uint8_t *b, int64_t n, uint8_t *out, hipStream_t st)
{
    unsigned g = (unsigned)((n + 255) / 256);
    if (g > 2048) g = 2048;
    hipLaunchKernelGGL(k_query_error, dim3(g), dim3(256), 0, st, a, b, n, out);
    return launch_status("raymarch");
}

} // namespace vr
