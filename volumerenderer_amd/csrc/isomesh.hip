// isomesh.hip -- the iso-surface of a dense volume as an indexed triangle mesh (vrhip.h "iso-surface meshes"):
// vr_isomesh_workspace_bytes, vr_isomesh_count and vr_isomesh_emit, at the end of the file.  The rule -- lattice, inside
// test, the six Kuhn tetrahedra of a cell, edge vertices, winding, ownership and order -- is stated in vrhip.h; this file
// only says how it is computed.
//
// The shape is count -> scan -> emit over the lattice POINTS of the own point box [own_lo, own_hi], x fastest:
// point n = px + PX (py + PY pz).  A RUN is 64 consecutive points, taken by one wave (a run may cross the end of a row;
// within a row the lanes' byte loads are contiguous); the waves of a bounded grid walk the runs with a grid stride.
// A lane loads the 8 corners of the cube whose low corner is its point (a corner beyond own_hi is not loaded: its edges
// and its cell are not the call's), forms the 8-bit inside mask, from it the 7-bit mask of the crossing edges the point
// owns and, where the cell is owned, the cell's triangle count (0, 1 or 2 per tetrahedron).
//
//   k_mesh_count   per point the 16-bit word (prefix << 7) | mask -- prefix = the vertices of the run's earlier points,
//                  at most 63 * 7 -- and per run the two totals (vertices <= 448, triangles <= 768), 32 bits each.
//   k_mesh_scan1   one workgroup per 1024 runs: the totals become exclusive prefixes within the 1024, the sums of the
//                  1024 go to a second level of 64-bit pairs.
//   k_mesh_scan2   one workgroup scans the second level with a 64-bit carry and leaves the two grand totals.
//   k_mesh_add     adds each run its second-level prefix (the low 32 bits: counts beyond 2^32 - 1 are refused).
//   k_mesh_emit    recomputes the classification and the in-run prefixes; writes the positions (and gradients) of the
//                  point's vertices at base(run) + prefix, and for an owned cell its triangles' indices at
//                  base(run) + prefix: a corner (owner point, edge type e) is the owner's base + prefix + the number of
//                  mask bits below e, the owner's word and run base looked up in the workspace.
//
// In-wave prefixes are ballots: a count of b bits takes b ballots and popcounts, no LDS and no cross-lane moves.
// No atomics anywhere: every address is fixed by the scans, which is also why the output is the same on every call.
// Stores: every output store is guarded by the num_vertices / num_triangles the caller passed; every workspace index is
// below the sizes vr_isomesh_workspace_bytes derives from the same desc; every volume index is inside the held voxels by
// the entry points' checks.
#include "brickset.h"
#include "raymarch.h"
#include <algorithm>
#include <cmath>

namespace vr {

std::atomic<int> g_meshCountOnly{0};

constexpr int M_THREADS = 256, M_WAVES = M_THREADS / 64;
constexpr int M_SCAN_RUNS = 1024;              // runs per workgroup of the first scan level: 4 per thread
constexpr int M_TOP_THREADS = 1024;
// The per-point kernels walk the runs with a grid stride from at most this many workgroups: a launch cannot have 2^32
// threads or more, and the bench volume alone has 2^33 points.
constexpr int64_t M_MAX_GRID = 65536;
static_assert(63 * 7 < (1 << 9), "a point's in-run vertex prefix fits 9 bits beside the 7-bit mask");
static_assert(M_SCAN_RUNS == 4 * M_THREADS, "four runs per thread");

// ---- the triangles of a tetrahedron: 6 permutations x 16 inside masks -------------------------------------------------
// Entry: bits 0-1 the number of triangles, then six 6-bit corner codes from bit 4 on (two triangles of three corners);
// a corner code is (owner corner of the cell, 3 bits: dx + 2 dy + 4 dz) | (edge type e << 3).  The winding is worked
// out here from the geometry, every edge vertex at its midpoint (coordinates doubled to stay integer): the normal
// cross(b - a, c - a) must point away from an inside corner.
struct TetTable { uint64_t e[96]; };
constexpr int TET_A1[6] = {1, 1, 2, 2, 4, 4}, TET_A2[6] = {3, 5, 3, 6, 5, 6};      // xyz xzy yxz yzx zxy zyx

constexpr TetTable make_tet_table()
{
    TetTable T{};
    for (int p = 0; p < 6; ++p)
        for (int m = 0; m < 16; ++m) {
            const int c[4] = {0, TET_A1[p], TET_A2[p], 7};
            int in[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0}, ni = 0, no = 0;
            for (int i = 0; i < 4; ++i) {
                if ((m >> i) & 1) in[ni++] = i;
                else out[no++] = i;
            }
            int tri[6][2] = {{0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}, {0, 0}}, nt = 0;
            if (ni == 1 || ni == 3) {
                const int i = ni == 1 ? in[0] : out[0];
                int k = 0;
                for (int j = 0; j < 4; ++j)
                    if (j != i) { tri[k][0] = i < j ? i : j; tri[k][1] = i < j ? j : i; ++k; }
                nt = 1;
            } else if (ni == 2) {
                const int q[4][2] = {{in[0], out[0]}, {in[0], out[1]}, {in[1], out[1]}, {in[1], out[0]}};
                const int order[6] = {0, 1, 2, 0, 2, 3};
                for (int k = 0; k < 6; ++k) {
                    const int a = q[order[k]][0], b = q[order[k]][1];
                    tri[k][0] = a < b ? a : b; tri[k][1] = a < b ? b : a;
                }
                nt = 2;
            }
            if (nt) {
                int P[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};       // the first triangle's corners, doubled
                for (int k = 0; k < 3; ++k)
                    for (int ax = 0; ax < 3; ++ax) P[k][ax] = ((c[tri[k][0]] >> ax) & 1) + ((c[tri[k][1]] >> ax) & 1);
                const int u[3] = {P[1][0] - P[0][0], P[1][1] - P[0][1], P[1][2] - P[0][2]};
                const int v[3] = {P[2][0] - P[0][0], P[2][1] - P[0][1], P[2][2] - P[0][2]};
                const int n[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2], u[0] * v[1] - u[1] * v[0]};
                int dot = 0;
                for (int ax = 0; ax < 3; ++ax) dot += n[ax] * (P[0][ax] - 2 * ((c[in[0]] >> ax) & 1));
                if (dot < 0) {                                         // swap the last two corners of each triangle:
                    for (int t = 0; t < nt; ++t)                       // (q0,q1,q2),(q0,q2,q3) -> (q0,q2,q1),(q0,q3,q2)
                        for (int h = 0; h < 2; ++h) {
                            const int s = tri[3 * t + 1][h]; tri[3 * t + 1][h] = tri[3 * t + 2][h]; tri[3 * t + 2][h] = s;
                        }
                    if (nt == 2)                                       // ... and the quad's two triangles change places
                        for (int k = 0; k < 3; ++k)
                            for (int h = 0; h < 2; ++h) { const int s = tri[k][h]; tri[k][h] = tri[3 + k][h]; tri[3 + k][h] = s; }
                }
            }
            uint64_t w = (uint64_t)nt;
            for (int k = 0; k < 3 * nt; ++k) {
                const int owner = c[tri[k][0]], e = (c[tri[k][1]] ^ owner) - 1;
                w |= (uint64_t)(owner | (e << 3)) << (4 + 6 * k);
            }
            T.e[p * 16 + m] = w;
        }
    return T;
}
__constant__ TetTable g_tet = make_tet_table();

struct MeshBox {
    int64_t X, XY;                             // the held volume's row and plane
    int org[3], G[3], lo[3];                   // vol_origin, global extents, own_lo
    int64_t PX, PY, PXY, N;                    // the own point box: points per row, rows per plane, points per plane, in all
    int64_t step[3];                           // the grid stride, gridDim.x * M_WAVES * 64 points, as (x, y, z) of the point box
    int hi[3];                                 // own_hi
    int cap;
    float level;
};

// Where a wave's run begins in the point box, kept in scalars: one pair of divisions when the wave starts, carries after.
struct RunWalk {
    int64_t x, y, z;
    __device__ __forceinline__ void start(const MeshBox &b, int64_t n0)
    {
        z = n0 / b.PXY;
        const int64_t r = n0 - z * b.PXY;
        y = r / b.PX;
        x = r - y * b.PX;
    }
    __device__ __forceinline__ void advance(const MeshBox &b)      // by the grid stride: each part is below its extent
    {
        x += b.step[0];
        if (x >= b.PX) { x -= b.PX; ++y; }
        y += b.step[1];
        if (y >= b.PY) { y -= b.PY; ++z; }
        z += b.step[2];
    }
};

struct Point {
    int g[3];                                  // global lattice coordinates
    uint32_t valid8;                           // bit d: corner g + d lies in the point box
    uint32_t load8;                            // bit d: ... and in the volume (else the cap's virtual layer: v = 0)
    const uint8_t *at;                         // the point's voxel in the held volume (dereferenced only under load8)
};

// the point `lane` places after w in the point box
__device__ __forceinline__ Point point_of(const uint8_t *__restrict__ vol, const MeshBox &b, const RunWalk &w, int lane)
{
    Point p;
    if (w.x + 63 < b.PX) {                     // the run stays in its row (the same in the whole wave): y and z are scalars
        p.g[0] = b.lo[0] + (int)w.x + lane; p.g[1] = b.lo[1] + (int)w.y; p.g[2] = b.lo[2] + (int)w.z;
        const int64_t row = (int64_t)(p.g[2] - b.org[2]) * b.XY + (int64_t)(p.g[1] - b.org[1]) * b.X + (b.lo[0] + w.x - b.org[0]);
        p.at = vol + row + lane;
    } else {
        uint32_t x = (uint32_t)w.x + (uint32_t)lane, y = (uint32_t)w.y, z = (uint32_t)w.z;
        const uint32_t PX = (uint32_t)b.PX, PY = (uint32_t)b.PY;
        if (x >= PX) {
            const uint32_t q = x / PX;
            x -= q * PX; y += q;
            if (y >= PY) { const uint32_t q2 = y / PY; y -= q2 * PY; z += q2; }
        }
        p.g[0] = b.lo[0] + (int)x; p.g[1] = b.lo[1] + (int)y; p.g[2] = b.lo[2] + (int)z;
        p.at = vol + ((int64_t)(p.g[2] - b.org[2]) * b.XY + (int64_t)(p.g[1] - b.org[1]) * b.X + (p.g[0] - b.org[0]));
    }
    // per axis: the corners that stay (bit pattern of d_k = 0) are fine, those that step need room below own_hi ...
    p.valid8 = (0x55u | (p.g[0] < b.hi[0] ? 0xAAu : 0u)) & (0x33u | (p.g[1] < b.hi[1] ? 0xCCu : 0u))
               & (0x0Fu | (p.g[2] < b.hi[2] ? 0xF0u : 0u));
    // ... and a corner is a voxel where all three of its coordinates are inside the volume
    const uint32_t ix = ((unsigned)p.g[0] < (unsigned)b.G[0] ? 0x55u : 0u) | ((unsigned)(p.g[0] + 1) < (unsigned)b.G[0] ? 0xAAu : 0u);
    const uint32_t iy = ((unsigned)p.g[1] < (unsigned)b.G[1] ? 0x33u : 0u) | ((unsigned)(p.g[1] + 1) < (unsigned)b.G[1] ? 0xCCu : 0u);
    const uint32_t iz = ((unsigned)p.g[2] < (unsigned)b.G[2] ? 0x0Fu : 0u) | ((unsigned)(p.g[2] + 1) < (unsigned)b.G[2] ? 0xF0u : 0u);
    p.load8 = p.valid8 & ix & iy & iz;
    return p;
}

// v(q) for the gradients' neighbours: 0 outside the volume; an in-volume q the entry point's check has proved held
__device__ __forceinline__ int voxel(const uint8_t *__restrict__ vol, const MeshBox &b, int x, int y, int z)
{
    if ((unsigned)x >= (unsigned)b.G[0] || (unsigned)y >= (unsigned)b.G[1] || (unsigned)z >= (unsigned)b.G[2]) return 0;
    return vol[(int64_t)(z - b.org[2]) * b.XY + (int64_t)(y - b.org[1]) * b.X + (x - b.org[0])];
}

// v^(q) of the gradients: clamped without cap, zero-extended with it
__device__ __forceinline__ int voxel_hat(const uint8_t *__restrict__ vol, const MeshBox &b, int x, int y, int z)
{
    if (!b.cap) {
        x = std::min(std::max(x, 0), b.G[0] - 1); y = std::min(std::max(y, 0), b.G[1] - 1); z = std::min(std::max(z, 0), b.G[2] - 1);
    }
    return voxel(vol, b, x, y, z);
}

__device__ __forceinline__ void gradient_at(const uint8_t *__restrict__ vol, const MeshBox &b, int x, int y, int z, float g[3])
{
    g[0] = (float)(voxel_hat(vol, b, x + 1, y, z) - voxel_hat(vol, b, x - 1, y, z));
    g[1] = (float)(voxel_hat(vol, b, x, y + 1, z) - voxel_hat(vol, b, x, y - 1, z));
    g[2] = (float)(voxel_hat(vol, b, x, y, z + 1) - voxel_hat(vol, b, x, y, z - 1));
}

// the 8 corner values of the point's cube (0 for a corner that is not the call's, or on the cap's virtual layer) and
// their inside mask.  A point of the own point box that lies in the volume is a held voxel (the entry points' check).
__device__ __forceinline__ uint32_t corners(const MeshBox &b, const Point &p, int v[8])
{
    uint32_t m8 = 0;
#pragma unroll
    for (int d = 0; d < 8; ++d) {
        v[d] = (p.load8 >> d) & 1u ? p.at[(d & 1) + ((d >> 1) & 1) * b.X + (d >> 2) * b.XY] : 0;
        m8 |= ((float)v[d] >= b.level ? 1u : 0u) << d;
    }
    return m8;
}

// the crossing edges the point owns: bit e for the edge to corner e + 1
__device__ __forceinline__ uint32_t edge_mask(uint32_t m8, uint32_t valid8)
{
    return (((m8 & 1u) ? ~m8 : m8) & valid8 & 0xFFu) >> 1;
}

// the triangles of the cell with inside mask m8: per tetrahedron 0 (0 or 4 corners inside), 1 (1 or 3) or 2 (2)
__device__ __forceinline__ uint32_t cell_triangles(uint32_t m8)
{
    if (m8 == 0u || m8 == 0xFFu) return 0u;
    const uint32_t ends = (m8 & 1u) + (m8 >> 7);
    uint32_t n = 0;
#pragma unroll
    for (int p = 0; p < 6; ++p) {
        const uint32_t pc = ends + ((m8 >> TET_A1[p]) & 1u) + ((m8 >> TET_A2[p]) & 1u);
        n += (pc & 1u) ? 1u : (pc & 2u);
    }
    return n;
}

// exclusive prefix and total over the wave of a count of BITS bits; every lane of the wave calls it
template <int BITS>
__device__ __forceinline__ void wave_prefix(uint32_t v, int lane, uint32_t &prefix, uint32_t &total)
{
    const unsigned long long below = (1ull << lane) - 1ull;
    prefix = 0; total = 0;
#pragma unroll
    for (int k = 0; k < BITS; ++k) {
        const unsigned long long bal = __ballot((v >> k) & 1u);
        prefix += (uint32_t)__popcll(bal & below) << k;
        total += (uint32_t)__popcll(bal) << k;
    }
}

__global__ void __launch_bounds__(M_THREADS)
k_mesh_count(const uint8_t *__restrict__ vol, MeshBox b, int64_t runs, uint16_t *__restrict__ words, uint32_t *__restrict__ vrun,
             uint32_t *__restrict__ trun)
{
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int64_t run = (int64_t)blockIdx.x * M_WAVES + wave;            // (a scalar: the whole wave stays or leaves)
    if (run >= runs) return;
    RunWalk w;
    w.start(b, run * 64);
    for (; run < runs; run += (int64_t)gridDim.x * M_WAVES, w.advance(b)) {
        const int64_t n = run * 64 + lane;
        uint32_t mask = 0, tris = 0;
        if (n < b.N) {
            const Point p = point_of(vol, b, w, lane);
            int v[8];
            const uint32_t m8 = corners(b, p, v);
            mask = edge_mask(m8, p.valid8);
            if (p.valid8 & 0x80u) tris = cell_triangles(m8);
        }
        uint32_t vpre, vtot, tpre, ttot;
        wave_prefix<3>((uint32_t)__popc(mask), lane, vpre, vtot);
        wave_prefix<4>(tris, lane, tpre, ttot);
        if (n < b.N) words[n] = (uint16_t)((vpre << 7) | mask);
        if (lane == 0) { vrun[run] = vtot; trun[run] = ttot; }
    }
}

// exclusive scan over the workgroup of (a, b); returns the workgroup's sums in (sa, sb)
template <class T, int THREADS>
__device__ __forceinline__ void block_scan2(T &a, T &b, T &sa, T &sb, T (*buf)[THREADS])
{
    const int t = (int)threadIdx.x;
    T ia = a, ib = b;                          // inclusive
    buf[0][t] = ia; buf[1][t] = ib;
    __syncthreads();
    for (int s = 1; s < THREADS; s <<= 1) {
        T xa = 0, xb = 0;
        if (t >= s) { xa = buf[0][t - s]; xb = buf[1][t - s]; }
        __syncthreads();
        ia += xa; ib += xb;
        buf[0][t] = ia; buf[1][t] = ib;
        __syncthreads();
    }
    sa = buf[0][THREADS - 1]; sb = buf[1][THREADS - 1];
    a = ia - a; b = ib - b;
    __syncthreads();                           // buf may be reused
}

__global__ void __launch_bounds__(M_THREADS)
k_mesh_scan1(int64_t runs, uint32_t *__restrict__ vrun, uint32_t *__restrict__ trun, unsigned long long *__restrict__ top)
{
    __shared__ uint32_t buf[2][M_THREADS];
    const int64_t r0 = ((int64_t)blockIdx.x * M_THREADS + threadIdx.x) * 4;
    uint32_t v[4], t[4], sv = 0, st = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        v[k] = r0 + k < runs ? vrun[r0 + k] : 0u; t[k] = r0 + k < runs ? trun[r0 + k] : 0u;
        sv += v[k]; st += t[k];
    }
    uint32_t totv, tott;
    block_scan2<uint32_t, M_THREADS>(sv, st, totv, tott, buf);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (r0 + k < runs) { vrun[r0 + k] = sv; trun[r0 + k] = st; }
        sv += v[k]; st += t[k];
    }
    if (threadIdx.x == 0) { top[2 * (int64_t)blockIdx.x] = totv; top[2 * (int64_t)blockIdx.x + 1] = tott; }
}

// top: `groups` pairs (vertices, triangles) -> exclusive prefixes in place; totals[0..1] = the grand totals
__global__ void __launch_bounds__(M_TOP_THREADS)
k_mesh_scan2(int64_t groups, unsigned long long *__restrict__ top, unsigned long long *__restrict__ totals)
{
    __shared__ unsigned long long buf[2][M_TOP_THREADS];
    unsigned long long cv = 0, ct = 0;         // the carry: the same in every thread
    for (int64_t first = 0; first < groups; first += M_TOP_THREADS) {
        const int64_t g = first + threadIdx.x;
        unsigned long long a = g < groups ? top[2 * g] : 0ull, c = g < groups ? top[2 * g + 1] : 0ull, sa, sc;
        block_scan2<unsigned long long, M_TOP_THREADS>(a, c, sa, sc, buf);
        if (g < groups) { top[2 * g] = cv + a; top[2 * g + 1] = ct + c; }
        cv += sa; ct += sc;
    }
    if (threadIdx.x == 0) { totals[0] = cv; totals[1] = ct; }
}

__global__ void __launch_bounds__(M_THREADS)
k_mesh_add(int64_t runs, uint32_t *__restrict__ vrun, uint32_t *__restrict__ trun, const unsigned long long *__restrict__ top)
{
    const int64_t r = (int64_t)blockIdx.x * M_THREADS + threadIdx.x;
    if (r >= runs) return;
    const int64_t g = r / M_SCAN_RUNS;
    vrun[r] += (uint32_t)top[2 * g]; trun[r] += (uint32_t)top[2 * g + 1];
}

__device__ __forceinline__ uint32_t select8(const uint32_t a[8], uint32_t k)
{
    const uint32_t l0 = (k & 1u) ? a[1] : a[0], l1 = (k & 1u) ? a[3] : a[2], l2 = (k & 1u) ? a[5] : a[4], l3 = (k & 1u) ? a[7] : a[6];
    const uint32_t m0 = (k & 2u) ? l1 : l0, m1 = (k & 2u) ? l3 : l2;
    return (k & 4u) ? m1 : m0;
}

// one run of k_mesh_emit, by one wave
template <bool GRAD>
__device__ __forceinline__ void emit_run(const uint8_t *__restrict__ vol, const MeshBox &b, int64_t run, const RunWalk &w, int lane,
                                         const uint16_t *__restrict__ words, const uint32_t *__restrict__ vrun,
                                         const uint32_t *__restrict__ trun, uint32_t nv, uint32_t nt, float *__restrict__ pos,
                                         float *__restrict__ grad, uint32_t *__restrict__ idx)
{
    const int64_t n = run * 64 + lane;
    uint32_t mask = 0, tris = 0, m8 = 0;
    Point p = {};
    int v[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    if (n < b.N) {
        p = point_of(vol, b, w, lane);
        m8 = corners(b, p, v);
        mask = edge_mask(m8, p.valid8);
        if (p.valid8 & 0x80u) tris = cell_triangles(m8);
    }
    uint32_t vpre, vtot, tpre, ttot;
    wave_prefix<3>((uint32_t)__popc(mask), lane, vpre, vtot);
    wave_prefix<4>(tris, lane, tpre, ttot);
    if (vtot == 0u) return;                    // no vertex in the run: no triangle either (the same in the whole wave)

    if (mask) {
        uint32_t vi = vrun[run] + vpre;
        float ga[3] = {0.0f, 0.0f, 0.0f};
        if (GRAD) gradient_at(vol, b, p.g[0], p.g[1], p.g[2], ga);
        const float va = (float)v[0];
#pragma unroll
        for (int e = 0; e < 7; ++e) {
            if (!((mask >> e) & 1u)) continue;
            const int d = e + 1;
            const float t = (b.level - va) / ((float)v[d] - va);
            if (vi < nv) {
                float *o = pos + 3 * (int64_t)vi;
                o[0] = (float)p.g[0] + ((d & 1) ? t : 0.0f);
                o[1] = (float)p.g[1] + ((d & 2) ? t : 0.0f);
                o[2] = (float)p.g[2] + ((d & 4) ? t : 0.0f);
                if (GRAD) {
                    float gb[3];
                    gradient_at(vol, b, p.g[0] + (d & 1), p.g[1] + ((d >> 1) & 1), p.g[2] + (d >> 2), gb);
                    float *og = grad + 3 * (int64_t)vi;
                    og[0] = ga[0] + t * (gb[0] - ga[0]);
                    og[1] = ga[1] + t * (gb[1] - ga[1]);
                    og[2] = ga[2] + t * (gb[2] - ga[2]);
                }
            }
            ++vi;
        }
    }

    if (tris) {
        // the eight owner points of the cell's edges: each one's 7-bit mask and the index of its first vertex
        uint32_t base[8];
        unsigned long long masks = 0;
#pragma unroll
        for (int d = 0; d < 8; ++d) {
            const int64_t q = n + (d & 1) + ((d >> 1) & 1) * b.PX + (d >> 2) * b.PXY;      // in the point box: the cell is owned
            const uint32_t w = words[q];
            base[d] = vrun[q >> 6] + (w >> 7);
            masks |= (unsigned long long)(w & 127u) << (7 * d);
        }
        uint32_t ti = trun[run] + tpre;
        const uint32_t ends = (m8 & 1u) | ((m8 >> 4) & 8u);
#pragma unroll 1
        for (int pi = 0; pi < 6; ++pi) {
            const int a1 = pi >> 1 == 0 ? 1 : (pi >> 1 == 1 ? 2 : 4);
            const int a2 = pi == 0 || pi == 2 ? 3 : (pi == 1 || pi == 4 ? 5 : 6);
            const uint32_t m4 = ends | (((m8 >> a1) & 1u) << 1) | (((m8 >> a2) & 1u) << 2);
            unsigned long long w = g_tet.e[pi * 16 + (int)m4];
            const int cnt = (int)(w & 3ull);
            w >>= 4;
            for (int k = 0; k < cnt; ++k) {
                uint32_t c[3];
#pragma unroll
                for (int j = 0; j < 3; ++j) {
                    const uint32_t code = (uint32_t)w & 63u, owner = code & 7u, e = code >> 3;
                    w >>= 6;
                    const uint32_t om = (uint32_t)(masks >> (7u * owner)) & 127u;
                    c[j] = select8(base, owner) + (uint32_t)__popc(om & ((1u << e) - 1u));
                }
                if (ti < nt) {
                    uint32_t *o = idx + 3 * (int64_t)ti;
                    o[0] = c[0]; o[1] = c[1]; o[2] = c[2];
                }
                ++ti;
            }
        }
    }
}

template <bool GRAD>
__global__ void __launch_bounds__(M_THREADS)
k_mesh_emit(const uint8_t *__restrict__ vol, MeshBox b, int64_t runs, const uint16_t *__restrict__ words,
            const uint32_t *__restrict__ vrun, const uint32_t *__restrict__ trun, uint32_t nv, uint32_t nt,
            float *__restrict__ pos, float *__restrict__ grad, uint32_t *__restrict__ idx)
{
    const int lane = (int)threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    int64_t run = (int64_t)blockIdx.x * M_WAVES + wave;            // (a scalar: the whole wave stays or leaves)
    if (run >= runs) return;
    RunWalk w;
    w.start(b, run * 64);
    for (; run < runs; run += (int64_t)gridDim.x * M_WAVES, w.advance(b))
        emit_run<GRAD>(vol, b, run, w, lane, words, vrun, trun, nv, nt, pos, grad, idx);
}

// ---- host ------------------------------------------------------------------------------------------------------------
struct MeshPlan {
    MeshBox box;
    int64_t runs, groups;                      // 0 for an empty box
    unsigned grid;                             // of the per-point kernels
    size_t offVrun, offTrun, offTop, offTotals, bytes;
};

static size_t up16(size_t n) { return (n + 15u) & ~(size_t)15u; }

// every check of the three entry points that needs no device; grads: the held voxels must reach one point further
static vr_status mesh_plan(const int64_t dims[3], const vr_isomesh_desc *d, bool grads, MeshPlan &pl)
{
    if (!dims || !d) return VR_ERR_INVALID;
    if (d->cap != 0 && d->cap != 1) return VR_ERR_INVALID;
    if (!std::isfinite(d->iso_value)) return VR_ERR_INVALID;
    MeshBox &b = pl.box;
    int64_t P[3];
    bool empty = false;
    for (int k = 0; k < 3; ++k) {
        if (dims[k] <= 0 || dims[k] >= (1ll << 31) || d->global_dims[k] < 0 || d->global_dims[k] >= (1ll << 31)) return VR_ERR_INVALID;
        const int64_t G = d->global_dims[k] ? d->global_dims[k] : dims[k], o = d->vol_origin[k], end = o + dims[k];
        if (o < 0 || end > G) return VR_ERR_INVALID;                                   // the local volume lies in the global one
        const int64_t lo = d->own_lo[k], hi = d->own_hi[k], g = grads ? 1 : 0;
        if (lo > hi || lo < (d->cap ? -1 : 0) || hi > (d->cap ? G : G - 1)) return VR_ERR_INVALID;
        if (std::max<int64_t>(lo - g, 0) < o || std::min<int64_t>(hi + g, G - 1) > end - 1) return VR_ERR_INVALID;     // not held
        b.org[k] = (int)o; b.G[k] = (int)G; b.lo[k] = (int)lo; b.hi[k] = (int)hi;
        P[k] = hi - lo + 1;
        empty = empty || lo == hi;
    }
    b.X = dims[0]; b.XY = dims[0] * dims[1];
    b.cap = d->cap;
    b.level = d->iso_value * 255.0f;
    b.PX = P[0]; b.PY = P[1]; b.PXY = P[0] * P[1];
    // more than 2^36 points: no device holds their workspace, and the scans' grids stay far below 2^32 threads
    if (!empty && P[2] > (1ll << 36) / b.PXY) return VR_ERR_UNSUPPORTED;
    b.N = empty ? 0 : P[0] * P[1] * P[2];
    pl.runs = (b.N + 63) / 64;
    pl.grid = (unsigned)std::min<int64_t>((pl.runs + M_WAVES - 1) / M_WAVES, M_MAX_GRID);
    const int64_t stride = (int64_t)pl.grid * M_WAVES * 64;      // in points; split as RunWalk::advance adds it
    b.step[2] = stride / b.PXY; b.step[1] = stride % b.PXY / b.PX; b.step[0] = stride % b.PXY % b.PX;
    pl.groups = (pl.runs + M_SCAN_RUNS - 1) / M_SCAN_RUNS;
    pl.offVrun = up16((size_t)b.N * 2);
    pl.offTrun = pl.offVrun + up16((size_t)pl.runs * 4);
    pl.offTop = pl.offTrun + up16((size_t)pl.runs * 4);
    pl.offTotals = pl.offTop + (size_t)pl.groups * 16;
    pl.bytes = pl.offTotals + 16;
    return VR_OK;
}

static bool have_device()
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess && n > 0;
}

} // namespace vr

using namespace vr;

extern "C" {

vr_status vr_isomesh_workspace_bytes(const int64_t dims[3], const vr_isomesh_desc *desc, int64_t *bytes)
{
    if (!bytes) return VR_ERR_INVALID;
    MeshPlan pl;
    const vr_status s = mesh_plan(dims, desc, false, pl);
    if (s != VR_OK) return s;
    *bytes = (int64_t)pl.bytes;
    return VR_OK;
}

vr_status vr_isomesh_count(const uint8_t *vol, const int64_t dims[3], const vr_isomesh_desc *desc, void *workspace,
                           uint64_t counts_host[2], void *stream)
{
    if (!vol || !workspace || !counts_host || ((uintptr_t)workspace & 15u) != 0) return VR_ERR_INVALID;
    MeshPlan pl;
    const vr_status s = mesh_plan(dims, desc, false, pl);
    if (s != VR_OK) return s;
    if (!have_device()) return VR_ERR_NO_DEVICE;
    hipStream_t st = (hipStream_t)stream;
    counts_host[0] = counts_host[1] = 0;
    if (pl.runs > 0) {
        uint8_t *ws = (uint8_t *)workspace;
        uint16_t *words = (uint16_t *)ws;
        uint32_t *vrun = (uint32_t *)(ws + pl.offVrun), *trun = (uint32_t *)(ws + pl.offTrun);
        unsigned long long *top = (unsigned long long *)(ws + pl.offTop), *totals = (unsigned long long *)(ws + pl.offTotals);
        hipLaunchKernelGGL(k_mesh_count, dim3(pl.grid), dim3(M_THREADS), 0, st, vol, pl.box, pl.runs, words, vrun, trun);
        if (g_meshCountOnly.load() != 0) {     // the per-point pass alone, for mesh_bench.py to price the scans: no counts
            const int rc0 = launch_status("mesh_count");
            return hipStreamSynchronize(st) != hipSuccess || rc0 != 0 ? VR_ERR_NO_DEVICE : VR_OK;
        }
        hipLaunchKernelGGL(k_mesh_scan1, dim3((unsigned)pl.groups), dim3(M_THREADS), 0, st, pl.runs, vrun, trun, top);
        hipLaunchKernelGGL(k_mesh_scan2, dim3(1), dim3(M_TOP_THREADS), 0, st, pl.groups, top, totals);
        hipLaunchKernelGGL(k_mesh_add, dim3((unsigned)((pl.runs + M_THREADS - 1) / M_THREADS)), dim3(M_THREADS), 0, st, pl.runs,
                           vrun, trun, top);
        int rc = launch_status("mesh_count");
        if (rc == 0 && hipMemcpyAsync(counts_host, totals, 16, hipMemcpyDeviceToHost, st) != hipSuccess) rc = 1;
        if (hipStreamSynchronize(st) != hipSuccess || rc != 0) return VR_ERR_NO_DEVICE;
    } else if (hipStreamSynchronize(st) != hipSuccess) {
        return VR_ERR_NO_DEVICE;
    }
    if (counts_host[0] > VR_ISOMESH_MAX_VERTICES || counts_host[1] > VR_ISOMESH_MAX_TRIANGLES) return VR_ERR_UNSUPPORTED;
    return VR_OK;
}

vr_status vr_isomesh_emit(const uint8_t *vol, const int64_t dims[3], const vr_isomesh_desc *desc, const void *workspace,
                          int64_t num_vertices, int64_t num_triangles, float *positions, float *gradients, uint32_t *indices,
                          void *stream)
{
    if (!vol || !workspace || ((uintptr_t)workspace & 15u) != 0) return VR_ERR_INVALID;
    if (num_vertices < 0 || num_vertices > (int64_t)VR_ISOMESH_MAX_VERTICES || num_triangles < 0
        || num_triangles > (int64_t)VR_ISOMESH_MAX_TRIANGLES)
        return VR_ERR_INVALID;
    if ((num_vertices > 0 && !positions) || (num_triangles > 0 && !indices)) return VR_ERR_INVALID;
    if ((((uintptr_t)positions | (uintptr_t)gradients | (uintptr_t)indices) & 3u) != 0) return VR_ERR_INVALID;
    MeshPlan pl;
    const vr_status s = mesh_plan(dims, desc, gradients != nullptr, pl);
    if (s != VR_OK) return s;
    if (!have_device()) return VR_ERR_NO_DEVICE;
    if ((num_vertices == 0 && num_triangles == 0) || pl.runs == 0) return VR_OK;
    hipStream_t st = (hipStream_t)stream;
    const uint8_t *ws = (const uint8_t *)workspace;
    const uint16_t *words = (const uint16_t *)ws;
    const uint32_t *vrun = (const uint32_t *)(ws + pl.offVrun), *trun = (const uint32_t *)(ws + pl.offTrun);
    if (gradients)
        hipLaunchKernelGGL(k_mesh_emit<true>, dim3(pl.grid), dim3(M_THREADS), 0, st, vol, pl.box, pl.runs, words, vrun, trun,
                           (uint32_t)num_vertices, (uint32_t)num_triangles, positions, gradients, indices);
    else
        hipLaunchKernelGGL(k_mesh_emit<false>, dim3(pl.grid), dim3(M_THREADS), 0, st, vol, pl.box, pl.runs, words, vrun, trun,
                           (uint32_t)num_vertices, (uint32_t)num_triangles, positions, gradients, indices);
    return launch_status("mesh_emit") == 0 ? VR_OK : VR_ERR_NO_DEVICE;
}

} // extern "C"
